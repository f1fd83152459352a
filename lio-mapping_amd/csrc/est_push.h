// est_push.h — Estimator::PushFrame's device work (Estimator.cc:62-103 TransformToEnd, :678-693 pcl::VoxelGrid of the new sweep) and
// SlideWindow's (:2602-2615) for the windows of a batch, one launch per stage over all of them (include/lio_est_push_batch.h).
//
// The push chain works on CLOUDS, not windows: a window contributes its surf cloud and, with the map refresh on, its corner cloud.  Every
// cloud has one record in device memory (one table upload per call) and a 256-aligned range of the chain's arrays:
//
//   uploads                      host clouds -> one staging array, at the records' offsets, no wait in between
//   k_bp_take_keys               (blocks of the largest cloud, clouds): de-skew where the record says so, the point to the chain's input
//                                array, its voxel key (absolute cells) and the block's share of the bounds
//   SegVoxFilter::finish         seg_vox.h, the filter the batched solve's local maps run too: key layout, segmented sort, run heads, centroids
//                                straight into the HANDLE's stack buffer, one copy of the output table
//   one host wait
//
// Device-fed form (include/lio_est_from_odom.h): a cloud whose points already lie in device memory (an odometry's last_corner_ / last_surf_) has
// its pointer in the record and no range of the staging array; k_bp_take_keys_dev reads it where it lies, and the same launch writes the full
// clouds of the call (cloud_kernels.h: FullTake, a processor's ring cloud through the odometry's TransformToEnd into a map's full cloud).
//
// The filter is the EstimatorBatch's one SegVoxFilter; what is the chain's own is here: the staging and input arrays, the records, the uploads.
// A cloud the filter cannot take (keys beyond the absolute range or beyond what the passes order, PCL's "leaf size too small") comes back
// flagged and is left to the handle's own VoxelGridDev, which reads input(i).
#pragma once
#include <vector>

#include "batch_kernels.h"
#include "cloud_kernels.h"
#include "cloud_src.h"
#include "seg_vox.h"

namespace lio {

struct BpCloud {
  int src_off;            // first point of the cloud in the staging array (the "source": where a later device-fed form plugs in)
  VoxSeg vox;             // the cloud's range of the chain's arrays; dst: the handle's buffer the centroids go to
  int deskew;             // TransformToEnd by (qe, te, time_factor) in front of the filter
  float qe[4], te[3];     // qx qy qz qw
  float time_factor;
  const float4 *src;      // the cloud where it lies in device memory (k_bp_take_keys_dev reads it there); null: staged at src_off
};

// SlideWindow of one window: the two segments of Estimator.cc:2602-2615 into the handle's scratch cloud
struct BpSlide {
  ConcatSeg seg[2];
  int total;
  float4 *dst;
};

// the chain's producer in front of SegVoxFilter::finish (no host wait; keys, partial, flag: the filter's)
void launch_bp_take_keys(const BpCloud *rec, int nclouds, int max_n, const float4 *staging, float4 *in_all, uint32_t *keys, float *partial, int *flag, hipStream_t s);
// the same with the clouds read from the records' device sources, and the full clouds behind them (grid rows nclouds .. nclouds + nfull - 1)
void launch_bp_take_keys_dev(const BpCloud *rec, int nclouds, const FullTake *full, int nfull, int max_n, float4 *in_all, uint32_t *keys, float *partial, int *flag,
                             hipStream_t s);
void launch_bp_slide(const BpSlide *rec, int nwin, int max_total, hipStream_t s);

// The chain's arrays and records; owned by an EstimatorBatch (one per part), sized by the largest call so far.
class PushChain {
 public:
  // a call: begin(), add() per filtered cloud (returns the cloud's index), add_full() per full cloud, run(), then vox.out(i) / input(i).  The
  // clouds of a call lie in one place (cloud_src.h), which begin() is told: the host's are staged and uploaded by run(), the device's are read
  // where they lie, and only a device-fed call takes full clouds.
  void begin(int max_clouds, int max_full = 0, bool device_fed = false);
  int add(CloudSrc src, float leaf, bool deskew, const float q[4], const float p[3], float time_factor, float4 *dst);
  void add_full(const FullTake &f);
  int clouds() const { return n_; }
  int uploads() const { return uploads_; }   // host-to-device copies of cloud data the last run() issued
  // uploads, the launches through vox.finish and the call's one wait; passes: 3 or 4.  No cloud and no full cloud: nothing is enqueued and
  // nothing waited for (returns false)
  bool run(SegVoxFilter &vox, int passes, hipStream_t s);
  const float4 *input(int i) const { return in_all_.p + h_rec_.p[i].vox.off; }   // the cloud as the filter read it: staged, de-skewed

 private:
  std::vector<const float4 *> src_;
  HostBuf<BpCloud> h_rec_;
  DBuf<BpCloud> d_rec_;
  HostBuf<FullTake> h_full_;
  DBuf<FullTake> d_full_;
  DBuf<float4> staging_, in_all_;
  int n_ = 0, cap_ = 0, total_ = 0, max_n_ = 0, staged_ = 0, nfull_ = 0, cap_full_ = 0, uploads_ = 0;
  bool device_fed_ = false;
};

}  // namespace lio
