// est_push.h — Estimator::PushFrame's device work (Estimator.cc:62-103 TransformToEnd, :678-693 pcl::VoxelGrid of the new sweep) and
// SlideWindow's (:2602-2615) for the windows of a batch, one launch per stage over all of them (include/lio_est_push_batch.h).
//
// The push chain works on CLOUDS, not windows: a window contributes its surf cloud and, with the map refresh on, its corner cloud.  Every
// cloud has one record in device memory (one table upload per call) and a 256-aligned range of the chain's arrays:
//
//   uploads                      host clouds -> one staging array, at the records' offsets, no wait in between
//   k_bp_take_keys               (blocks of the largest cloud, clouds): de-skew where the record says so, the point to the chain's input
//                                array, its voxel key (absolute cells) and the block's share of the bounds
//   k_bp_key_layout              one block per cloud: bounds -> VoxParams, how the sort sees the keys
//   seg_sort_passes              one segment per cloud, three or four 9-bit passes
//   k_bp_vox_heads / _centroids  run heads per tile, centroids straight into the HANDLE's stack buffer; the last tile posts count, bounds, flag
//   one copy, one host wait
//
// The arithmetic is cloud_device.h's, which the single-window filter (VoxelGridDev) and the batched solve's local maps run too: the
// centroids of a cloud are the same bits alone and in any batch.  A cloud the chain cannot take (keys beyond the absolute range or beyond
// what the passes order, PCL's "leaf size too small") is flagged and left to the handle's own VoxelGridDev.
#pragma once
#include <vector>

#include "batch_kernels.h"
#include "cloud_kernels.h"
#include "seg_sort.h"

namespace lio {

struct BpCloud {
  int src_off;            // first point of the cloud in the staging array (the "source": where a later device-fed form plugs in)
  int n, off, cap;        // points; the cloud's range of the chain's arrays (off, cap multiples of 256, cap >= max(n, 1))
  float inv_leaf;
  int deskew;             // TransformToEnd by (qe, te, time_factor) in front of the filter
  float qe[4], te[3];     // qx qy qz qw
  float time_factor;
  float4 *dst;            // the handle's buffer the centroids go to (room for n points)
};
// what the chain reports per cloud (read by the host behind the call's one wait); flagged: keys beyond the range or the passes
struct BpVoxOut { int count; VoxParams params; int flagged; };

// SlideWindow of one window: the two segments of Estimator.cc:2602-2615 into the handle's scratch cloud
struct BpSlide {
  BwSeg seg[2];
  int total;
  float4 *dst;
};

// the chain's launches (no host wait; `flag`: one int per cloud, zero between calls — the centroids' last tile clears it)
void launch_bp_take_keys(const BpCloud *rec, int nclouds, int max_n, const float4 *staging, float4 *in_all, uint32_t *keys, float *partial, VoxParams *params,
                         KeyLayout *layout, int *flag, int max_bits, hipStream_t s);
void launch_bp_vox_finish(const BpCloud *rec, int nclouds, int max_cap, const float4 *in_all, const uint32_t *keys_sorted, const uint32_t *vals_sorted, int *tile_heads,
                          const VoxParams *params, int *flag, BpVoxOut *out, hipStream_t s);
void launch_bp_slide(const BpSlide *rec, int nwin, int max_total, hipStream_t s);

// The chain's arrays and tables; owned by an EstimatorBatch (one per part), sized by the largest call so far.
class PushChain {
 public:
  // a call: begin(), add() per filtered cloud (host pointer; returns the cloud's index), run(), then out(i) / input(i)
  void begin(int max_clouds);
  int add(const float *host_xyzi, size_t n, float leaf, bool deskew, const float q[4], const float p[3], float time_factor, float4 *dst);
  int clouds() const { return n_; }
  // uploads, the launches, the read-back and the wait; passes: 3 or 4.  No cloud: nothing is enqueued and nothing waited for (returns false)
  bool run(int passes, hipStream_t s);
  const BpVoxOut &out(int i) const { return h_out_.p[i]; }
  const float4 *input(int i) const { return in_all_.p + h_rec_.p[i].off; }   // the cloud as the filter read it: staged, de-skewed

 private:
  std::vector<const float *> src_;
  HostBuf<BpCloud> h_rec_; HostBuf<BpVoxOut> h_out_; HostBuf<SegDesc> h_seg_;
  DBuf<BpCloud> d_rec_; DBuf<BpVoxOut> d_out_; DBuf<SegDesc> d_seg_;
  DBuf<KeyLayout> d_layout_; DBuf<VoxParams> d_params_;
  DBuf<int> d_flag_, tile_heads_;
  DBuf<float4> staging_, in_all_;
  DBuf<uint32_t> ckeys_, keys_, keysb_, vals_, valsb_, hist_;
  DBuf<float> partial_;
  int n_ = 0, cap_ = 0, total_ = 0, max_n_ = 0, max_cap_ = 0;
};

}  // namespace lio
