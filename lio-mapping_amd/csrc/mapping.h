// mapping.h — PointMapping (LOAM scan-to-map step + cube map) on the GPU.
// Reference: src/point_processor/PointMapping.cc:303-323 (point association), :325-753 (OptimizeTransformTobeMapped),
// :755-763 (TransformAssociateToMap / TransformUpdate), :765-1110 (Process), :1112-1208 (UpdateMapDatabase).
//
// MI355X-first layout: instead of 2 x 4851 per-cube clouds the map of one feature class is ONE device pool of
// float4 points plus a packed absolute cube key per point.  A cube's cloud is the subsequence of the pool with
// its key (pool order == the reference's per-cube order).  Shifting the 21x21x11 window only changes which keys
// are inside it; extracting the FOV cubes is one 8-bit radix pass + gather that leaves the pool as
// [rest | valid cubes in valid_idx order], so laser_cloud_*_from_map_ is a contiguous tail of the pool; the per-cube
// VoxelGrid of UpdateMapDatabase is ONE segmented voxel pass with 64-bit (cube rank, voxel) keys.
//
// One route steps a handle: ProcessBatch drives a MapChain (mapping.hip) through prepare, filter, grids, table, rounds, give back and
// update for all handles of a call, and Process is ProcessBatch of the handle alone.  The Gauss-Newton rounds are the keyframe chain of
// cloud_kernels.h on a table of the call's iterating sensors; the host reads convergence and the final states from per-sensor mailboxes.
#pragma once
#include <memory>
#include <vector>

#include "../../include/lio_c.h"
#include "cloud_kernels.h"
#include "cloud_src.h"
#include "hmath.h"
#include "seg_sort.h"

namespace lio {

#define LIO_MAP_MAX_VALID 125
#define LIO_MAP_RANK_REST 254u
#define LIO_MAP_RANK_DROP 255u

struct MapValidSet {
  uint32_t key[LIO_MAP_MAX_VALID];  // packed absolute cube keys, ascending == valid_idx order (i-major)
  int n;
  int lo[3], hi[3];                 // absolute cube range [lo, hi) of the current 21x21x11 window
};

// the 5x5x5 surround of the last Process (PointMapping.cc:927,984) as packed absolute cube keys; ascending == list order (i-major)
struct MapSurroundSet {
  uint32_t key[LIO_MAP_MAX_VALID];
  int n;
};
#define LIO_MAP_SURROUND_DROP 255u   // bin of a point outside the surround; kept points have bin 2 * slot + class (< 250)

struct MapCounters { int n_valid, n_rest, n_new_valid, n_new_rest, n_out, pad[3]; };

// The full cloud a handle takes with a step whose clouds lie in device memory (lio_map_process_batch_from_odom): what SetFullCloud does, fed from
// the device.  Only such a step takes one.
struct MapFullSource {
  bool set;                  // false: the handle's full cloud stays as it is
  const float4 *pts;         // n points in the sensor frame at their own times, in device memory; n = 0 clears the handle's full cloud
  size_t n;
  ToEnd to_end;              // the odometry's TransformToEnd the points go through on the way (cloud_kernels.h; st null: a copy)
};
// One sensor's sweep as the scan-to-scan odometry hands it on, to a map (ProcessBatch) or to a window of the estimator (est_batch.h): the
// last corner and surf clouds, host or device (cloud_src.h), its transform_sum_, and the full cloud that goes with them.
struct OdomSweep { CloudSrc corner, surf; Rigid<float> transform_sum; MapFullSource full; };

struct MapChain;   // mapping.hip: the launch chain every step runs through (prepare, filter, grids, table, rounds, give back, update) and its scratch

class MappingDev {
 public:
  static constexpr int L = 21, Wd = 21, H = 11;  // laser_cloud_length_/width_/height_ (PointMapping.cc:79-81)

  explicit MappingDev(const lio_map_config &cfg);
  ~MappingDev();
  MappingDev(const MappingDev &) = delete;
  MappingDev &operator=(const MappingDev &) = delete;

  // ProcessBatch of this handle alone
  void Process(const float *corner_last, size_t n_corner, const float *surf_last, size_t n_surf, const Rigid<float> &transform_sum);
  // include/lio_map_batch.h: one sweep for each of n distinct handles, with the steps of the chain lined up across the handles and the rounds
  // of all of them in one keyframe table.  Array k of every argument belongs to m[k].  Every handle ends in the state a chain of one leaves,
  // bit for bit.  Handles without common launch parameters run as chains of one.  Returns synchronised (the full cloud's registration too).
  // sweep[k] is m[k]'s; the clouds of a call lie in one place (cloud_src.h).  The device's (include/lio_map_from_odom.h): one launch takes
  // them and every sweep[k].full, no copy per handle.
  static void ProcessBatch(MappingDev *const *m, int n, const OdomSweep *sweep);
  void UpdateMapDatabase(const float *corner_ds, size_t n_corner, const float *surf_ds, size_t n_surf, const uint32_t *valid_idx, size_t n_valid,
                         const Rigid<float> &T, const int cube_center[3]);
  // the same with the stacks where they live (HBM, sensor frame): no cloud crosses PCIe.  producer: the stream that wrote them (the
  // update waits for it through an event; nullptr: they are complete).  Returns after the update has read them.
  void UpdateMapDatabase(const float4 *d_corner_ds, size_t n_corner, const float4 *d_surf_ds, size_t n_surf, const uint32_t *valid_idx, size_t n_valid,
                         const Rigid<float> &T, const int cube_center[3], hipStream_t producer);
  // laser_cloud_surround_downsampled_ (PointMapping.cc:1223-1234): the cubes of surround_idx_ in list order, corner then surf points
  // of each, through the VoxelGrid at `leaf`.  Returns the count; copies the points when out != nullptr.  0 before the first Process.
  size_t GetSurround(float leaf, float *out);
  size_t GetCloud(int which, float *out);
  // full_cloud_ (PointMapping.cc:212-224): the full-resolution sweep, sensor frame until a Process with the init flag off has mapped it
  // in place with the transform_tobe_mapped_ it ended with (PublishResults, :1244-1248) — once per set.  n = 0 clears it.
  void SetFullCloud(const float *xyzi, size_t n);
  // SetFullCloud with the points written by the caller, on the stream `writer`: the handle's side of it (FullBegin), the wait for a reader of
  // the old cloud on another stream, and where the n points go (null: n = 0, the cloud is cleared).  The caller returns synchronised.
  float4 *FullTake(size_t n, hipStream_t writer);
  size_t GetFullCloud(float *out);
  const float4 *FullDevice() const { return full_.p; }
  size_t FullSize() const { return n_full_; }
  void FullWaitOn(hipStream_t consumer);
  void FullReadBy(hipStream_t consumer);
  hipStream_t stream() const { return stream_; }
  size_t GetCube(int cls, uint32_t cube_idx, float *out);
  size_t GetScorePointCoeff(float *score, float *point, float *coeff);
  // laser_cloud_{corner,surf}_stack_downsampled_ where they live (HBM), for the estimator's pre-initialisation pushes
  const float4 *StackDevice(int cls) const { return cls_[cls].stack_ds.p; }
  size_t StackSize(int cls) const { return cls_[cls].n_stack; }
  void Sync() { LIO_HIP(hipStreamSynchronize(stream_)); }

  Rigid<float> transform_sum_, transform_tobe_mapped_, transform_bef_mapped_, transform_aft_mapped_;
  bool imu_inited_ = false;
  int cen_[3] = {10, 10, 5};  // laser_cloud_cen_length_/width_/height_ (:76-78)
  std::vector<uint32_t> valid_idx_;
  std::vector<uint32_t> surround_idx_;   // laser_cloud_surround_idx_: every in-range cube of the 5x5x5 neighbourhood, FOV or not
  int iterations_ = 0, num_selected_ = 0;
  bool degenerate_ = false;
  int kz_ = 0;   // leading update components masked by round 0's degeneracy test (PointMapping.cc:650-680)

 private:
  friend struct MapChain;
  struct ClassMap {
    DBuf<float4> pool, pool2;       // points in the map frame; pool2 = gather target (swapped in)
    DBuf<uint32_t> pkey, pkey2;     // packed absolute cube key per pool point
    DBuf<uint32_t> vrank;           // cube rank of the valid tail
    size_t n = 0, n_rest = 0, n_valid = 0;
    bool layout_ok = false;
    std::vector<uint32_t> layout_keys;
    int layout_lo[3] = {0, 0, 0}, layout_hi[3] = {0, 0, 0};
    // scratch
    DBuf<uint32_t> rk, rk2, vals, vals2;
    DBuf<char> tmp;
    DBuf<MapCounters> counters;
    DBuf<float4> new_pts, u_pts;
    DBuf<uint32_t> new_key, u_rank;
    DBuf<unsigned long long> k64, k64b;
    DBuf<int> flags, pos;
    DBuf<int> cube_bounds;          // [LIO_MAP_MAX_VALID][6] order-preserving int images of min/max
    KnnGrid grid;
    VoxelGridDev vox;
    DBuf<float4> in, stack_raw, stack_ds;
    size_t n_stack = 0;
    HostBuf<MapCounters> h_counters;
  };

  MapValidSet MakeValidSet(const uint32_t *valid_idx, size_t n, const int cen_of_idx[3]) const;
  bool LayoutMatches(const ClassMap &m, const MapValidSet &vs) const;
  void LayoutLaunch(ClassMap &m, const MapValidSet &vs);   // rank + sort + gather, counters D2H queued
  void LayoutFinish(ClassMap &m, const MapValidSet &vs);   // after a stream sync
  void UpdateLaunch(ClassMap &m, const float4 *new_sensor_pts, size_t n_new, const MapValidSet &vs, const Rigid<float> &T, float leaf);
  void UpdateFinish(ClassMap &m);

  // ---- what a step does on the handle alone; MapChain's steps (mapping.hip) call these for every handle of a call
  struct Step {            // what one handle carries between the chain's steps
    Rigid<float> T0;       // transform_tobe_mapped_ after the association: the stack's round trip, the window and the FOV test use it
    MapValidSet vs;
    size_t cnt[2];
    bool relayout[2];
  };
  void StepBegin(const Rigid<float> &transform_sum, Step &st);           // the call's resets, TransformAssociateToMap / the 4-D one
  Rigid<float> AssociatedPose(const Rigid<float> &transform_sum) const;  // the transform_tobe_mapped_ StepBegin would leave; changes nothing
  void WindowAt(const Rigid<float> &T0, int cen[3], int cc[3]) const;    // the centre the window shift would leave at T0 and the sensor's cube
  static bool CenFits(const int cen[3]);                                 // every cube offset of a window centred so fits the packed key
  void KeepFromMap();                                                    // the from-map clouds into their own buffers before the pool is rewritten
  void StepWindow(Step &st);                                             // cube bookkeeping, valid set, surround set, LayoutLaunch where the layout changed
  void StepFilterLaunch(const Step &st);                                 // the two VoxelGrids, the surf one on stream2_, joined back into stream_
  bool StepOptimizes();                                                  // MapBuilder's skip_count: false on a call that only updates the map (and does what that call does)
  void TransformUpdate();                                                // :760-763
  void OptimizeEnd(const OdomState &st, int M, bool four_dof);           // the state the rounds ended with into the handle, TransformUpdate
  bool StepUpdates() const { return cfg_.map_builder != 0 || !imu_inited_; }
  void FullBegin(size_t n);                                              // a new full cloud of n points, before its points are written: the count, "not registered yet", room
  void StepRegisterFull();                                               // PublishResults on full_cloud_, once per set
  bool FourDof() const { return cfg_.map_builder != 0 && cfg_.enable_4d != 0; }
  MapChain &Chain();

  lio_map_config cfg_;
  hipStream_t stream_ = nullptr, stream2_ = nullptr;   // stream2_: the surf stack's VoxelGrid beside the corner one
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr, ev_full_ = nullptr, ev_full_read_ = nullptr;   // ev_full_: recorded behind the full cloud's registration
  bool full_event_ = false, full_read_ = false;   // ev_full_read_: behind another stream's copy out of it
  ClassMap cls_[2];  // 0 corner, 1 surf
  float pz_[3] = {0, 0, 10};
  DBuf<float4> stack_all_;
  DBuf<uint8_t> f_valid_;
  DBuf<float4> f_coef_, f_abs_;
  size_t n_score_slots_ = 0;
  bool score_ready_ = false;
  size_t n_from_map_[2] = {0, 0};  // sizes of laser_cloud_{corner,surf}_from_map_ of the last Process
  bool from_map_in_u_ = false;      // the map update moved them into the work list
  bool from_map_kept_ = false;      // a direct UpdateMapDatabase copied them into from_map_keep_ before it rewrote the pool and the work list
  DBuf<float4> from_map_keep_[2];
  // surround-map assembly: bin per point of [corner pool | surf pool], one 8-bit seg_sort pass over it, gather
  DBuf<uint32_t> sur_bin_, sur_bin2_, sur_src_, sur_hist_;
  DBuf<SegDesc> sur_desc_;
  DBuf<int> sur_count_;
  HostBuf<int> h_sur_count_;
  HostBuf<SegDesc> h_sur_desc_;
  DBuf<float4> sur_cloud_, sur_out_;
  VoxelGridDev sur_vox_;
  DBuf<float4> full_, full_in_;     // full_cloud_ and the sensor-frame upload the registration reads (it writes out of place)
  size_t n_full_ = 0;
  bool full_mapped_ = false;        // this set has been through PublishResults
  bool system_init_ = false;        // MapBuilder.h:65
  int odom_count_ = 0;              // MapBuilder.h:69
  std::unique_ptr<MapChain> chain_;  // the chain's scratch when this handle is the first of a call (Process: the only one); no results live there
};

}  // namespace lio
