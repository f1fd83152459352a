// seg_vox.h — pcl::VoxelGrid (Estimator.cc:678-693, :1518-1519) for the CLOUDS of a call side by side, one launch per stage over all of them:
// the local maps of a batched solve (batch_kernels.h) and the sweeps of a batched push (est_push.h) run this one chain.
//
// A cloud is a VoxSeg inside its caller's own record (BatchWin, BpCloud): the kernels read it as (first record's VoxSeg, byte stride, index),
// so no caller uploads a second table.  The caller's producer kernel (k_bw_concat_keys, k_bp_take_keys) writes the points, their stored keys
// (cloud_device.h: vox_take_point, absolute cells), the blocks' shares of the bounds and raises the cloud's flag; finish() runs the rest:
//
//   k_seg_vox_layout               one block per cloud: bounds -> VoxParams, how the sort sees the keys (seg_sort.h: KeyLayout)
//   seg_sort_passes                one segment per cloud, three or four 9-bit passes
//   k_seg_vox_heads / _centroids   (max cap / 256, clouds): run heads per tile, centroids; the cloud's last tile posts count, bounds and flag
//   one copy of the output table
//
// The arithmetic is cloud_device.h's, which the single-window filter (VoxelGridDev) runs too: the centroids of a cloud are the same bits
// alone and in any call.  A cloud the chain cannot take (keys beyond the absolute range or beyond what the passes order) comes back flagged.
#pragma once
#include "cloud_kernels.h"
#include "seg_sort.h"

namespace lio {

struct VoxSeg {
  int n, off, cap;   // points; the cloud's range of the call's arrays (off, cap multiples of 256, cap >= max(n, 1))
  float inv_leaf;
  float4 *dst;       // where the centroids go (room for n points); null: the call's shared output array, at off
};
// what the filter reports per cloud (read by the host behind the caller's wait); flagged: keys beyond the range or the passes
struct VoxSegOut { int count; VoxParams params; int flagged; };

// The chain's arrays and tables; owned by an EstimatorBatch (one per part), sized by the largest call so far.  Its users take turns on the
// batch's one stream and each reads out() behind its own wait, before the other runs.
class SegVoxFilter {
 public:
  // the pass rule: three 9-bit passes order 27 bits — 26 of key and "no point" above them, which is what a 200 m x 200 m x 25 m map at a
  // 0.4 m leaf takes.  The bounds are only known on the device, so the host goes by what a cloud's keys took the last time (0: not known yet,
  // four passes); a cloud that outgrows the guess is flagged by the layout kernel.
  static int passes_for(int last_bits) { return last_bits == 0 || last_bits > 26 ? 4 : 3; }
  // bits the relative keys of a cloud with these bounds took; 0: the cloud had no finite point
  static int bits_taken(const VoxParams &v) { return v.n_valid > 0 ? std::max(1, bits_for(v.divb[0]) + bits_for(v.divb[1]) + bits_for(v.divb[2])) : 0; }

  // room for a call of `points` (the clouds' caps added up) in `clouds` clouds
  void reserve(size_t points, int clouds, hipStream_t s);
  // what the producer kernel writes: stored keys and 8 floats per 256-point block at the clouds' ranges, one flag per cloud (zero between calls:
  // the centroids' last tile clears it)
  uint32_t *keys() const { return ckeys_.p; }
  float *partial() const { return partial_.p; }
  int *flag() const { return flag_.p; }
  // Behind the producer: layout, sort, heads, centroids and the copy of the output table, enqueued on s; no wait.  rec: the first cloud's VoxSeg on
  // the device, h_rec: the same on the host, both `stride` bytes apart.  pts: the array the clouds' ranges index; out: the shared output array
  // of the clouds without a dst.  passes: 3 or 4.
  void finish(const VoxSeg *rec, const VoxSeg *h_rec, size_t stride, int clouds, int passes, const float4 *pts, float4 *out, hipStream_t s);
  const VoxSegOut &out(int i) const { return h_out_.p[i]; }   // after the caller's wait
  // the sort's scratch, for a caller's own segmented sort between two calls (the K-NN grids of a solve): the ping-pong pairs, `entries` histogram words
  SegSortPair ping() const { return {keys_.p, vals_.p}; }
  SegSortPair pong() const { return {keysb_.p, valsb_.p}; }
  uint32_t *hist(size_t entries, hipStream_t s) { hist_.reserve(std::max<size_t>(entries, 1), s); return hist_.p; }

 private:
  DBuf<uint32_t> ckeys_, keys_, keysb_, vals_, valsb_, hist_;
  DBuf<float> partial_;
  DBuf<int> tile_heads_, flag_;
  DBuf<SegDesc> d_seg_; DBuf<KeyLayout> d_layout_; DBuf<VoxParams> d_params_; DBuf<VoxSegOut> d_out_;
  HostBuf<SegDesc> h_seg_; HostBuf<VoxSegOut> h_out_;   // pinned
};

}  // namespace lio
