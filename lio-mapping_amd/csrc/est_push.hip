// est_push.hip — see est_push.h.  gfx950 kernels; blockIdx.y = the cloud (or the window of a slide), blockIdx.x = a block of 256 of its points,
// blocks past a cloud's own range leave at once.  Every kernel is a caller of the bodies of cloud_device.h; pointers read from a record are
// tied to a kernel-argument pointer (dev.h: rebase).  No atomics, no block waits for another: plain dependent launches on the part's stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "est_push.h"
#include "cloud_device.h"

namespace lio {

#define BP_THREADS 256
static_assert(BP_THREADS == VOX_TILE, "the filter bodies of cloud_device.h work on 256-entry tiles");

// ------------------------------------------------------------------------------------------------
// TransformToEnd (Estimator.cc:62-103, where the record says so) and, from the point still in registers, the filter's sort key in absolute
// cells and the block's share of the bounds (batch_kernels.hip: k_bw_concat_keys does the same behind its concat).  One point per lane: one
// 16-byte load from a clamped address, one 16-byte store.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BP_THREADS) k_bp_take_keys(const BpCloud *__restrict__ rec, const float4 *__restrict__ staging, float4 *__restrict__ in_all,
                                                            uint32_t *__restrict__ keys, float *__restrict__ partial, int *__restrict__ flag) {
  const int c = blockIdx.y;
  const BpCloud &R = rec[c];
  const int base = int(blockIdx.x) * BP_THREADS;
  if (base >= R.cap) return;
  const int gid = base + threadIdx.x;
  float4 p = staging[R.src_off + min(gid, max(R.n - 1, 0))];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float cnt = 0;
  if (gid < R.n) {
    if (R.deskew) p = deskew_to_end_point<false>(p, Quat<float>(R.qe[3], R.qe[0], R.qe[1], R.qe[2]), Vec3<float>(R.te[0], R.te[1], R.te[2]), R.time_factor);
    in_all[R.off + gid] = p;
    uint32_t key = BW_KEY_NONE;
    if (finite3(p)) {
      cnt = 1.f;
      mn[0] = mx[0] = p.x; mn[1] = mx[1] = p.y; mn[2] = mx[2] = p.z;
      if (!vox_abs_key<9>(p, R.inv_leaf, key)) flag[c] = 1;   // beyond the absolute key: the handle's own filter has that form
    }
    keys[R.off + gid] = key;
  }
  vox_block_partial(mn, mx, cnt, partial + (size_t(R.off / BP_THREADS) + blockIdx.x) * 8);
}

// the cloud's bounds folded into VoxParams, and from them how the sort sees the keys: one block per cloud
__global__ void __launch_bounds__(BP_THREADS) k_bp_key_layout(const BpCloud *__restrict__ rec, const float *__restrict__ partial, VoxParams *__restrict__ params,
                                                             KeyLayout *__restrict__ layout, int *__restrict__ flag, int max_bits) {
  const int c = blockIdx.x;
  const BpCloud &R = rec[c];
  VoxParams v;
  if (!vox_fold_bounds(partial + size_t(R.off / BP_THREADS) * 8, R.cap / BP_THREADS, R.inv_leaf, v)) return;
  params[c] = v;
  KeyLayout L{0, 0, 0, 0, 0, 0};
  if (v.n_valid > 0 && !flag[c]) {
    if (!vox_key_layout(v.minb, v.divb, max_bits, L)) flag[c] = 1;   // more bits than the launch's passes order
  }
  layout[c] = L;
}

void launch_bp_take_keys(const BpCloud *rec, int nclouds, int max_n, const float4 *staging, float4 *in_all, uint32_t *keys, float *partial, VoxParams *params,
                         KeyLayout *layout, int *flag, int max_bits, hipStream_t s) {
  if (nclouds <= 0) return;
  hipLaunchKernelGGL(k_bp_take_keys, dim3(std::max(1, cdiv(max_n, BP_THREADS)), nclouds), dim3(BP_THREADS), 0, s, rec, staging, in_all, keys, partial, flag);
  hipLaunchKernelGGL(k_bp_key_layout, dim3(nclouds), dim3(BP_THREADS), 0, s, rec, partial, params, layout, flag, max_bits);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// pcl::VoxelGrid (Estimator.cc:678-693) behind the sort: heads per tile of a cloud's sorted range, then the centroids — written into the
// handle's own stack buffer, in the order and by the sums of the single-window filter (cloud_device.h: vox_centroid_tile)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BP_THREADS) k_bp_vox_heads(const BpCloud *__restrict__ rec, const uint32_t *__restrict__ keys, int *__restrict__ tile_heads) {
  const BpCloud &R = rec[blockIdx.y];
  if (int(blockIdx.x) >= R.cap / BP_THREADS) return;
  vox_tile_head_count(keys + R.off, R.n, blockIdx.x, tile_heads + R.off / BP_THREADS + blockIdx.x);
}

__global__ void __launch_bounds__(BP_THREADS) k_bp_vox_centroids(const BpCloud *__restrict__ rec, const float4 *in_all, const uint32_t *__restrict__ keys,
                                                                const uint32_t *__restrict__ vals, const int *__restrict__ tile_heads,
                                                                const VoxParams *__restrict__ params, int *__restrict__ flag, BpVoxOut *__restrict__ vout) {
  const int c = blockIdx.y;
  const BpCloud &R = rec[c];
  const int ntiles = R.cap / BP_THREADS;
  if (int(blockIdx.x) >= ntiles) return;
  // (vals index the chain's input array: in_all is not shifted; the destination is the handle's, tied to the argument)
  const VoxSlot r = vox_centroid_tile(in_all, keys + R.off, vals + R.off, tile_heads + R.off / BP_THREADS, R.n, blockIdx.x, rebase(in_all, R.dst));
  if (int(blockIdx.x) == ntiles - 1 && threadIdx.x == BP_THREADS - 1) {   // the cloud's last tile knows the total
    BpVoxOut o;
    o.count = r.pos + (r.head ? 1 : 0);
    o.params = params[c];
    o.flagged = flag[c];
    flag[c] = 0;   // clear for the next call (no fill command in front of it)
    vout[c] = o;
  }
}

void launch_bp_vox_finish(const BpCloud *rec, int nclouds, int max_cap, const float4 *in_all, const uint32_t *keys_sorted, const uint32_t *vals_sorted, int *tile_heads,
                          const VoxParams *params, int *flag, BpVoxOut *out, hipStream_t s) {
  if (nclouds <= 0 || max_cap <= 0) return;
  const int ntiles = max_cap / BP_THREADS;
  hipLaunchKernelGGL(k_bp_vox_heads, dim3(ntiles, nclouds), dim3(BP_THREADS), 0, s, rec, keys_sorted, tile_heads);
  hipLaunchKernelGGL(k_bp_vox_centroids, dim3(ntiles, nclouds), dim3(BP_THREADS), 0, s, rec, in_all, keys_sorted, vals_sorted, tile_heads, params, flag, out);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// SlideWindow (Estimator.cc:2602-2615) of every window: what is left of the pivot's stack mapped into the next frame, then that frame's
// own stack, into the handle's scratch cloud (cloud_kernels.hip: k_transform_concat for one window)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BP_THREADS) k_bp_slide(const BpSlide *__restrict__ rec) {
  const BpSlide &S = rec[blockIdx.y];
  const int base = int(blockIdx.x) * BP_THREADS;
  if (base >= S.total) return;
  const int gid = base + threadIdx.x, g = min(gid, S.total - 1);
  const int sidx = g >= S.seg[1].dst_off ? 1 : 0;
  const BwSeg &sg = S.seg[sidx];
  const float4 p = rebase(rec, sg.src)[g - sg.dst_off];
  float4 o;
  if (sg.identity) o = p;
  else o = affine_map_point(sg.tf.m, p);
  if (sg.set_intensity) o.w = sg.intensity;
  if (gid < S.total) rebase(rec, S.dst)[gid] = o;
}
void launch_bp_slide(const BpSlide *rec, int nwin, int max_total, hipStream_t s) {
  if (nwin <= 0 || max_total <= 0) return;
  hipLaunchKernelGGL(k_bp_slide, dim3(cdiv(max_total, BP_THREADS), nwin), dim3(BP_THREADS), 0, s, rec);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// the chain
// ------------------------------------------------------------------------------------------------
void PushChain::begin(int max_clouds) {
  n_ = 0; total_ = 0; max_n_ = 0; max_cap_ = 0;
  src_.clear();
  if (max_clouds > cap_) {
    const size_t c = size_t(max_clouds) + size_t(max_clouds) / 2;
    h_rec_.alloc(c, hipHostMallocDefault, true); h_out_.alloc(c, hipHostMallocDefault, true); h_seg_.alloc(c, hipHostMallocDefault, true);
    cap_ = int(c);
  }
}

int PushChain::add(const float *host_xyzi, size_t n, float leaf, bool deskew, const float q[4], const float p[3], float time_factor, float4 *dst) {
  if (n_ >= cap_) throw std::runtime_error("PushChain: more clouds than the call announced");
  const int cap = int((std::max<size_t>(n, 1) + 255) / 256 * 256);
  if (size_t(total_) + size_t(cap) > size_t(INT_MAX) / 2) throw CapacityError("lio_est_batch_push_frames: the call's clouds exceed 2^30 points");
  BpCloud &R = h_rec_.p[n_];
  R.src_off = total_; R.n = int(n); R.off = total_; R.cap = cap;
  R.inv_leaf = 1.0f / leaf;
  R.deskew = deskew ? 1 : 0;
  for (int k = 0; k < 4; ++k) R.qe[k] = q[k];
  for (int k = 0; k < 3; ++k) R.te[k] = p[k];
  R.time_factor = time_factor;
  R.dst = dst;
  src_.push_back(host_xyzi);
  total_ += cap;
  max_n_ = std::max(max_n_, int(n)); max_cap_ = std::max(max_cap_, cap);
  return n_++;
}

bool PushChain::run(int passes, hipStream_t s) {
  if (n_ == 0) return false;
  const size_t N = size_t(total_), C = size_t(n_);
  staging_.reserve(N, s); in_all_.reserve(N, s);
  ckeys_.reserve(N, s); keys_.reserve(N, s); keysb_.reserve(N, s); vals_.reserve(N, s); valsb_.reserve(N, s);
  partial_.reserve(N / 256 * 8, s); tile_heads_.reserve(N / 256, s);
  d_rec_.reserve(C, s); d_out_.reserve(C, s); d_seg_.reserve(C, s); d_layout_.reserve(C, s); d_params_.reserve(C, s);
  if (d_flag_.cap < C) { d_flag_.reserve(C, s); LIO_HIP(hipMemsetAsync(d_flag_.p, 0, sizeof(int) * d_flag_.cap, s)); }
  // 1. the clouds into the staging array, the records and the segments in one table each
  for (int i = 0; i < n_; ++i) {
    const BpCloud &R = h_rec_.p[i];
    if (R.n) LIO_HIP(hipMemcpyAsync(staging_.p + R.src_off, src_[size_t(i)], size_t(R.n) * sizeof(float4), hipMemcpyHostToDevice, s));
    h_seg_.p[i] = SegDesc{R.off, R.n, 0};
  }
  const SegSortPlan plan = seg_sort_plan(h_seg_.p, n_, SS_MAX_BITS);
  hist_.reserve(std::max<size_t>(plan.hist_entries, 1), s);
  LIO_HIP(hipMemcpyAsync(d_rec_.p, h_rec_.p, sizeof(BpCloud) * C, hipMemcpyHostToDevice, s));
  LIO_HIP(hipMemcpyAsync(d_seg_.p, h_seg_.p, sizeof(SegDesc) * C, hipMemcpyHostToDevice, s));
  // 2. - 5.
  launch_bp_take_keys(d_rec_.p, n_, max_n_, staging_.p, in_all_.p, ckeys_.p, partial_.p, d_params_.p, d_layout_.p, d_flag_.p, std::min(31, SS_MAX_BITS * passes - 1), s);
  const SegSortPair sorted = seg_sort_passes(d_seg_.p, n_, plan, ckeys_.p, nullptr, {keys_.p, vals_.p}, {keysb_.p, valsb_.p}, hist_.p, SS_MAX_BITS, passes, d_layout_.p, s);
  launch_bp_vox_finish(d_rec_.p, n_, max_cap_, in_all_.p, sorted.keys, sorted.vals, tile_heads_.p, d_params_.p, d_flag_.p, d_out_.p, s);
  // 6. one copy, one wait
  LIO_HIP(hipMemcpyAsync(h_out_.p, d_out_.p, sizeof(BpVoxOut) * C, hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
  return true;
}

}  // namespace lio
