// seg_vox.hip — see seg_vox.h.  gfx950 kernels; blockIdx.y = the cloud, blockIdx.x = a 256-entry tile of its range, blocks past a cloud's own
// range leave at once.  Every kernel is a caller of the bodies of cloud_device.h.  No atomics, no block waits for another: plain dependent
// launches on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "seg_vox.h"
#include "cloud_device.h"

namespace lio {

// cloud c's record: the VoxSeg inside the caller's own record type, `stride` bytes from cloud to cloud
__device__ __forceinline__ const VoxSeg &vox_seg(const VoxSeg *__restrict__ rec, int stride, int c) {
  return *reinterpret_cast<const VoxSeg *>(reinterpret_cast<const char *>(rec) + size_t(stride) * c);
}

// the cloud's bounds folded into VoxParams (cloud_device.h: vox_fold_bounds), and from them how the sort sees the keys: one block per cloud
__global__ void __launch_bounds__(VOX_TILE) k_seg_vox_layout(const VoxSeg *__restrict__ rec, int stride, const float *__restrict__ partial,
                                                            VoxParams *__restrict__ params, KeyLayout *__restrict__ layout, int *__restrict__ flag, int max_bits) {
  const int c = blockIdx.x;
  const VoxSeg &R = vox_seg(rec, stride, c);
  VoxParams v;
  if (!vox_fold_bounds(partial + size_t(R.off / VOX_TILE) * 8, R.cap / VOX_TILE, R.inv_leaf, v)) return;
  params[c] = v;
  KeyLayout L{0, 0, 0, 0, 0, 0};
  if (v.n_valid > 0 && !flag[c]) {
    if (!vox_key_layout(v.minb, v.divb, max_bits, L)) flag[c] = 1;   // the launch's passes order max_bits + 1 bits
  }
  layout[c] = L;
}

// Behind the sort: heads per 256-entry tile of a cloud's sorted range, then the centroids — a run is added up in sorted order, i.e. in
// ascending original index (the sort is stable), the order the oracle fixes.  Keys: the sort's relative keys, all ones = no point (sorted
// last); positions from n on hold nothing.
__global__ void __launch_bounds__(VOX_TILE) k_seg_vox_heads(const VoxSeg *__restrict__ rec, int stride, const uint32_t *__restrict__ keys,
                                                           int *__restrict__ tile_heads) {
  const VoxSeg &R = vox_seg(rec, stride, blockIdx.y);
  if (int(blockIdx.x) >= R.cap / VOX_TILE) return;
  vox_tile_head_count(keys + R.off, R.n, blockIdx.x, tile_heads + R.off / VOX_TILE + blockIdx.x);
}

__global__ void __launch_bounds__(VOX_TILE) k_seg_vox_centroids(const VoxSeg *__restrict__ rec, int stride, const float4 *pts, const uint32_t *__restrict__ keys,
                                                               const uint32_t *__restrict__ vals, const int *__restrict__ tile_heads, float4 *out,
                                                               const VoxParams *__restrict__ params, int *__restrict__ flag, VoxSegOut *__restrict__ vout) {
  const int c = blockIdx.y;
  const VoxSeg &R = vox_seg(rec, stride, c);
  const int ntiles = R.cap / VOX_TILE;
  if (int(blockIdx.x) >= ntiles) return;
  // (vals index the call's point array: pts is not shifted; a destination read from the record is tied to the argument, dev.h: rebase)
  float4 *dst = R.dst ? rebase(pts, R.dst) : out + R.off;
  const VoxSlot r = vox_centroid_tile(pts, keys + R.off, vals + R.off, tile_heads + R.off / VOX_TILE, R.n, blockIdx.x, dst);
  if (int(blockIdx.x) == ntiles - 1 && threadIdx.x == VOX_TILE - 1) {   // the cloud's last tile knows the total
    VoxSegOut o;
    o.count = r.pos + (r.head ? 1 : 0);
    o.params = params[c];
    o.flagged = flag[c];
    flag[c] = 0;   // clear for the next call (no fill command in front of it)
    vout[c] = o;
  }
}

void SegVoxFilter::reserve(size_t points, int clouds, hipStream_t s) {
  const size_t N = points, C = size_t(std::max(clouds, 1));
  ckeys_.reserve(N, s); keys_.reserve(N, s); keysb_.reserve(N, s); vals_.reserve(N, s); valsb_.reserve(N, s);
  partial_.reserve(N / VOX_TILE * 8, s); tile_heads_.reserve(N / VOX_TILE, s);
  d_seg_.reserve(C, s); d_layout_.reserve(C, s); d_params_.reserve(C, s); d_out_.reserve(C, s);
  if (flag_.cap < C) { flag_.reserve(C, s); LIO_HIP(hipMemsetAsync(flag_.p, 0, sizeof(int) * flag_.cap, s)); }
  if (h_seg_.n < C) { const size_t c = C + C / 2; h_seg_.alloc(c, hipHostMallocDefault, true); h_out_.alloc(c, hipHostMallocDefault, true); }
}

void SegVoxFilter::finish(const VoxSeg *rec, const VoxSeg *h_rec, size_t stride, int clouds, int passes, const float4 *pts, float4 *out, hipStream_t s) {
  if (clouds <= 0) return;
  int max_cap = 0;
  for (int c = 0; c < clouds; ++c) {
    const VoxSeg &R = *reinterpret_cast<const VoxSeg *>(reinterpret_cast<const char *>(h_rec) + stride * size_t(c));
    h_seg_.p[c] = SegDesc{R.off, R.n, 0};
    max_cap = std::max(max_cap, R.cap);
  }
  const SegSortPlan plan = seg_sort_plan(h_seg_.p, clouds, SS_MAX_BITS);
  LIO_HIP(hipMemcpyAsync(d_seg_.p, h_seg_.p, sizeof(SegDesc) * size_t(clouds), hipMemcpyHostToDevice, s));
  const int ntiles = max_cap / VOX_TILE, max_bits = std::min(31, SS_MAX_BITS * passes - 1);
  hipLaunchKernelGGL(k_seg_vox_layout, dim3(clouds), dim3(VOX_TILE), 0, s, rec, int(stride), partial_.p, d_params_.p, d_layout_.p, flag_.p, max_bits);
  const SegSortPair sorted = seg_sort_passes(d_seg_.p, clouds, plan, ckeys_.p, nullptr, ping(), pong(), hist(plan.hist_entries, s), SS_MAX_BITS, passes, d_layout_.p, s);
  hipLaunchKernelGGL(k_seg_vox_heads, dim3(ntiles, clouds), dim3(VOX_TILE), 0, s, rec, int(stride), sorted.keys, tile_heads_.p);
  hipLaunchKernelGGL(k_seg_vox_centroids, dim3(ntiles, clouds), dim3(VOX_TILE), 0, s, rec, int(stride), pts, sorted.keys, sorted.vals, tile_heads_.p, out, d_params_.p,
                     flag_.p, d_out_.p);
  LIO_HIP(hipGetLastError());
  LIO_HIP(hipMemcpyAsync(h_out_.p, d_out_.p, sizeof(VoxSegOut) * size_t(clouds), hipMemcpyDeviceToHost, s));
}

}  // namespace lio
