// batch_kernels.hip — see batch_kernels.h.  gfx950 kernels; blockIdx.y (or .z) = the window, blockIdx.x = a block of that window's
// share, blocks past a window's own size leave at once.  Clouds are float4 AoS as everywhere (cloud_kernels.hip); the batch's
// arrays are the windows' ranges laid end to end, so a wave's 64 lanes always read one window's consecutive points.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batch_kernels.h"
#include "seg_sort.h"
#include "cloud_device.h"

namespace lio {

#define BW_THREADS 256
static_assert(BW_THREADS == VOX_TILE, "the filter bodies of cloud_device.h work on 256-entry tiles");

int bw_round_blocks(int M) { return std::max(1, cdiv(M, 64)); }

// ------------------------------------------------------------------------------------------------
// BuildLocalMap, first half: pcl::transformPointCloud + `+=` (Estimator.cc:1480-1507) and, from the point still in registers, the
// filter's sort key — the window above PCL's voxel index in absolute cells (cloud_kernels.hip: k_vox_keys_abs; the window in the
// high word keeps every window's points together through ONE sort of the whole batch) — and the block's share of the bounds.
// The layout, the sort, the heads and the centroids behind it: SegVoxFilter::finish (seg_vox.hip).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VOX_TILE) k_bw_concat_keys(const BatchWin *__restrict__ win, float4 *__restrict__ local_all, uint32_t *__restrict__ keys,
                                                            float *__restrict__ partial, int *__restrict__ flag) {
  const int w = blockIdx.y;
  const BatchWin &W = win[w];
  const int base = int(blockIdx.x) * VOX_TILE;
  if (base >= W.vox.cap) return;
  const int gid = base + threadIdx.x;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float cnt = 0;
  if (gid < W.vox.n) {
    const float4 o = concat_point(W.seg, W.nseg, gid, local_all);
    local_all[W.vox.off + gid] = o;
    // z 9 bits (+-102 m of height at a 0.4 m leaf; a window beyond that takes the single-window path); the sort runs on the key relative
    // to the window's bounds (seg_sort.h: KeyLayout)
    keys[W.vox.off + gid] = vox_take_point<9, BW_KEY_NONE>(o, W.vox.inv_leaf, mn, mx, cnt, flag + w);
  }
  vox_block_partial(mn, mx, cnt, partial + (size_t(W.vox.off / VOX_TILE) + blockIdx.x) * 8);
}
void launch_bw_concat_keys(const BatchWin *win, int B, int max_local, float4 *local_all, uint32_t *keys, float *partial, int *flag, hipStream_t s) {
  if (B <= 0 || max_local <= 0) return;
  hipLaunchKernelGGL(k_bw_concat_keys, dim3(cdiv(max_local, VOX_TILE), B), dim3(VOX_TILE), 0, s, win, local_all, keys, partial, flag);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// what a solve's feature stage starts from (cloud_kernels.hip: k_solve_setup, per window): feature flags cleared, the newest
// frame's Gauss-Newton state = its local transform; a window without a newest frame counts as converged from the start
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BW_THREADS) k_bw_setup(const BatchWin *__restrict__ win, uint8_t *__restrict__ valid_all, OdomState *__restrict__ odom,
                                                        int *__restrict__ n_converged) {
  const int w = blockIdx.y;
  const BatchWin &W = win[w];
  clear_valid_block(valid_all + W.slot_base, size_t(W.n_slots));   // slot_base is a multiple of 16
  if (blockIdx.x == 0) {
    const bool none = W.newest.M <= 0;
    odom_state_init(odom + w, W.tf[LIO_BW_MAX_STATIC], none);
    if (none && threadIdx.x == 0) atomicAdd(n_converged, 1);
  }
}
void launch_bw_setup(const BatchWin *win, int B, int max_slots, uint8_t *valid_all, OdomState *odom, int *n_converged, hipStream_t s) {
  if (B <= 0) return;
  const int nb = std::max(1, cdiv((long long)max_slots, BW_THREADS * 16));
  hipLaunchKernelGGL(k_bw_setup, dim3(nb, B), dim3(BW_THREADS), 0, s, win, valid_all, odom, n_converged);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// K-NN grid (KdTreeFLANN::setInputCloud, Estimator.cc:1544-1545): a window's filtered points ordered by cell (seg_sort.h: the same
// segmented sort as the filter's, so the order inside a cell is the filtered cloud's — defined, unlike a histogram's atomics) and a
// dense table of run starts per window; the tables of the batch are laid end to end, an entry is a position in the batch's
// cell-sorted point array and the search kernels take that array's base as their map.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BW_THREADS) k_bw_cell_keys(const BatchWin *__restrict__ win, const BatchGrid *__restrict__ grid,
                                                            const float4 *__restrict__ filtered_all, uint32_t *__restrict__ keys) {
  const int w = blockIdx.y;
  const BatchGrid &G = grid[w];
  const int i = int(blockIdx.x) * BW_THREADS + threadIdx.x;
  if (i >= G.n_filtered) return;
  const int gi = win[w].vox.off + i;
  keys[gi] = cell_key_clamped(filtered_all[gi], G.g);
}
// behind the sort by cell: the cell-sorted points, and the table — entry c = position of the first point whose cell is >= c (an empty cell
// holds the start of the next occupied one, entry n_cells the end), every entry written here: no histogram, no scan, no clearing.
// A point whose cell differs from its predecessor's owns the entries (predecessor's cell, its own]; the wave writes those ranges one
// after the other, 64 entries per store.
__global__ void __launch_bounds__(BW_THREADS) k_bw_cell_table(const BatchWin *__restrict__ win, const BatchGrid *__restrict__ grid,
                                                             const float4 *__restrict__ filtered_all, const uint32_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ vals, int *__restrict__ cells_all, float4 *__restrict__ sorted_all) {
  const int w = blockIdx.y;
  const BatchGrid &G = grid[w];
  const int n = G.n_filtered;
  const int i0 = int(blockIdx.x) * BW_THREADS;
  if (i0 >= max(n, 1)) return;
  const int off = win[w].vox.off, i = i0 + threadIdx.x, lane = threadIdx.x & 63;
  const int ncells = G.g.dims[0] * G.g.dims[1] * G.g.dims[2];
  int *cells = cells_all + G.cell_off;
  if (n == 0) {   // (block 0 only)
    for (int c = threadIdx.x; c <= ncells; c += BW_THREADS) cells[c] = off;
    return;
  }
  int lo = 0, hi = -1;   // entries [lo, hi] get the value off + i
  if (i < n) {
    const uint32_t gsrc = vals[off + i];
    float4 p = filtered_all[gsrc];
    p.w = __int_as_float(int(gsrc) - off);   // the point's index in the window's filtered cloud: what the search orders ties by
    sorted_all[off + i] = p;
    const int k = int(keys[off + i]), prev = i ? int(keys[off + i - 1]) : -1;
    lo = prev + 1; hi = k;
  }
  // most ranges are one to a few entries (neighbouring occupied cells): the owning lane writes up to four itself; only what is left of the
  // long ones (a jump to the next row or layer) goes through the wave, 64 entries per store
#pragma unroll
  for (int q = 0; q < 4; ++q) if (lo + q <= hi) cells[lo + q] = off + i;
  lo += 4;
  unsigned long long heads = __ballot(hi >= lo);
  while (heads) {
    const int src = __ffsll((long long)heads) - 1;
    heads &= heads - 1;
    const int a = __shfl(lo, src, 64), b = __shfl(hi, src, 64), v = off + (i - lane) + src;
    for (int c = a + lane; c <= b; c += 64) cells[c] = v;
  }
  // entries behind the last occupied cell: the end (the whole block of the last point writes them)
  __shared__ int s_last;
  if (threadIdx.x == 0) s_last = -2;
  __syncthreads();
  if (i == n - 1) s_last = int(keys[off + i]);
  __syncthreads();
  if (s_last != -2)
    for (int c = s_last + 1 + int(threadIdx.x); c <= ncells; c += BW_THREADS) cells[c] = off + n;
}
void launch_bw_cell_keys(const BatchWin *win, const BatchGrid *grid, int B, int max_filtered, const float4 *filtered_all, uint32_t *keys, hipStream_t s) {
  if (B <= 0 || max_filtered <= 0) return;
  hipLaunchKernelGGL(k_bw_cell_keys, dim3(cdiv(max_filtered, BW_THREADS), B), dim3(BW_THREADS), 0, s, win, grid, filtered_all, keys);
  LIO_HIP(hipGetLastError());
}
void launch_bw_cell_table(const BatchWin *win, const BatchGrid *grid, int B, int max_filtered, const float4 *filtered_all, const uint32_t *keys_sorted,
                          const uint32_t *vals_sorted, int *cells_all, float4 *sorted_all, hipStream_t s) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_bw_cell_table, dim3(std::max(1, cdiv(max_filtered, BW_THREADS)), B), dim3(BW_THREADS), 0, s, win, grid, filtered_all, keys_sorted, vals_sorted,
                     cells_all, sorted_all);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// CalculateFeatures (Estimator.cc:1014-1097) of the frames behind the pivot: grid (64-query blocks of the largest frame, frames,
// windows).  A block always owns 64 queries; LPQ lanes work on each, so the block is 64 LPQ threads wide.  The result does not
// depend on LPQ (the candidate set and the total order (distance, index) do not: cloud_device.h), which therefore follows the
// size of the launch: eight lanes shorten a query's dependent candidate walk when the launch is small, one lane per query wins
// once the launch fills the chip many times over (no merge shuffles, no idle lanes in the fit; DESIGN.md: keyframe batch).
// ------------------------------------------------------------------------------------------------
template <int LPQ>
__device__ __forceinline__ void bw_features_body(const BatchWin *__restrict__ win, const BatchGrid *__restrict__ grid, const float4 *__restrict__ sorted_all,
                                                 const int *__restrict__ cells_all, uint8_t *__restrict__ valid_all, float4 *__restrict__ coef_all,
                                                 float *__restrict__ score_all) {
  const int w = blockIdx.z;
  const BatchWin &W = win[w];
  if (int(blockIdx.y) >= W.nstatic) return;
  const BatchGrid &G = grid[w];
  const FeatScalars fs{W.min_match_sq_dis, W.min_plane_dis, 0, {0.f, 0.f, 0.f}};
  FeatFrame frm = W.fr[blockIdx.y];
  frm.stack = rebase(sorted_all, frm.stack);   // (dev.h: a pointer read from a descriptor is generic until it is tied to a kernel argument)
  features_block<false, LPQ, 64 * LPQ>(frm, fs, int(blockIdx.x), &W.tf[0][0], sorted_all, cells_all + G.cell_off, G.g, valid_all, coef_all, score_all,
                                       nullptr);
}
template <int LPQ>
__global__ void __launch_bounds__(64 * LPQ) k_bw_features(const BatchWin *__restrict__ win, const BatchGrid *__restrict__ grid,
                                                         const float4 *__restrict__ sorted_all, const int *__restrict__ cells_all,
                                                         uint8_t *__restrict__ valid_all, float4 *__restrict__ coef_all, float *__restrict__ score_all) {
  bw_features_body<LPQ>(win, grid, sorted_all, cells_all, valid_all, coef_all, score_all);
}
// The one-lane-per-query form of the features at six waves per SIMD (the keyframe batch's k_kf_round1_w8 gained 15 % from eight
// waves per SIMD at 64 VGPRs).  Measured at 512 windows (round 6, flat candidate lists): features 4.09 ms at 6 waves, 4.29 at 8,
// 4.31 as compiled; the rounds lose at a fixed occupancy (4.84 ms as compiled, 6.39 at 6: their fit + row phase spills), so
// k_bw_odom_round<1> keeps the compiler's choice (earlier numbers: profiles/r5_m_occupancy.txt).
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6)))
k_bw_features1_w6(const BatchWin *__restrict__ win, const BatchGrid *__restrict__ grid, const float4 *__restrict__ sorted_all,
                  const int *__restrict__ cells_all, uint8_t *__restrict__ valid_all, float4 *__restrict__ coef_all, float *__restrict__ score_all) {
  bw_features_body<1>(win, grid, sorted_all, cells_all, valid_all, coef_all, score_all);
}
static int bw_lanes_per_query(const BatchKnobs &k, long long total_queries) {
  if (k.lanes_per_query) return k.lanes_per_query;
  // measured with the flat candidate lists (round 6, tools/r6 logs): one lane per query wins from ~100 k queries per launch (8 windows' newest
  // frames: rounds 0.27 -> 0.21 ms), four lanes from ~15 k (one window's newest frame: 0.148 -> 0.127 ms)
  return total_queries >= 100000 ? 1 : (total_queries >= 15000 ? 4 : 8);
}
void launch_bw_features(const BatchWin *win, const BatchGrid *grid, int B, int max_M, int max_static, long long total_queries, const BatchKnobs &knobs,
                        const float4 *sorted_all, const int *cells_all, uint8_t *valid_all, float4 *coef_all, float *score_all, hipStream_t s) {
  if (B <= 0 || max_M <= 0 || max_static <= 0) return;
  const dim3 g(cdiv(max_M, 64), max_static, B);
  switch (bw_lanes_per_query(knobs, total_queries)) {
    case 1: hipLaunchKernelGGL(k_bw_features1_w6, g, dim3(64), 0, s, win, grid, sorted_all, cells_all, valid_all, coef_all, score_all); break;
    case 4: hipLaunchKernelGGL(k_bw_features<4>, g, dim3(256), 0, s, win, grid, sorted_all, cells_all, valid_all, coef_all, score_all); break;
    default: hipLaunchKernelGGL(k_bw_features<8>, g, dim3(512), 0, s, win, grid, sorted_all, cells_all, valid_all, coef_all, score_all); break;
  }
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// One round of CalculateLaserOdom (Estimator.cc:1242-1359) for every window whose newest frame has not converged: the search /
// fit / rows launch and the fold + 6x6 step launch of cloud_kernels.hip's launch_odom_round, windows in blockIdx.y / .x.
// A search block owns 64 queries whatever the lanes per query, and leaves ONE row of partial sums: the fold — and with it
// every bit of the step — does not depend on how wide the launch made its blocks.
// ------------------------------------------------------------------------------------------------
template <int LPQ>
__device__ __forceinline__ void bw_odom_round_body(const BatchWin *__restrict__ win, const BatchGrid *__restrict__ grid, const OdomState *__restrict__ odom,
                                                   const float4 *__restrict__ sorted_all, const int *__restrict__ cells_all, uint8_t *__restrict__ valid_all,
                                                   float4 *__restrict__ coef_all, float *__restrict__ score_all, double *__restrict__ partials, int round) {
  const int w = blockIdx.y;
  const OdomState &st = odom[w];
  if (st.converged) return;
  const BatchWin &W = win[w];
  if (int(blockIdx.x) >= W.nb_round) return;
  const BatchGrid &G = grid[w];
  const float *tp = st.T;
  const Quat<float> q(tp[3], tp[0], tp[1], tp[2]);
  const Vec3<float> t(tp[4], tp[5], tp[6]);
  const FeatScalars fs{W.min_match_sq_dis, W.min_plane_dis, 0, {0.f, 0.f, 0.f}};
  FeatFrame frm = W.newest;
  frm.stack = rebase(sorted_all, frm.stack);
  const double v = odom_round_block<LPQ, 64 * LPQ>(fs, frm, q, t, sorted_all, cells_all + G.cell_off, G.g, valid_all, coef_all, score_all, W.newest.slot_off,
                                                   round, W.keep, int(blockIdx.x));
  if (threadIdx.x < 28) partials[(size_t(W.part_off) + blockIdx.x) * 28 + threadIdx.x] = v;
}
template <int LPQ>
__global__ void __launch_bounds__(64 * LPQ) k_bw_odom_round(const BatchWin *__restrict__ win, const BatchGrid *__restrict__ grid,
                                                           const OdomState *__restrict__ odom, const float4 *__restrict__ sorted_all,
                                                           const int *__restrict__ cells_all, uint8_t *__restrict__ valid_all,
                                                           float4 *__restrict__ coef_all, float *__restrict__ score_all,
                                                           double *__restrict__ partials, int round) {
  bw_odom_round_body<LPQ>(win, grid, odom, sorted_all, cells_all, valid_all, coef_all, score_all, partials, round);
}
__global__ void __launch_bounds__(1024) k_bw_odom_update(const BatchWin *__restrict__ win, OdomState *__restrict__ odom, const double *__restrict__ partials,
                                                        int round, int *__restrict__ n_converged) {
  const int w = blockIdx.x;
  OdomState *st = odom + w;
  if (st->converged) return;
  const BatchWin &W = win[w];
  odom_update_wide_block(partials + size_t(W.part_off) * 28, W.nb_round, st, round, 0, 0, nullptr, HostSignal());
  if (threadIdx.x == 0 && st->converged) atomicAdd(n_converged, 1);   // (thread 0 wrote the flag itself)
}
void launch_bw_odom_round(const BatchWin *win, const BatchGrid *grid, int B, int max_nb, long long total_queries, const BatchKnobs &knobs, int round, OdomState *odom,
                          const float4 *sorted_all, const int *cells_all, uint8_t *valid_all, float4 *coef_all, float *score_all, double *partials,
                          int *n_converged, hipStream_t s) {
  if (B <= 0 || max_nb <= 0) return;
  const dim3 g(max_nb, B);
  switch (bw_lanes_per_query(knobs, total_queries)) {
    case 1: hipLaunchKernelGGL(k_bw_odom_round<1>, g, dim3(64), 0, s, win, grid, odom, sorted_all, cells_all, valid_all, coef_all, score_all, partials, round); break;
    case 4: hipLaunchKernelGGL(k_bw_odom_round<4>, g, dim3(256), 0, s, win, grid, odom, sorted_all, cells_all, valid_all, coef_all, score_all, partials, round); break;
    default: hipLaunchKernelGGL(k_bw_odom_round<8>, g, dim3(512), 0, s, win, grid, odom, sorted_all, cells_all, valid_all, coef_all, score_all, partials, round); break;
  }
  hipLaunchKernelGGL(k_bw_odom_update, dim3(B), dim3(1024), 0, s, win, odom, partials, round, n_converged);
  LIO_HIP(hipGetLastError());
}

}  // namespace lio
