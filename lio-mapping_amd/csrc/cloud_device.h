// cloud_device.h — device-side bodies shared by the single-window kernels (cloud_kernels.hip) and the batched-window kernels
// (batch_kernels.hip): the K-NN walk over the cell grid, the plane fit of CalculateFeatures (Estimator.cc:1014-1097), the rows and
// the 6x6 step of CalculateLaserOdom (Estimator.cc:1242-1359).  One definition, so a window solved alone and a window solved inside
// a batch run the same instructions.  The map stage in front of them is here too: the voxel filter's bounds, keys, run heads and centroid
// tile (pcl::VoxelGrid, Estimator.cc:1518-1519), the cell key of a point and what a solve's feature stage starts from.  Every body takes
// pointers already shifted to the window's range (a kernel argument + an offset: global to the compiler, dev.h); the kernels keep what
// differs — where a window's range starts, and what the last tile posts.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstddef>

#include "cloud_kernels.h"
#include "hmath.h"
#include "knn_merge.h"

#if defined(__HIPCC__)
namespace lio {

__device__ inline bool finite3(const float4 &p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }
__device__ inline bool finite3(const Vec3<float> &p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }


// TransformToEnd of one point, x y z only: q_e * (slerp(id, s, q_e).conjugate() * (p - s t)) + t.  Stated once for its two forms:
// the estimator's (Estimator.cc:62-103) normalises the conjugate (:88), the odometry's (PointOdometry.cc:261-292) does not.  What a
// form does with the intensity (strip the ring, strip the fraction, keep both) is the calling kernel's; .w is returned as it came.
template <bool NORMALISE_CONJ>
__device__ __forceinline__ float4 to_end_point(float4 p, float s, const Quat<float> &qe, const Vec3<float> &te) {
  p.x -= s * te.x; p.y -= s * te.y; p.z -= s * te.z;
  Quat<float> qid;
  Quat<float> qs = slerp(qid, s, qe, FLT_EPSILON);
  Quat<float> qc = conj(qs);
  if (NORMALISE_CONJ) qc = normalized(qc);
  Vec3<float> v = rotate(qc, Vec3<float>(p.x, p.y, p.z));
  v = rotate(qe, v);
  p.x = v.x + te.x; p.y = v.y + te.y; p.z = v.z + te.z;
  return p;
}
// The estimator's TransformToEnd (Estimator.cc:62-103) of one point as the cloud carries it: s from the fraction of the intensity; KEEP (:79)
// carries the intensity through, else the ring is stripped.  Stated once for a cloud de-skewed on its own (k_deskew_to_end) and for the clouds
// of a batched push (est_push.hip: k_bp_take_keys).
template <bool KEEP>
__device__ __forceinline__ float4 deskew_to_end_point(float4 p, const Quat<float> &qe, const Vec3<float> &te, float time_factor) {
  float s = time_factor * (p.w - int(p.w));
  if (!KEEP) p.w -= int(p.w);
  return to_end_point<true>(p, s, qe, te);
}
// pcl::transformPointCloud of one point by the row-major 3x4 [R | t]: m00*x + m01*y + m02*z + m03, intensity kept
__device__ __forceinline__ float4 affine_map_point(const float *__restrict__ m, const float4 &p) {
  float4 o;
  o.x = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
  o.y = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
  o.z = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
  o.w = p.w;
  return o;
}
// Position g of a concat of `nseg` segments (pcl::transformPointCloud + `+=`, Estimator.cc:1480-1507, :2602-2615): the segment that holds it,
// the load, the segment's map or none, its intensity.  Stated once for the concat of one window (k_transform_concat), of a batch's local maps
// (k_bw_concat_keys) and of a batch's slides (k_bp_slide); the caller keeps its own range test or clamp of g.  base: the kernel-argument
// pointer the segments' sources are tied to (dev.h: rebase); nullptr where the segments arrive as kernel arguments themselves.
template <class B> __device__ __forceinline__ const float4 *concat_src(B *base, const float4 *p) { return rebase(base, p); }
__device__ __forceinline__ const float4 *concat_src(std::nullptr_t, const float4 *p) { return p; }
template <class B>
__device__ __forceinline__ float4 concat_point(const ConcatSeg *__restrict__ seg, int nseg, int g, B base) {
  int sidx = 0;
  for (int k = 1; k < nseg; ++k)
    if (g >= seg[k].dst_off) sidx = k;
  const ConcatSeg &sg = seg[sidx];
  const float4 p = concat_src(base, sg.src)[g - sg.dst_off];
  float4 o;
  if (sg.identity) o = p;
  else o = affine_map_point(sg.tf.m, p);
  if (sg.set_intensity) o.w = sg.intensity;
  return o;
}
// The odometry's TransformToEnd (PointOdometry.cc:261-292) of point i with the transform_es_ the iterations left on the device; out == in: in
// place.  Stated once for the odometry's own clouds, lio_odom_full_to_end and the full cloud the scan-to-map step takes from the odometry
// (mapping.hip: k_mb_from_odom): the same instructions, so the same bits.
__device__ __forceinline__ void odo_to_end_body(const float4 *in, float4 *out, const int i, const OdomState *__restrict__ st, float time_factor,
                                                int no_deskew) {
  Quat<float> qe(st->T[3], st->T[0], st->T[1], st->T[2]);
  Vec3<float> te(st->T[4], st->T[5], st->T[6]);
  float4 p = in[i];
  float s = time_factor * (p.w - int(p.w));
  if (no_deskew) s = 0;
  p.w = float(int(p.w));
  out[i] = to_end_point<false>(p, s, qe, te);
}
// Point i of a full cloud a take launch writes (cloud_kernels.h: FullTake), through TransformToEnd or, without a state, as it is: k_mb_from_odom
// (mapping.hip) and k_bp_take_keys_dev (est_push.hip).  in, out, st: the record's pointers as the caller resolved them (as read, or dev.h: rebase).
__device__ __forceinline__ void full_take_body(const float4 *in, float4 *out, const int i, const OdomState *st, const ToEnd &e) {
  if (st) odo_to_end_body(in, out, i, st, e.time_factor, e.no_deskew);
  else out[i] = in[i];
}
// PointAssociateToMap (PointMapping.cc:303-314): rot * p + pos in the operation order of rotate (hmath.h), intensity kept
__device__ __forceinline__ float4 rigid_map_point(float4 p, const Quat<float> &q, const Vec3<float> &t) {
  const Vec3<float> v = rotate(q, Vec3<float>(p.x, p.y, p.z));
  return make_float4(v.x + t.x, v.y + t.y, v.z + t.z, p.w);
}

__device__ inline int cell_coord(float v, float inv_cell) { return int(floorf(v * inv_cell)); }
// the cell of (x, y, z) relative to the grid's origin; true when it lies inside the grid
__device__ __forceinline__ bool cell_of(float x, float y, float z, const GridDesc &g, int &cx, int &cy, int &cz) {
  cx = cell_coord(x, g.inv_cell) - g.origin[0];
  cy = cell_coord(y, g.inv_cell) - g.origin[1];
  cz = cell_coord(z, g.inv_cell) - g.origin[2];
  return cx >= 0 && cy >= 0 && cz >= 0 && cx < g.dims[0] && cy < g.dims[1] && cz < g.dims[2];
}
__device__ __forceinline__ uint32_t cell_index(int cx, int cy, int cz, const GridDesc &g) { return uint32_t(cx + g.dims[0] * (cy + g.dims[1] * cz)); }
// the cell a map point is filed under: points outside the grid go to the border cells
__device__ __forceinline__ uint32_t cell_key_clamped(const float4 &p, const GridDesc &g) {
  int cx, cy, cz;
  cell_of(p.x, p.y, p.z, g, cx, cy, cz);
  cx = min(max(cx, 0), g.dims[0] - 1); cy = min(max(cy, 0), g.dims[1] - 1); cz = min(max(cz, 0), g.dims[2] - 1);
  return cell_index(cx, cy, cz, g);
}

// The counting sort by cell of KnnGrid::build, per point, stated once for a grid built alone (k_cell_count, k_cell_place) and for the grids
// of a batch built side by side (GridBatch: k_seg_cell_count, k_seg_cell_place).  Point i takes a slot inside its cell ...
__device__ __forceinline__ void cell_count_point(const float4 *__restrict__ pts, int i, const GridDesc &g, uint32_t *__restrict__ keys,
                                                 uint32_t *__restrict__ slot, int *__restrict__ cnt) {
  const uint32_t c = cell_key_clamped(pts[i], g);
  keys[i] = c;
  slot[i] = uint32_t(atomicAdd(&cnt[c], 1));
}
// ... and, once the counts have been scanned into `starts`, goes to its place with its index in .w and puts its cell's count back to zero
__device__ __forceinline__ void cell_place_point(const float4 *__restrict__ pts, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ slot, int i,
                                                 const int *__restrict__ starts, float4 *__restrict__ sorted, int *__restrict__ cnt) {
  float4 p = pts[i];
  p.w = __int_as_float(i);
  const uint32_t c = keys[i];
  sorted[starts[c] + int(slot[i])] = p;
  cnt[c] = 0;
}

// out[i] = base + in[0] + ... + in[i - 1] for i < n, by ONE workgroup of SEG_SCAN_THREADS threads that walks the table in chunks of
// SEG_SCAN_THREADS * SEG_SCAN_ITEMS entries: a thread adds its own entries, the wavefront scans the threads' sums with shuffles, the
// wavefronts' totals and the carry from chunk to chunk go through LDS.  Nothing outside the workgroup is waited for.  in != out.
#define SEG_SCAN_THREADS 1024
#define SEG_SCAN_ITEMS 4
__device__ __forceinline__ void block_exclusive_scan(const int *__restrict__ in, int *__restrict__ out, int n, int base) {
  __shared__ int wsum[SEG_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = base;
  for (int c0 = 0; c0 < n; c0 += SEG_SCAN_THREADS * SEG_SCAN_ITEMS) {   // (uniform: every thread of the block takes every chunk)
    const int i0 = c0 + tid * SEG_SCAN_ITEMS;
    int v[SEG_SCAN_ITEMS], tsum = 0;
#pragma unroll
    for (int k = 0; k < SEG_SCAN_ITEMS; ++k) { v[k] = i0 + k < n ? in[i0 + k] : 0; tsum += v[k]; }
    int inc = tsum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(inc, off, 64);
      if (lane >= off) inc += u;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEG_SCAN_THREADS / 64; ++w) { const int t = wsum[w]; if (w < wv) before += t; total += t; }
    int run = carry + before + inc - tsum;
#pragma unroll
    for (int k = 0; k < SEG_SCAN_ITEMS; ++k)
      if (i0 + k < n) { out[i0 + k] = run; run += v[k]; }
    carry += total;
    __syncthreads();   // the next chunk rewrites wsum
  }
}

// ------------------------------------------------------------------------------------------------
// pcl::VoxelGrid
// ------------------------------------------------------------------------------------------------
#define VOX_TILE 256                 // threads of every filter kernel = entries of a tile of the sorted keys
#define VOX_KEY_NONE 0xFFFFFFFFu     // sorted key of an entry that holds no point (non-finite): behind every real key

// PCL's voxel index in ABSOLUTE cells floor(p * inverse_leaf), z ZBITS bits | y 11 | x 11, each with a fixed offset: it orders the voxels
// like PCL's own index (cells relative to the cloud's minimum).  False: the point leaves the key's range (`key` is left as it is).
template <int ZBITS>
__device__ __forceinline__ bool vox_abs_key(const float4 &p, float inv_leaf, uint32_t &key) {
  constexpr int ZOFF = 1 << (ZBITS - 1);
  const float cx = floorf(p.x * inv_leaf), cy = floorf(p.y * inv_leaf), cz = floorf(p.z * inv_leaf);
  if (!(fabsf(cx) < 1024.f && fabsf(cy) < 1024.f && fabsf(cz) < float(ZOFF - 1))) return false;
  key = (uint32_t(int(cz) + ZOFF) << 22) | (uint32_t(int(cy) + 1024) << 11) | uint32_t(int(cx) + 1024);
  return true;
}
// A point still in registers taken into the filter: its stored key (NONE: no point, i.e. not finite) and the lane's share (mn, mx, cnt) of
// the bounds; a finite point beyond the key's range raises *flag and keeps NONE.  Stated once for the single-window filter (k_vox_keys_abs),
// the local maps of a batched solve (k_bw_concat_keys) and the clouds of a batched push (k_bp_take_keys).
template <int ZBITS, uint32_t NONE>
__device__ __forceinline__ uint32_t vox_take_point(const float4 &p, float inv_leaf, float (&mn)[3], float (&mx)[3], float &cnt, int *__restrict__ flag) {
  uint32_t key = NONE;
  if (finite3(p)) {
    cnt = 1.f;
    mn[0] = mx[0] = p.x; mn[1] = mx[1] = p.y; mn[2] = mx[2] = p.z;
    if (!vox_abs_key<ZBITS>(p, inv_leaf, key)) *flag = 1;
  }
  return key;
}

// the block's bounds and count of finite points from every lane's (mn, mx, cnt) -> row[0 .. 6]: wave shuffles, then the four waves through LDS
__device__ __forceinline__ void vox_block_partial(float (&mn)[3], float (&mx)[3], float cnt, float *__restrict__ row) {
  __shared__ float sm[7][VOX_TILE / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    for (int d = 0; d < 3; ++d) { mn[d] = fminf(mn[d], __shfl_xor(mn[d], o, 64)); mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], o, 64)); }
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) { for (int d = 0; d < 3; ++d) { sm[d][wv] = mn[d]; sm[3 + d][wv] = mx[d]; } sm[6][wv] = cnt; }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int t = threadIdx.x;
    float v = sm[t][0];
    for (int w = 1; w < VOX_TILE / 64; ++w) v = t < 3 ? fminf(v, sm[t][w]) : (t < 6 ? fmaxf(v, sm[t][w]) : v + sm[t][w]);
    row[t] = v;
  }
}
// The bounds pass of a cloud, per block: block `block` of the cloud's `nb` (cloud_bounds_blocks) takes the finite points of pts[0, n) at the
// stride nb * VOX_TILE -> row[0 .. 6].  Stated once for every cloud whose bounds are asked for on their own (k_seg_bounds, k_cloud_bounds).
__device__ __forceinline__ void cloud_bounds_block(const float4 *__restrict__ pts, int n, int block, int nb, float *__restrict__ row) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float cnt = 0;
  for (int i = block * VOX_TILE + threadIdx.x; i < n; i += nb * VOX_TILE) {
    const float4 p = pts[i];
    if (!finite3(p)) continue;
    cnt += 1.f;
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
  vox_block_partial(mn, mx, cnt, row);
}

// `nb` rows of partials (eight floats each) folded by a VOX_TILE-thread block into the cloud's VoxParams: min, max, PCL's cell bounds and its
// "leaf size too small" guard.  True on thread 0, which holds the result.
__device__ __forceinline__ bool vox_fold_bounds(const float *__restrict__ partial, int nb, float inv_leaf, VoxParams &v) {
  __shared__ float sm[7][VOX_TILE];
  const int t = threadIdx.x;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float cnt = 0;
  for (int b = t; b < nb; b += VOX_TILE) {
    for (int d = 0; d < 3; ++d) { mn[d] = fminf(mn[d], partial[size_t(b) * 8 + d]); mx[d] = fmaxf(mx[d], partial[size_t(b) * 8 + 3 + d]); }
    cnt += partial[size_t(b) * 8 + 6];   // integers below 2^24: exact in any order
  }
  for (int d = 0; d < 3; ++d) { sm[d][t] = mn[d]; sm[3 + d][t] = mx[d]; }
  sm[6][t] = cnt;
  __syncthreads();
  for (int st = VOX_TILE / 2; st > 0; st >>= 1) {
    if (t < st) {
      for (int d = 0; d < 3; ++d) { sm[d][t] = fminf(sm[d][t], sm[d][t + st]); sm[3 + d][t] = fmaxf(sm[3 + d][t], sm[3 + d][t + st]); }
      sm[6][t] += sm[6][t + st];
    }
    __syncthreads();
  }
  if (t != 0) return false;
  long long dd[3];
  for (int d = 0; d < 3; ++d) {
    v.mn[d] = sm[d][0]; v.mx[d] = sm[3 + d][0];
    dd[d] = (long long)((v.mx[d] - v.mn[d]) * inv_leaf) + 1;
    v.minb[d] = int(floorf(v.mn[d] * inv_leaf));
    const int maxb = int(floorf(v.mx[d] * inv_leaf));
    v.divb[d] = maxb - v.minb[d] + 1;
  }
  v.overflow = (sm[6][0] > 0 && dd[0] * dd[1] * dd[2] > (long long)INT_MAX) ? 1 : 0;
  v.n_valid = int(sm[6][0]);
  return true;
}

// entry i (key k) of a window's sorted keys opens a run of equal keys
__device__ __forceinline__ bool vox_is_head(const uint32_t *__restrict__ keys, int i, uint32_t k) {
  return k != VOX_KEY_NONE && (i == 0 || keys[i - 1] != k);
}
// heads in tile `tile` of the n sorted keys -> *count
__device__ __forceinline__ void vox_tile_head_count(const uint32_t *__restrict__ keys, int n, int tile, int *__restrict__ count) {
  __shared__ int swave[VOX_TILE / 64];
  const int i = tile * VOX_TILE + threadIdx.x;
  const uint32_t k = i < n ? keys[i] : VOX_KEY_NONE;
  const unsigned long long b = __ballot(vox_is_head(keys, i, k));
  if ((threadIdx.x & 63) == 0) swave[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) *count = (swave[0] + swave[1]) + (swave[2] + swave[3]);
}

// Centroids of the sorted runs that start in tile `tile`.  The tile's points are gathered into LDS by all lanes at once; the thread of a
// run's first entry then adds the run up in sorted order (stable sort => ascending original index inside a voxel: the within-voxel order
// the oracle fixes) out of LDS, and out of global memory only for the part of a run that leaves the tile.  One thread per run walking
// global memory was a chain of dependent gathers: 57 us on the 150 k-point local map against 4 us like this.
// The output slot of a run = heads in the tiles before this one + heads before it in the tile.  Handed back: this thread's slot and
// whether it opened a run — the last thread of the last tile knows the total, pos + head.
struct VoxSlot { int pos; bool head; };
__device__ __forceinline__ VoxSlot vox_centroid_tile(const float4 *__restrict__ pts, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                     const int *__restrict__ tile_heads, int n, int tile, float4 *__restrict__ out) {
  __shared__ float4 sp[VOX_TILE];
  __shared__ uint32_t sk[VOX_TILE];
  __shared__ int swave[VOX_TILE / 64], sbase[VOX_TILE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int base_i = tile * VOX_TILE, i = base_i + tid;
  int before = 0;
  for (int b = tid; b < tile; b += VOX_TILE) before += tile_heads[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  const uint32_t k = i < n ? keys[i] : VOX_KEY_NONE;
  sk[tid] = k;
  if (k != VOX_KEY_NONE) sp[tid] = pts[vals[i]];
  const bool head = vox_is_head(keys, i, k);
  const unsigned long long hb = __ballot(head);
  if (lane == 0) { swave[wv] = __popcll(hb); sbase[wv] = before; }
  __syncthreads();
  int pos = (sbase[0] + sbase[1]) + (sbase[2] + sbase[3]);
  for (int w = 0; w < wv; ++w) pos += swave[w];
  pos += __popcll(hb & ((1ull << lane) - 1ull));
  if (head) {
    float ax = 0, ay = 0, az = 0, ai = 0;
    int e = tid;
    while (e < VOX_TILE && sk[e] == k) { const float4 p = sp[e]; ax += p.x; ay += p.y; az += p.z; ai += p.w; ++e; }
    int cnt = e - tid;
    if (e == VOX_TILE) {
      int g = base_i + VOX_TILE;
      while (g < n && keys[g] == k) { const float4 p = pts[vals[g]]; ax += p.x; ay += p.y; az += p.z; ai += p.w; ++g; ++cnt; }
    }
    const float c = float(cnt);
    out[pos] = make_float4(ax / c, ay / c, az / c, ai / c);
  }
  return VoxSlot{pos, head};
}

// ---- the filter's sort of (key, index) pairs: a sample sort (cloud_kernels.h states the sizing rule)
#define VSORT_THREADS 256            // threads of the kernels that sort in registers
#define VSORT_SCATTER_THREADS 512    // threads of the bucket scatter, VSORT_SCATTER_ITEMS points each
#define VSORT_SCATTER_ITEMS 2

// the value of lane (byte_addr / 4) of the wave, both halves of a pair
__device__ __forceinline__ unsigned long long vsort_from_lane(unsigned long long v, int byte_addr) {
  const uint32_t lo = uint32_t(__builtin_amdgcn_ds_bpermute(byte_addr, int(uint32_t(v))));
  const uint32_t hi = uint32_t(__builtin_amdgcn_ds_bpermute(byte_addr, int(uint32_t(v >> 32))));
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// VSORT_THREADS * E pairs sorted ascending by a bitonic network, by a block of VSORT_THREADS threads: thread t holds the entries
// t E + e in registers, before and after.  A step with stride j pairs entry i with i ^ j: inside the thread for j < E (no traffic at
// all), in another lane of the wave for E <= j < 64 E (one lane permute per half), and only for j >= 64 E in another wave (through `lds`,
// VSORT_THREADS * E entries, two barriers).  Both partners of a cross-thread step hold all E partners of each other, so each keeps the
// minima or the maxima.  (Through LDS alone every step was a dependent read - write - barrier chain: 285 ns a step.)
template <int E>
__device__ __forceinline__ void vsort_block(unsigned long long (&v)[E], unsigned long long *__restrict__ lds) {
  constexpr int P = VSORT_THREADS * E;
  const int base = int(threadIdx.x) * E, lane = int(threadIdx.x) & 63;
#pragma unroll 1
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll 1
    for (int j = k >> 1; j >= 64 * E; j >>= 1) {
      __syncthreads();   // the readers of the step before are done
#pragma unroll
      for (int e = 0; e < E; ++e) lds[base + e] = v[e];
      __syncthreads();
      const bool keep_min = ((base & j) == 0) == ((base & k) == 0);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned long long o = lds[(base ^ j) + e];
        if ((o < v[e]) == keep_min) v[e] = o;   // equal only for two fillers: either stays
      }
    }
#pragma unroll 1
    for (int j = min(k >> 1, 32 * E); j >= E; j >>= 1) {
      const bool keep_min = ((base & j) == 0) == ((base & k) == 0);
      const int partner = (lane ^ (j / E)) << 2;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned long long o = vsort_from_lane(v[e], partner);
        if ((o < v[e]) == keep_min) v[e] = o;
      }
    }
#pragma unroll
    for (int j = E / 2; j > 0; j >>= 1) {
      if (j < k) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if ((e & j) == 0) {
            const bool asc = ((base + e) & k) == 0;
            const unsigned long long x = v[e], y = v[e | j];
            if ((x > y) == asc) { v[e] = y; v[e | j] = x; }
          }
        }
      }
    }
  }
}

// the E for m entries: the smallest power of two with VSORT_THREADS * E >= m
__device__ __forceinline__ int vsort_items_for(int m) {
  int E = 1;
  while (VSORT_THREADS * E < m) E <<= 1;
  return E;
}

// m pairs (key << 32 | index) at src sorted and written to keys_out / vals_out at `off`; m <= VSORT_THREADS * E; lds: VSORT_THREADS * E pairs
template <int E>
__device__ __forceinline__ void vsort_pairs_sort_store(const unsigned long long *__restrict__ src, int m, unsigned long long *__restrict__ lds,
                                                       uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out, int off) {
  unsigned long long v[E];
  const int base = int(threadIdx.x) * E;
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = base + e < m ? src[base + e] : ~0ull;   // behind every pair: an index is below 2^32 - 1
  vsort_block<E>(v, lds);
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (base + e < m) { keys_out[off + base + e] = uint32_t(v[e] >> 32); vals_out[off + base + e] = uint32_t(v[e]); }
}
// The number of pairs (ss[j], j), j < S, below `mine`: the sorted position of `mine` among them.  ss: LDS, S a multiple of four;
// VSORT_RANK_LANES neighbouring lanes (part = 0 ..) share the count and all get it.
#define VSORT_RANK_LANES 16
__device__ __forceinline__ int vsort_rank_of(const uint32_t *__restrict__ ss, int S, int part, unsigned long long mine) {
  int rank = 0;
  const uint4 *ss4 = reinterpret_cast<const uint4 *>(ss);
  for (int q = part; q < S / 4; q += VSORT_RANK_LANES) {
    const uint4 k4 = ss4[q];
    const uint32_t j = uint32_t(q) * 4;
    rank += ((static_cast<unsigned long long>(k4.x) << 32) | j) < mine;
    rank += ((static_cast<unsigned long long>(k4.y) << 32) | (j + 1)) < mine;
    rank += ((static_cast<unsigned long long>(k4.z) << 32) | (j + 2)) < mine;
    rank += ((static_cast<unsigned long long>(k4.w) << 32) | (j + 3)) < mine;
  }
#pragma unroll
  for (int o = VSORT_RANK_LANES / 2; o > 0; o >>= 1) rank += __shfl_xor(rank, o, 64);
  return rank;
}

// Splitters of the n keys for NB buckets.  The sample: S = OVERSAMPLE * NB keys at the fixed positions floor((j + 0.5) n / S).  Splitter
// b (b = 1 .. NB - 1) is entry OVERSAMPLE * b of the sorted sample, found without sorting: the rank of sample i is the number of samples
// below it as pairs (key, i), counted by VSORT_RANK_LANES lanes over the whole sample in LDS (`ss`, S keys); the sample whose rank is
// OVERSAMPLE * b writes splitter b.  A block ranks VSORT_THREADS / VSORT_RANK_LANES samples; no block waits for another.
// (One block sorting the sample was the longest kernel of the three: 13 us for 1384 keys, and it grows with NB.)
template <int OVERSAMPLE>
__device__ __forceinline__ void vsort_pick_splitters(const uint32_t *__restrict__ keys, int n, int NB, uint32_t *__restrict__ ss,
                                                     uint32_t *__restrict__ splitters) {
  const int S = OVERSAMPLE * NB;
  static_assert(OVERSAMPLE % 4 == 0, "the sample is read four keys at a time");
  // floor((2 t + 1) n / (2 S)) with n = q S + r is t q + floor((q S + (2 t + 1) r) / (2 S)): 32-bit arithmetic (r < S <= 8192, n < 2^19), no 64-bit division per load
  const uint32_t q = uint32_t(n) / uint32_t(S), r = uint32_t(n) % uint32_t(S);
  for (int t = threadIdx.x; t < S; t += VSORT_THREADS) ss[t] = keys[uint32_t(t) * q + (q * uint32_t(S) + (2u * uint32_t(t) + 1u) * r) / (2u * uint32_t(S))];
  __syncthreads();
  const int i = blockIdx.x * (VSORT_THREADS / VSORT_RANK_LANES) + int(threadIdx.x) / VSORT_RANK_LANES, part = int(threadIdx.x) % VSORT_RANK_LANES;
  const unsigned long long mine = i < S ? (static_cast<unsigned long long>(ss[i]) << 32) | uint32_t(i) : 0ull;
  const int rank = vsort_rank_of(ss, S, part, mine);
  if (part == 0 && i < S && rank >= OVERSAMPLE && rank % OVERSAMPLE == 0) splitters[rank / OVERSAMPLE - 1] = uint32_t(mine >> 32);
}

// bucket of a key = number of splitters <= key (upper bound): equal keys share a bucket
__device__ __forceinline__ int vsort_bucket_of(const uint32_t *__restrict__ spl, int NB, uint32_t key) {
  int lo = 0, hi = NB - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (spl[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------
// what a solve's feature stage starts from
// ------------------------------------------------------------------------------------------------
// feature flags valid[0, n) <- 0, sixteen bytes per lane of a VOX_TILE-thread block (valid is 16-byte aligned)
__device__ __forceinline__ void clear_valid_block(uint8_t *__restrict__ valid, size_t n) {
  const size_t i = (size_t(blockIdx.x) * VOX_TILE + threadIdx.x) * 16;
  if (i + 16 <= n) *reinterpret_cast<uint4 *>(valid + i) = make_uint4(0, 0, 0, 0);
  else for (size_t k = i; k < n; ++k) valid[k] = 0;
}
// the newest frame's Gauss-Newton state = its local transform T (eight floats), every other word zero, by the block's first lanes;
// converged: the state of a frame that has nothing to iterate on
__device__ __forceinline__ void odom_state_init(OdomState *__restrict__ st, const float *__restrict__ T, bool converged) {
  static_assert(offsetof(OdomState, T) == 0 && sizeof(OdomState) <= VOX_TILE * 4, "state layout: T first, the rest zero");
  unsigned *o = reinterpret_cast<unsigned *>(st);
  const int nw = int(sizeof(OdomState) / 4);
  if (int(threadIdx.x) < nw) {
    unsigned v = threadIdx.x < 8 ? __float_as_uint(T[threadIdx.x]) : 0u;
    if (converged && threadIdx.x == offsetof(OdomState, converged) / 4) v = 1u;
    o[threadIdx.x] = v;
  }
}


// ------------------------------------------------------------------------------------------------
// CalculateFeatures (surf branch)
// ------------------------------------------------------------------------------------------------
// LPQ lanes cooperate on one query: sub-lane `sub` scans candidates sub, sub+LPQ, ... of each 3-cell x-run
// (one contiguous, coalesced stream per query group), keeps its own top-K, then the LPQ partial lists are
// merged by xor-shuffles.  The total order (d2, original index) makes the result independent of the split:
// bit-identical to the single-lane scan.  The serial dependent-load chain per lane shrinks LPQ-fold, which
// is what bounds this kernel (a query touches ~100 candidates; maps are L2-resident).
#define FEAT_LPQ 8
#ifndef KNN_BATCH
#define KNN_BATCH 4   // candidate loads in flight per lane
#endif
// Top-K list ordered by (squared distance, original index).  Both live in ONE 64-bit key — the distance's bit pattern (non-negative
// floats order like their bits) above the index — so a comparison is one v_cmp_lt_u64 instead of three compares and two logic
// ops, and a compare-exchange moves three registers instead of three guarded by that chain.  The search kernels are bound by
// vector-instruction issue (3473 VALU instructions per wave measured in k_odom_round before this form).
__device__ __forceinline__ unsigned long long knn_key(float d, int idx) {
  return (static_cast<unsigned long long>(__float_as_uint(d)) << 32) | static_cast<unsigned int>(idx);
}
template <int K>
__device__ __forceinline__ void knn_insert(unsigned long long key, int j, unsigned long long (&bk)[K], int (&bj)[K]) {
  if (key < bk[K - 1]) {
    bk[K - 1] = key; bj[K - 1] = j;
#pragma unroll
    for (int k = K - 1; k > 0; --k) {
      const bool sw = bk[k - 1] > bk[k];
      const unsigned long long tk = sw ? bk[k - 1] : bk[k];
      const int tj = sw ? bj[k - 1] : bj[k];
      bk[k - 1] = sw ? bk[k] : bk[k - 1];
      bj[k - 1] = sw ? bj[k] : bj[k - 1];
      bk[k] = tk; bj[k] = tj;
    }
  }
}
// The walk is organised around memory latency (the kernel is bound by dependent loads, not by bandwidth: a wave used to issue
// one candidate load, wait for it, compare, and only then issue the next — ~36 round trips per query):
//   1. the run bounds of the nine x-runs (3 x-adjacent cells each) of the 27-cell block: 18 independent loads, one round trip;
//   2. the nine runs seen as ONE flat candidate list of length T; sub-lane `sub` takes the flat positions sub, sub + LPQ, ...
//      and keeps KNN_BATCH loads in flight (position -> address by a select chain over the nine prefix sums, no indexed
//      register arrays), i.e. ceil(T / (LPQ * KNN_BATCH)) round trips (3-4 at ~100 candidates);
//   3. xor-shuffle merge of the LPQ partial lists.
// The candidate SET and the total order (d2, original index) are unchanged, so the result is bit-identical to the serial walk.
// With four or more lanes per query and K = 5 nothing goes through knn_insert: a trip's four candidates enter by ONE knn_merge4 and a
// butterfly stage is ONE knn_merge5 (knn_merge.h: fixed networks — ten compare-exchanges and four selects for a trip, five and five for
// a stage, against the sixteen and twenty guarded compare-exchanges of four and five insertions; docs/knn_merge.md has the counts and
// the kernel times).  The five smallest of a set of distinct keys and their order are unique, so the lists keep their bits.
template <int K, int LPQ>
__device__ inline void knn_scan_group(const Vec3<float> &q, bool active, int sub, const float4 *__restrict__ map,
                                      const int *__restrict__ cells, const GridDesc &g, float (&bd)[K], int (&bi)[K], int (&bj)[K]) {
  unsigned long long bk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { bk[k] = knn_key(INFINITY, INT_MAX); bj[k] = 0; }
  int cx, cy, cz;
  cell_of(q.x, q.y, q.z, g, cx, cy, cz);
  // a query with a NaN / inf coordinate has no cell (the float -> int conversion above is not defined for it): like a query outside
  // the grid it finds nothing and only takes part in the shuffles below.  (cell_of's own inside test, written out in one chain with the
  // finite test: taken from its return value, the one-lane search kernels compile to 5-8 % more instructions.)
  if (!finite3(q) || cx < 0 || cy < 0 || cz < 0 || cx >= g.dims[0] || cy >= g.dims[1] || cz >= g.dims[2]) active = false;
  if (active) {
    // cells x-1..x+1 have consecutive ids => their points are one contiguous run of the cell-sorted array
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dims[0] - 1);
    if constexpr (LPQ <= 2) {
      // throughput regime (one or two lanes per query — the keyframe batch: tens of millions of queries keep every CU full and
      // the kernel runs under a 64-VGPR cap): the plain run-by-run walk, nothing held in batch registers.  Measured there
      // (profiles/r2_pmc_sq_search_kernels.md): 5-8 k vector instructions per wave, 70 % of the kernel's time in VALU issue, and
      // with a query per lane the ~35-instruction insertion runs for every candidate (some lane always inserts).  So whole
      // rows are skipped: the query's own row is walked first, then the rows sharing a face, then the corners, and a row is
      // entered only if the distance from the query to that row of cells (a lower bound for every point in it, shrunk by
      // 1e-3 cell against rounding of the cell arithmetic) does not exceed the current fifth-best distance.  Exact: a skipped
      // row cannot hold a candidate that would enter the list.
      const float uy = q.y * g.inv_cell, uz = q.z * g.inv_cell;
      const float fy = uy - floorf(uy), fz = uz - floorf(uz);
      const float cell = 1.0f / g.inv_cell;
      const float ey_lo = fmaxf(fy - 1e-3f, 0.f) * cell, ey_hi = fmaxf(1.0f - fy - 1e-3f, 0.f) * cell;
      const float ez_lo = fmaxf(fz - 1e-3f, 0.f) * cell, ez_hi = fmaxf(1.0f - fz - 1e-3f, 0.f) * cell;
      // Three phases — own row | the four rows sharing a face | the four corner rows — and inside a phase ONE flat candidate list over
      // its (up to four) runs: a wave then runs a phase to its slowest lane's SUM of run lengths, not to the sum over the rows of the
      // slowest lane of each (measured on the headline map, 64 consecutive queries: 130 wave iterations row by row, 73 flat, 42 the mean
      // lane).  A row's bound is tested when its phase starts (after the own row / after the face rows), its two table entries are
      // loaded together with the phase's other rows'.  Round 6: features 4.91 -> 4.28 ms, rounds 5.93 -> 4.84 ms at 512 windows, keyframe
      // batch 38.1 k -> 47.2 k keyframes/s.
      auto walk = [&](int j) {
        const float4 pc = map[j];
        float ddx = pc.x - q.x, ddy = pc.y - q.y, ddz = pc.z - q.z;
        float d = ddx * ddx;
        d += ddy * ddy;
        d += ddz * ddz;
        knn_insert<K>(knn_key(d, __float_as_int(pc.w)), j, bk, bj);
      };
      {   // own row
        const int row = g.dims[0] * (cy + g.dims[1] * cz);
        const int a = cells[row + x0], e = cells[row + x1 + 1];
        for (int j = a + sub; j < e; j += LPQ) walk(j);
      }
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0, c1 = 0, c2 = 0, c3 = 0, T = 0;
        const float worst = __uint_as_float(static_cast<unsigned int>(bk[K - 1] >> 32));
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int r = 1 + 4 * ph + qq;
          // (dy, dz) + 1 packed two bits each: own row, four face rows, four corner rows
          const int dy = int((0x22161u >> (2 * r)) & 3u) - 1, dz = int((0x28215u >> (2 * r)) & 3u) - 1;
          const int z = cz + dz, y = cy + dy;
          const float ey = dy < 0 ? ey_lo : (dy > 0 ? ey_hi : 0.f), ez = dz < 0 ? ez_lo : (dz > 0 ? ez_hi : 0.f);
          const bool on = z >= 0 && z < g.dims[2] && y >= 0 && y < g.dims[1] && !(ey * ey + ez * ez > worst);
          const int row = on ? g.dims[0] * (y + g.dims[1] * z) : 0;
          // this sub-lane's candidates of the run: positions a + sub, a + sub + LPQ, ... (every run is dealt out from ITS start: the
          // sub-lanes of a query may skip different rows, their lists need not be the same)
          const int a = (on ? cells[row + x0] : 0) + sub, e = on ? cells[row + x1 + 1] : 0;
          const int len = e > a ? (e - a + LPQ - 1) / LPQ : 0;
          if (qq == 0) { s0 = a; c1 = len; }
          if (qq == 1) { s1 = a; c2 = c1 + len; }
          if (qq == 2) { s2 = a; c3 = c2 + len; }
          if (qq == 3) { s3 = a; T = c3 + len; }
        }
        for (int f = 0; f < T; ++f) {
          int j = s0 + f * LPQ;
          j = f >= c1 ? s1 + (f - c1) * LPQ : j;
          j = f >= c2 ? s2 + (f - c2) * LPQ : j;
          j = f >= c3 ? s3 + (f - c3) * LPQ : j;
          walk(j);
        }
      }
    } else {
      int rs[9], pre[10];
      pre[0] = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r) {
        const int z = cz + r / 3 - 1, y = cy + r % 3 - 1;
        const bool in = z >= 0 && z < g.dims[2] && y >= 0 && y < g.dims[1];
        const int row = g.dims[0] * (y + g.dims[1] * z);
        const int a = in ? cells[row + x0] : 0, b = in ? cells[row + x1 + 1] : 0;
        rs[r] = a;
        pre[r + 1] = b - a;   // run length for now
      }
#pragma unroll
      for (int r = 0; r < 9; ++r) pre[r + 1] = pre[r] + max(pre[r + 1], 0);
      const int T = pre[9];
      for (int base = sub; base < T; base += LPQ * KNN_BATCH) {
        float4 p[KNN_BATCH];
        int jj[KNN_BATCH];
#pragma unroll
        for (int b = 0; b < KNN_BATCH; ++b) {
          const int f = base + b * LPQ;
          int j = f + rs[0];
#pragma unroll
          for (int r = 1; r < 9; ++r) j = f >= pre[r] ? f - pre[r] + rs[r] : j;
          jj[b] = f < T ? j : -1;
          p[b] = f < T ? map[j] : make_float4(0, 0, 0, 0);
        }
        if constexpr (K == 5 && KNN_BATCH == 4) {
          // the trip's four candidates in one merge; a position past the list's end carries the sentinel's key (it cannot enter, like a
          // NaN distance, whose key lies above the sentinel's), and the wave skips the merge when no lane holds a key below its fifth
          unsigned long long ck[KNN_BATCH];
          bool any = false;
#pragma unroll
          for (int b = 0; b < KNN_BATCH; ++b) {
            float ddx = p[b].x - q.x, ddy = p[b].y - q.y, ddz = p[b].z - q.z;
            float d = ddx * ddx;
            d += ddy * ddy;
            d += ddz * ddz;
            ck[b] = jj[b] < 0 ? knn_key(INFINITY, INT_MAX) : knn_key(d, __float_as_int(p[b].w));
            any = any || ck[b] < bk[K - 1];
          }
          if (any) knn_merge4(bk, bj, ck, jj);
        } else {
#pragma unroll
          for (int b = 0; b < KNN_BATCH; ++b) {
            if (jj[b] < 0) continue;
            float ddx = p[b].x - q.x, ddy = p[b].y - q.y, ddz = p[b].z - q.z;
            float d = ddx * ddx;
            d += ddy * ddy;
            d += ddz * ddz;
            knn_insert<K>(knn_key(d, __float_as_int(p[b].w)), jj[b], bk, bj);
          }
        }
      }
    }
  }
  // butterfly merge of the LPQ partial lists (every lane of the wave takes part in the shuffles)
#pragma unroll
  for (int m = 1; m < LPQ; m <<= 1) {
    unsigned long long ok[K]; int oj[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned int lo = __shfl_xor(static_cast<unsigned int>(bk[k]), m, 64), hi = __shfl_xor(static_cast<unsigned int>(bk[k] >> 32), m, 64);
      ok[k] = (static_cast<unsigned long long>(hi) << 32) | lo;
      oj[k] = __shfl_xor(bj[k], m, 64);
    }
    if constexpr (K == 5 && LPQ >= 4) {
      knn_merge5(bk, bj, ok, oj);
    } else {
#pragma unroll
      for (int c = 0; c < K; ++c) knn_insert<K>(ok[c], oj[c], bk, bj);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) { bd[k] = __uint_as_float(static_cast<unsigned int>(bk[k] >> 32)); bi[k] = int(static_cast<unsigned int>(bk[k])); }
}

struct FeatScalars { float min_match_sq_dis, min_plane_dis; int mapping_mode; float fixed_pz[3]; };
__device__ __forceinline__ FeatScalars feat_scalars(const FeatArgs &a) {
  return FeatScalars{a.min_match_sq_dis, a.min_plane_dis, a.mapping_mode, {a.fixed_pz[0], a.fixed_pz[1], a.fixed_pz[2]}};
}
// what the owner lane (sub == 0 of an in-range query) of features_eval comes back with
struct FeatResult { bool owner; uint8_t ok; float4 c; float sc; float4 abs; float4 po; int slot; };
// The fit half of a surf feature (Estimator.cc:1021-1097 / PointMapping.cc:503-619) for ONE query whose five nearest map
// points are known: 5x3 column-pivoted QR plane fit, validity, score, FOV.  q, t: the frame's transform; po: the stack point;
// sel: its image; bd4 / bi4: distance and original index of the fifth neighbour; bj: positions of the five in `map`.
template <bool MAPPING>
__device__ __forceinline__ FeatResult features_fit(const FeatScalars &a, int slot, const Quat<float> &q, const Vec3<float> &t, const float4 &po,
                                                   const Vec3<float> &sel, float bd4, int bi4, const int (&bj)[5], const float4 *__restrict__ map) {
  FeatResult res;
  res.owner = true; res.ok = 0; res.c = make_float4(0, 0, 0, 0); res.sc = 0; res.abs = make_float4(0, 0, 0, 0); res.po = po; res.slot = slot;
  uint8_t ok = 0;
  float4 c = make_float4(0, 0, 0, 0);
  float sc = 0;
  if (bi4 != INT_MAX && bd4 < a.min_match_sq_dis) {
    float A[15], B[5] = {-1, -1, -1, -1, -1}, X[3];
    float nx[5], ny[5], nz[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float4 pn = map[bj[j]];
      nx[j] = pn.x; ny[j] = pn.y; nz[j] = pn.z;
      A[j * 3 + 0] = pn.x; A[j * 3 + 1] = pn.y; A[j * 3 + 2] = pn.z;
    }
    qr_solve<float, 5, 3>(A, B, X, FLT_EPSILON);
    float pa = X[0], pb = X[1], pc = X[2], pd = 1;
    float ps = sqrtf(pa * pa + pb * pb + pc * pc);
    pa /= ps; pb /= ps; pc /= ps; pd /= ps;
    bool plane_valid = true;
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (!(fabsf(pa * nx[j] + pb * ny[j] + pc * nz[j] + pd) <= a.min_plane_dis)) plane_valid = false;   // a NaN distance (0 * NaN: a NaN coordinate in a column the rank cut dropped) is no plane
    if (plane_valid) {
      float pd2 = pa * sel.x + pb * sel.y + pc * sel.z + pd;
      float s = 1 - 0.9f * fabsf(pd2) / sqrtf(sqrtf(sel.x * sel.x + sel.y * sel.y + sel.z * sel.z));
      // FOV test (+-60 deg about the sensor z axis, Estimator.cc:1063-1086)
      Vec3<float> rz = rotate(q, Vec3<float>(0.f, 0.f, 10.f));
      Vec3<float> pz(rz.x + t.x, rz.y + t.y, rz.z + t.z);
      if (MAPPING) pz = Vec3<float>(a.fixed_pz[0], a.fixed_pz[1], a.fixed_pz[2]);
      float dx1 = t.x - sel.x, dy1 = t.y - sel.y, dz1 = t.z - sel.z;
      float side1 = dx1 * dx1 + dy1 * dy1 + dz1 * dz1;
      float dx2 = pz.x - sel.x, dy2 = pz.y - sel.y, dz2 = pz.z - sel.z;
      float side2 = dx2 * dx2 + dy2 * dy2 + dz2 * dz2;
      float check1 = 100.0f + side1 - side2 - 10.0f * sqrtf(3.0f) * sqrtf(side1);
      float check2 = 100.0f + side1 - side2 + 10.0f * sqrtf(3.0f) * sqrtf(side1);
      bool in_fov = check1 < 0 && check2 > 0;
      if (double(s) > 0.1 && in_fov) {
        ok = 1;
        c = make_float4(s * pa, s * pb, s * pc, s * pd);
        sc = s;
        if (MAPPING) {  // PointMapping.cc:572-592
          const bool pos = pd2 > 0 || a.mapping_mode == 2;  // MapBuilder::OptimizeMap keeps the fitted sign (MapBuilder.cc:786-789)
          c = pos ? make_float4(s * pa, s * pb, s * pc, s * pd2) : make_float4(-s * pa, -s * pb, -s * pc, -s * pd2);
          res.abs = pos ? make_float4(pa, pb, pc, pd) : make_float4(-pa, -pb, -pc, -pd);
        }
      }
    }
  }
  res.ok = ok; res.c = c; res.sc = sc;
  return res;
}
template <bool MAPPING, int LPQ>
__device__ __forceinline__ FeatResult features_eval(const FeatFrame fr, const FeatScalars a, int block_x, const float *__restrict__ transforms,
                                                    const float4 *__restrict__ map, const int *__restrict__ cells, const GridDesc &g) {
  FeatResult res;
  res.owner = false; res.ok = 0; res.c = make_float4(0, 0, 0, 0); res.sc = 0; res.abs = make_float4(0, 0, 0, 0); res.po = make_float4(0, 0, 0, 0); res.slot = 0;
  const int gt = block_x * blockDim.x + threadIdx.x;
  const int it = gt / LPQ, sub = gt % LPQ;
  const bool active = it < fr.M;
  const int i = (active && fr.order) ? int(fr.order[it]) - fr.slot_off : it;   // (FeatFrame::order: which query this lane group works on)
  const float *tp = transforms + 8 * fr.tf_index;
  Quat<float> q(tp[3], tp[0], tp[1], tp[2]);
  Vec3<float> t(tp[4], tp[5], tp[6]);
  float4 po = active ? fr.stack[i] : make_float4(0, 0, 0, 0);
  Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
  Vec3<float> sel(r.x + t.x, r.y + t.y, r.z + t.z);
  float bd[5]; int bi[5], bj[5];
  knn_scan_group<5, LPQ>(sel, active, sub, map, cells, g, bd, bi, bj);
  if (!active || sub != 0) return res;
  return features_fit<MAPPING>(a, fr.slot_off + i, q, t, po, sel, bd[4], bi[4], bj, map);
}
template <bool MAPPING, int LPQ>
__device__ __forceinline__ void features_body(const FeatFrame fr, const FeatScalars a, int block_x, const float *__restrict__ transforms,
                                              const float4 *__restrict__ map, const int *__restrict__ cells, const GridDesc &g,
                                              uint8_t *__restrict__ valid, float4 *__restrict__ coef, float *__restrict__ score,
                                              float4 *__restrict__ abs_coef) {
  const FeatResult r = features_eval<MAPPING, LPQ>(fr, a, block_x, transforms, map, cells, g);
  if (!r.owner) return;
  valid[r.slot] = r.ok; coef[r.slot] = r.c;
  if (score) score[r.slot] = r.sc;
  if (MAPPING && abs_coef && r.ok) abs_coef[r.slot] = r.abs;
}

// CalculateFeatures for every frame of the launch (blockIdx.y).  Two phases, like k_odom_round below: FEAT_THREADS lanes search
// with LPQ lanes per query and park each query's five neighbours in LDS, then ONE wave runs the plane fit with a query per lane
// (the fit used to occupy one lane in LPQ of every wave while costing all of its issue slots — these kernels are bound by
// vector-instruction issue, not by memory).
#define FEAT_THREADS 256
template <bool MAPPING, int LPQ, int THREADS = FEAT_THREADS>
__device__ __forceinline__ void features_block(const FeatFrame fr, const FeatScalars fs, int block_x, const float *__restrict__ transforms, const float4 *__restrict__ map,
                                               const int *__restrict__ cells, const GridDesc &g, uint8_t *__restrict__ valid,
                                               float4 *__restrict__ coef, float *__restrict__ score, float4 *__restrict__ abs_coef) {
  constexpr int QPB = THREADS / LPQ;
  static_assert(QPB <= 64, "the fit phase is one wave");
  __shared__ int s_bj[QPB][5];
  __shared__ float s_bd4[QPB];
  __shared__ int s_bi4[QPB];
  if (block_x * QPB >= fr.M) return;
  const float *tp = transforms + 8 * fr.tf_index;
  const Quat<float> q(tp[3], tp[0], tp[1], tp[2]);
  const Vec3<float> t(tp[4], tp[5], tp[6]);
  {
    const int ql = int(threadIdx.x) / LPQ, sub = int(threadIdx.x) % LPQ;
    const int i = block_x * QPB + ql;
    const bool active = i < fr.M;
    const float4 po = active ? fr.stack[i] : make_float4(0, 0, 0, 0);
    const Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
    const Vec3<float> sel(r.x + t.x, r.y + t.y, r.z + t.z);
    float bd[5]; int bi[5], bj[5];
    knn_scan_group<5, LPQ>(sel, active, sub, map, cells, g, bd, bi, bj);
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 5; ++k) s_bj[ql][k] = bj[k];
      s_bd4[ql] = bd[4]; s_bi4[ql] = bi[4];
    }
  }
  __syncthreads();
  const int ql = threadIdx.x, i = block_x * QPB + ql;
  if (ql >= QPB || i >= fr.M) return;
  const float4 po = fr.stack[i];
  const Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
  const Vec3<float> sel(r.x + t.x, r.y + t.y, r.z + t.z);
  int bj[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) bj[k] = s_bj[ql][k];
  const FeatResult res = features_fit<MAPPING>(fs, fr.slot_off + i, q, t, po, sel, s_bd4[ql], s_bi4[ql], bj, map);
  valid[res.slot] = res.ok; coef[res.slot] = res.c;
  if (score) score[res.slot] = res.sc;
  if (MAPPING && abs_coef && res.ok) abs_coef[res.slot] = res.abs;
}

// one row of (mat_A | mat_B) of a selected feature (Estimator.cc:1272-1301): a[6] and b.  Also called by the test hook lio_gn_rows_map.
__device__ __forceinline__ void odom_row_form(const float4 po, const float4 c, const Quat<float> &q, const Vec3<float> &t, const Mat3<float> &Rm,
                                              const Mat3<float> &Rinv, int b_from_coef, float (&a)[6], float &bb) {
  Vec3<float> p(po.x, po.y, po.z), w(c.x, c.y, c.z);
  Mat3<float> RS = Rm * skew(p);
  a[0] = -(w.x * RS(0, 0) + w.y * RS(1, 0) + w.z * RS(2, 0));
  a[1] = -(w.x * RS(0, 1) + w.y * RS(1, 1) + w.z * RS(2, 1));
  a[2] = -(w.x * RS(0, 2) + w.y * RS(1, 2) + w.z * RS(2, 2));
  if (b_from_coef == 2) {  // MapBuilder::OptimizeMap (MapBuilder.cc:903-914): (-w^T R skew(p)) R^-1 diag(5e-3, 5e-3, 1)
    const float t0 = a[0], t1 = a[1], t2 = a[2];
    a[0] = (t0 * Rinv(0, 0) + t1 * Rinv(1, 0) + t2 * Rinv(2, 0)) * 5e-3f;
    a[1] = (t0 * Rinv(0, 1) + t1 * Rinv(1, 1) + t2 * Rinv(2, 1)) * 5e-3f;
    a[2] = (t0 * Rinv(0, 2) + t1 * Rinv(1, 2) + t2 * Rinv(2, 2)) * 1.f;
  }
  a[3] = w.x; a[4] = w.y; a[5] = w.z;
  Vec3<float> rp = rotate(q, p);
  float d2 = w.x * (rp.x + t.x) + w.y * (rp.y + t.y) + w.z * (rp.z + t.z) + c.w;
  bb = b_from_coef ? -c.w : -d2;
}
// a row added to the 21 + 6 + 1 running sums
__device__ __forceinline__ void odom_row_add(const float (&a)[6], const float bb, double (&acc)[28]) {
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int cc = r; cc < 6; ++cc) acc[k++] += double(a[r] * a[cc]);
#pragma unroll
  for (int r = 0; r < 6; ++r) acc[21 + r] += double(a[r] * bb);
  acc[27] += 1.0;
}
__device__ __forceinline__ void odom_row_accumulate(const float4 po, const float4 c, const Quat<float> &q, const Vec3<float> &t, const Mat3<float> &Rm,
                                                    const Mat3<float> &Rinv, int b_from_coef, double (&acc)[28]) {
  float a[6], bb;
  odom_row_form(po, c, q, t, Rm, Rinv, b_from_coef, a, bb);
  odom_row_add(a, bb, acc);
}


__device__ __forceinline__ void odom_update_from_sums(const double *ssum, OdomState *st, int iter, int min_rows, int left_update) {
  if (threadIdx.x != 0) return;
  double sum[28];
  for (int k = 0; k < 28; ++k) sum[k] = ssum[k];
  st->nsel = int(sum[27]);
  if (min_rows > 0 && st->nsel < min_rows) { st->iters = iter + 1; return; }
  float AtA[36], AtB[6];
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) { AtA[r * 6 + c] = float(sum[k]); AtA[c * 6 + r] = float(sum[k]); ++k; }
  for (int r = 0; r < 6; ++r) AtB[r] = float(sum[21 + r]);
  float Ac[36], Bc[6], X[6];
  for (int i = 0; i < 36; ++i) Ac[i] = AtA[i];
  for (int i = 0; i < 6; ++i) Bc[i] = AtB[i];
  qr_solve<float, 6, 6>(Ac, Bc, X, FLT_EPSILON);
  if (iter == 0) {
    const int kz = count_eigs_below<6>(AtA, 100.0);
    st->kz = kz;
    st->degenerate = kz > 0;
  }
  if (st->degenerate)
    for (int i = 0; i < st->kz; ++i) X[i] = 0.f;  // matP = diag(0..0,1..1) (A.6)
  Quat<float> q(st->T[3], st->T[0], st->T[1], st->T[2]);
  Quat<float> R0 = normalized(q);
  Vec3<float> t(st->T[4], st->T[5], st->T[6]);
  t.x += X[3]; t.y += X[4]; t.z += X[5];
  q = left_update ? deltaQ(Vec3<float>(X[0], X[1], X[2])) * q : q * deltaQ(Vec3<float>(X[0], X[1], X[2]));
  if (!isfinite(t.x)) t.x = 0;
  if (!isfinite(t.y)) t.y = 0;
  if (!isfinite(t.z)) t.z = 0;
  st->T[0] = q.x; st->T[1] = q.y; st->T[2] = q.z; st->T[3] = q.w; st->T[4] = t.x; st->T[5] = t.y; st->T[6] = t.z;
  // angularDistance(R0, q): 2*atan2(|vec(R0 * conj(q))|, |w|)
  Quat<float> d = R0 * conj(q);
  float ang = 2.f * atan2f(norm(d.vec()), fabsf(d.w));
  float delta_r = float(double(ang) * 180.0 / M_PI);
  // std::pow(float, int) promotes to double in the reference (Estimator.cc:1352)
  double dt0 = double(X[3] * 100), dt1 = double(X[4] * 100), dt2 = double(X[5] * 100);
  float delta_t = float(sqrt(dt0 * dt0 + dt1 * dt1 + dt2 * dt2));
  st->iters = iter + 1;
  if (double(delta_r) < 0.05 && double(delta_t) < 0.05) st->converged = 1;
}


// ------------------------------------------------------------------------------------------------
// One round of the newest frame's Gauss-Newton loop (Estimator::CalculateLaserOdom, Estimator.cc:1242-1359) in TWO launches
// instead of three: the search / plane-fit kernel also forms the rows of (mat_A | mat_B) of the features it has just fitted
// (and, with keep_features, of the ones it kept from the earlier rounds of the same point, Estimator.cc:978-980) and leaves
// one 28-double partial per block; the update kernel folds them (fixed order), solves the 6x6 system and tests convergence.
//
// The kernel is bound by vector-instruction issue, not by memory (A/B on the MI355X: 4 / 8 lanes per query, 4 / 8 candidate
// loads in flight and a merged first round trip all leave it at 34 us; 16 lanes per query make it slower).  With LPQ lanes per
// query the fit + row half used to run on 1 lane in LPQ while costing the whole wave's issue slots, and it is as long as the
// search half.  So the block works in two phases: all ODOM_ROUND_THREADS lanes search (LPQ per query) and park the five
// neighbours of each of the block's ODOM_ROUND_THREADS / LPQ queries in LDS; then ONE wave fits and forms rows with one query
// per lane (every lane busy) while the other waves retire.  Rows are summed in ascending query order: one partial per block.
#define ODOM_ROUND_THREADS 256
// one block's share of a round at the transform (q, t): phase 1 on all lanes, phase 2 on wave 0, which leaves the block's 28 sums
// in `out28` (lanes 0..27 of wave 0 return them; the other waves return 0 and must not use the value)
template <int LPQ, int THREADS = ODOM_ROUND_THREADS>
__device__ __forceinline__ double odom_round_block(const FeatScalars fs, FeatFrame fr, const Quat<float> q, const Vec3<float> t, const float4 *__restrict__ map,
                                                   const int *__restrict__ cells, const GridDesc &g, uint8_t *__restrict__ valid, float4 *__restrict__ coef,
                                                   float *__restrict__ score, int base_slot, int round, int keep, int block) {
  constexpr int QPB = THREADS / LPQ;   // queries per block
  static_assert(QPB <= 64, "the fit phase is one wave");
  __shared__ int s_bj[QPB][5];
  __shared__ float s_bd4[QPB];
  __shared__ int s_bi4[QPB];
  const int M = fr.M;
  fr.slot_off = base_slot + (keep ? round * M : 0);
  {   // ---- phase 1: search, LPQ lanes per query
    const int ql = threadIdx.x / LPQ, sub = threadIdx.x % LPQ;
    const int i = block * QPB + ql;
    const bool active = i < M;
    const float4 po = active ? fr.stack[i] : make_float4(0, 0, 0, 0);
    const Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
    const Vec3<float> sel(r.x + t.x, r.y + t.y, r.z + t.z);
    float bd[5]; int bi[5], bj[5];
    knn_scan_group<5, LPQ>(sel, active, sub, map, cells, g, bd, bi, bj);
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 5; ++k) s_bj[ql][k] = bj[k];
      s_bd4[ql] = bd[4]; s_bi4[ql] = bi[4];
    }
  }
  __syncthreads();
  double v = 0;
  if (threadIdx.x < 64) {
    // ---- phase 2 (wave 0): fit + rows, one query per lane
    const int ql = threadIdx.x;
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0;
    const int i = block * QPB + ql;
    if (ql < QPB && i < M) {
      const float4 po = fr.stack[i];
      const Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
      const Vec3<float> sel(r.x + t.x, r.y + t.y, r.z + t.z);
      int bj[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) bj[k] = s_bj[ql][k];
      const FeatResult res = features_fit<false>(fs, fr.slot_off + i, q, t, po, sel, s_bd4[ql], s_bi4[ql], bj, map);
      valid[res.slot] = res.ok; coef[res.slot] = res.c;
      if (score) score[res.slot] = res.sc;
      const Mat3<float> Rm = toRot(q), Rinv = Rm;   // Rinv unused for b_from_coef = 0
      if (keep)
        for (int rr = 0; rr < round; ++rr) {   // the factor lists of the earlier rounds stay in the problem: ascending slot order
          const int sl = base_slot + rr * M + i;
          if (valid[sl]) odom_row_accumulate(res.po, coef[sl], q, t, Rm, Rinv, 0, acc);
        }
      if (res.ok) odom_row_accumulate(res.po, res.c, q, t, Rm, Rinv, 0, acc);
    }
    // the block's 28 sums: an xor butterfly over the wave's 64 lanes (lanes without a query hold zeros) — a fixed tree, so the
    // sums do not depend on how many lanes worked on a query, and no LDS (the first form parked 64 x 28 doubles there, which
    // capped the one-lane-per-query launch at ten waves per CU)
#pragma unroll
    for (int k = 0; k < 28; ++k) {
      double sres = acc[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sres += __shfl_xor(sres, o, 64);
      if (int(threadIdx.x) == k) v = sres;
    }
  }
  return v;
}


// fold of `nblocks` 28-double partials by a 1024-thread block (32 groups of rows b = g mod 32, ascending, then the group sums
// ascending) into ssum[0..27]; ends with a barrier.  Also called by the test hook lio_gn_fold.
__device__ __forceinline__ void fold_partials28_wide(const double *__restrict__ partials, int nblocks, double *ssum /* shared, >= 28 */) {
  __shared__ double part[32][32];
  const int c = threadIdx.x & 31, gq = threadIdx.x >> 5;
  double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
  if (c < 28) {
    // The sums are those of the four-at-a-time walk (rows b, b + 32, b + 64, b + 96 into v0 .. v3, the tail into v0, ascending b) — the
    // order the resident form of the loop folds in too — but the LOADS go out eight, then four, then up to three at a time: the
    // fold is a chain of memory round trips (19 rows per lane at 606 blocks: 7 trips before, 3 now), not of additions.
    int b = gq;
    for (; b + 224 < nblocks; b += 256) {
      double x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = partials[size_t(b + 32 * k) * 28 + c];
      v0 += x[0]; v1 += x[1]; v2 += x[2]; v3 += x[3];
      v0 += x[4]; v1 += x[5]; v2 += x[6]; v3 += x[7];
    }
    for (; b + 96 < nblocks; b += 128) {
      const double x0 = partials[size_t(b) * 28 + c], x1 = partials[size_t(b + 32) * 28 + c], x2 = partials[size_t(b + 64) * 28 + c],
                   x3 = partials[size_t(b + 96) * 28 + c];
      v0 += x0; v1 += x1; v2 += x2; v3 += x3;
    }
    {   // at most three rows are left
      const bool h0 = b < nblocks, h1 = b + 32 < nblocks, h2 = b + 64 < nblocks;
      const double x0 = h0 ? partials[size_t(b) * 28 + c] : 0.0, x1 = h1 ? partials[size_t(b + 32) * 28 + c] : 0.0,
                   x2 = h2 ? partials[size_t(b + 64) * 28 + c] : 0.0;
      if (h0) v0 += x0;
      if (h1) v0 += x1;
      if (h2) v0 += x2;
    }
  }
  part[gq][c] = (v0 + v1) + (v2 + v3);
  __syncthreads();
  if (threadIdx.x < 28) {
    double s2 = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) s2 += part[k][threadIdx.x];
    ssum[threadIdx.x] = s2;
  }
  __syncthreads();
}

// fold_partials28_wide followed by the update of odom_update_from_sums
// mail: a copy of the state in coherent pinned host memory, posted with the round's sequence number after every round (also
// by the no-op rounds behind convergence), so the host's look at the convergence flag is a read of its own memory.
__device__ __forceinline__ void odom_update_wide_block(const double *__restrict__ partials, int nblocks, OdomState *st, int iter, int min_rows,
                                                      int left_update, OdomState *mail, const HostSignal &sig) {
  if (st->converged) {
    if (sig.flag && threadIdx.x < 64) post_host_mail(sig, mail, st, int(sizeof(OdomState) / 4), threadIdx.x);
    return;
  }
  __shared__ double ssum[28];
  fold_partials28_wide(partials, nblocks, ssum);
  odom_update_from_sums(ssum, st, iter, min_rows, left_update);
  if (sig.flag) {
    __syncthreads();   // thread 0's update of *st is visible to wave 0
    if (threadIdx.x < 64) post_host_mail(sig, mail, st, int(sizeof(OdomState) / 4), threadIdx.x);
  }
}

}  // namespace lio
#endif
