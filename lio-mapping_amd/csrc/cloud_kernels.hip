// cloud_kernels.hip — gfx950 kernels for the point-cloud stages (see cloud_kernels.h for the reference
// call sites).  fp32 arithmetic mirrors the CPU operation order (no FMA contraction: -ffp-contract=off)
// so neighbour sets, validity flags and coefficients are reproducible bit for bit.
//
// Layout: clouds are float4 AoS (x,y,z,intensity) — 16 B per lane per load, the coalescing sweet spot
// (cdna_hip_programming.md §2); the K-NN grid stores points cell-sorted so a 3-cell x-run is one
// contiguous stream per lane, served out of L2 (maps are a few MB).
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <cfloat>
#include <climits>

#include "cloud_kernels.h"
#include "cloud_device.h"

namespace lio {

// ------------------------------------------------------------------------------------------------
// rigid transform + concat
// ------------------------------------------------------------------------------------------------
__global__ void k_transform_concat(ConcatArgs a, float4 *__restrict__ dst) {
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.total) return;
  dst[gid] = concat_point(a.seg, a.nseg, gid, nullptr);   // (the sources are kernel arguments: nothing to tie them to)
}

void launch_transform_concat(const ConcatArgs &a, float4 *dst, hipStream_t s) {
  if (a.total <= 0) return;
  hipLaunchKernelGGL(k_transform_concat, dim3(cdiv(a.total, 256)), dim3(256), 0, s, a, dst);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// deskew (TransformToEnd)
// ------------------------------------------------------------------------------------------------
// One point per lane: one 16-byte load, one 16-byte store, 256 lanes per workgroup, cdiv(n, 256) workgroups (an HDL-64E sweep of 130 k
// points: 508, one launch).  KEEP: the intensity (ring + rel_time) is carried through (keep_intensity, :79); else the ring is stripped.
template <bool KEEP>
__global__ void __launch_bounds__(256) k_deskew_to_end(float4 *pts, int n, Quat<float> qe, Vec3<float> te, float time_factor) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pts[i] = deskew_to_end_point<KEEP>(pts[i], qe, te, time_factor);
}
void launch_deskew_to_end(float4 *pts, int n, const float q[4], const float p[3], float time_factor, hipStream_t s, bool keep_intensity) {
  if (n <= 0) return;
  const Quat<float> qe(q[3], q[0], q[1], q[2]);
  const Vec3<float> te(p[0], p[1], p[2]);
  if (keep_intensity) hipLaunchKernelGGL(k_deskew_to_end<true>, dim3(cdiv(n, 256)), dim3(256), 0, s, pts, n, qe, te, time_factor);
  else hipLaunchKernelGGL(k_deskew_to_end<false>, dim3(cdiv(n, 256)), dim3(256), 0, s, pts, n, qe, te, time_factor);
  LIO_HIP(hipGetLastError());
}

// out[i] = rot * in[i] + pos, intensity kept (PointAssociateToMap, PointMapping.cc:303-314); out of place, in != out
__global__ void __launch_bounds__(256) k_rigid_map(const float4 *__restrict__ in, int n, Quat<float> q, Vec3<float> t, float4 *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = rigid_map_point(in[i], q, t);
}
void launch_rigid_map(const float4 *in, int n, const float q[4], const float p[3], float4 *out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_rigid_map, dim3(cdiv(n, 256)), dim3(256), 0, s, in, n, Quat<float>(q[3], q[0], q[1], q[2]), Vec3<float>(p[0], p[1], p[2]), out);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// voxel grid
// ------------------------------------------------------------------------------------------------
// The bounds pass (cloud_kernels.h).  grid (max nb, clouds): cloud blockIdx.y by its first nb blocks ...
__global__ void __launch_bounds__(VOX_TILE) k_seg_bounds(const BoundsSeg *__restrict__ recs, float *__restrict__ partial) {
  const BoundsSeg r = recs[blockIdx.y];
  if (int(blockIdx.x) >= r.nb) return;
  cloud_bounds_block(r.pts, r.n, blockIdx.x, r.nb, partial + (size_t(r.off) + blockIdx.x) * 8);
}
// ... and one block per cloud
__global__ void __launch_bounds__(VOX_TILE) k_seg_bounds_fold(const BoundsSeg *__restrict__ recs, const float *__restrict__ partial, float inv_leaf,
                                                              VoxParams *__restrict__ out) {
  const BoundsSeg r = recs[blockIdx.x];
  VoxParams v;
  if (vox_fold_bounds(partial + size_t(r.off) * 8, r.nb, inv_leaf, v)) out[blockIdx.x] = v;
}
void launch_seg_bounds(const BoundsSeg *d_segs, int nseg, int max_nb, float *partial, float inv_leaf, VoxParams *d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_seg_bounds, dim3(max_nb, nseg), dim3(VOX_TILE), 0, s, d_segs, partial);
  hipLaunchKernelGGL(k_seg_bounds_fold, dim3(nseg), dim3(VOX_TILE), 0, s, d_segs, partial, inv_leaf, d_out);
  LIO_HIP(hipGetLastError());
}
// The same pass over one cloud that the launch itself names (the filter's exact path: no record to upload): gridDim.x blocks, then one
__global__ void __launch_bounds__(VOX_TILE) k_cloud_bounds(const float4 *__restrict__ pts, int n, float *__restrict__ partial) {
  cloud_bounds_block(pts, n, blockIdx.x, gridDim.x, partial + size_t(blockIdx.x) * 8);
}
__global__ void __launch_bounds__(VOX_TILE) k_cloud_bounds_fold(const float *__restrict__ partial, int nb, float inv_leaf, VoxParams *out) {
  VoxParams v;
  if (vox_fold_bounds(partial, nb, inv_leaf, v)) *out = v;
}

__global__ void k_vox_keys(const float4 *__restrict__ pts, int n, float inv_leaf, const VoxParams *__restrict__ vp,
                           uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 p = pts[i];
  uint32_t key = VOX_KEY_NONE;
  if (finite3(p)) {
    int i0 = int(floorf(p.x * inv_leaf) - float(vp->minb[0]));
    int i1 = int(floorf(p.y * inv_leaf) - float(vp->minb[1]));
    int i2 = int(floorf(p.z * inv_leaf) - float(vp->minb[2]));
    key = uint32_t(i0 + i1 * vp->divb[0] + i2 * vp->divb[0] * vp->divb[1]);
  }
  keys[i] = key;
  vals[i] = uint32_t(i);
}

// The fast path needs no bounds before the keys.  PCL's voxel index i0 + i1 * div0 + i2 * div0 * div1 (cells relative to the
// cloud's minimum) orders the voxels lexicographically by (cell_z, cell_y, cell_x), and so does any key that packs the ABSOLUTE
// cells floor(p * inverse_leaf) with a fixed offset per axis: 10 bits for z, 11 for y and x (+-204 m x +-409 m x +-409 m at a
// 0.4 m leaf).  A cloud that leaves that range raises `range_overflow` and the filter reruns with PCL's own index (exact path
// below).  The same pass leaves the per-block bounds the later kernels and the host need (VoxParams); they are folded by the
// extra block of k_vox_tile_heads, after the sort, so nothing waits for them.
__global__ void __launch_bounds__(VOX_TILE) k_vox_keys_abs(const float4 *__restrict__ pts, int n, float inv_leaf, uint32_t *__restrict__ keys,
                                                          uint32_t *__restrict__ vals, float *__restrict__ partial, int *__restrict__ range_overflow) {
  const int i = blockIdx.x * VOX_TILE + threadIdx.x;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float cnt = 0;
  if (i < n) {
    keys[i] = vox_take_point<10, VOX_KEY_NONE>(pts[i], inv_leaf, mn, mx, cnt, range_overflow);
    vals[i] = uint32_t(i);
  }
  vox_block_partial(mn, mx, cnt, partial + size_t(blockIdx.x) * 8);
}

// ---- the sort between the keys and the tile heads (cloud_kernels.h: sizing rule; docs/voxel_sort.md).  The values are the points' own
// indices, so the stable sort by key IS the sort by the 64-bit pair (key, index): any correct sort of the pairs gives the library's
// keys2_ / vals2_ bit for bit, whatever order the atomics of the scatter hand out.  No kernel waits for another workgroup.
// 1: splitters from a sample of this call's keys; the fill counters and the overflow word go back to zero here (no fill command per run)
__global__ void __launch_bounds__(VSORT_THREADS) k_vsort_splitters(const uint32_t *__restrict__ keys, int n, int NB, uint32_t *__restrict__ splitters,
                                                                  int *__restrict__ fill, int *__restrict__ overflow) {
  __shared__ __attribute__((aligned(16))) uint32_t ss[VSORT_OVERSAMPLE * VSORT_MAX_BUCKETS];
  if (blockIdx.x == 0) {
    for (int b = threadIdx.x; b < NB; b += VSORT_THREADS) fill[b] = 0;
    if (threadIdx.x == 0) *overflow = 0;
  }
  vsort_pick_splitters<VSORT_OVERSAMPLE>(keys, n, NB, ss, splitters);
}

// 2: every point into its bucket's region of VSORT_CAP pairs; one global atomic per (workgroup, non-empty bucket) reserves the room
__global__ void __launch_bounds__(VSORT_SCATTER_THREADS) k_vsort_scatter(const uint32_t *__restrict__ keys, int n, int NB,
                                                                        const uint32_t *__restrict__ splitters, int *__restrict__ fill,
                                                                        unsigned long long *__restrict__ pairs, int *__restrict__ overflow) {
  __shared__ uint32_t sspl[VSORT_MAX_BUCKETS];
  __shared__ int scnt[VSORT_MAX_BUCKETS], sbase[VSORT_MAX_BUCKETS];
  const int tid = threadIdx.x;
  for (int b = tid; b < NB; b += VSORT_SCATTER_THREADS) { scnt[b] = 0; if (b < NB - 1) sspl[b] = splitters[b]; }
  __syncthreads();
  uint32_t key[VSORT_SCATTER_ITEMS];
  int bucket[VSORT_SCATTER_ITEMS], rank[VSORT_SCATTER_ITEMS];
#pragma unroll
  for (int r = 0; r < VSORT_SCATTER_ITEMS; ++r) {
    const int i = (blockIdx.x * VSORT_SCATTER_ITEMS + r) * VSORT_SCATTER_THREADS + tid;
    bucket[r] = -1;
    if (i < n) {
      key[r] = keys[i];
      bucket[r] = vsort_bucket_of(sspl, NB, key[r]);
      rank[r] = atomicAdd(&scnt[bucket[r]], 1);
    }
  }
  __syncthreads();
  for (int b = tid; b < NB; b += VSORT_SCATTER_THREADS) {
    const int c = scnt[b];
    if (c > 0) sbase[b] = atomicAdd(&fill[b], c);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < VSORT_SCATTER_ITEMS; ++r) {
    if (bucket[r] < 0) continue;
    const int i = (blockIdx.x * VSORT_SCATTER_ITEMS + r) * VSORT_SCATTER_THREADS + tid;
    const int pos = sbase[bucket[r]] + rank[r];
    if (pos < VSORT_CAP) pairs[size_t(bucket[r]) * VSORT_CAP + pos] = (static_cast<unsigned long long>(key[r]) << 32) | uint32_t(i);
    else *overflow = 1;   // nothing is written beyond the capacity; finish() redoes the filter with the library sort
  }
}

// 3: workgroup b sorts bucket b (registers; LDS for the strides that cross waves) and writes it behind the buckets before it
__global__ void __launch_bounds__(VSORT_THREADS) k_vsort_buckets(const unsigned long long *__restrict__ pairs, const int *__restrict__ fill, int NB, int n,
                                                                const int *__restrict__ overflow, uint32_t *__restrict__ keys_out,
                                                                uint32_t *__restrict__ vals_out) {
  __shared__ unsigned long long sp[VSORT_CAP];
  __shared__ int swave[VSORT_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (*overflow) {
    // the run is going to be redone: leave "no point" everywhere, so that the kernels behind gather through no stale index
    const int chunk = (n + NB - 1) / NB;
    for (int i = b * chunk + tid; i < min(n, (b + 1) * chunk); i += VSORT_THREADS) keys_out[i] = VOX_KEY_NONE;
    return;
  }
  int before = 0;
  for (int j = tid; j < b; j += VSORT_THREADS) before += min(fill[j], VSORT_CAP);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  if ((tid & 63) == 0) swave[tid >> 6] = before;
  const int m = min(fill[b], VSORT_CAP);
  __syncthreads();
  int off = 0;
#pragma unroll
  for (int w = 0; w < VSORT_THREADS / 64; ++w) off += swave[w];
  const unsigned long long *src = pairs + size_t(b) * VSORT_CAP;
  switch (vsort_items_for(m)) {   // uniform over the block
    case 1: vsort_pairs_sort_store<1>(src, m, sp, keys_out, vals_out, off); break;
    case 2: vsort_pairs_sort_store<2>(src, m, sp, keys_out, vals_out, off); break;
    case 4: vsort_pairs_sort_store<4>(src, m, sp, keys_out, vals_out, off); break;
    case 8: vsort_pairs_sort_store<8>(src, m, sp, keys_out, vals_out, off); break;
    default: vsort_pairs_sort_store<16>(src, m, sp, keys_out, vals_out, off); break;
  }
}

// n <= VSORT_CAP: the keys are sorted directly, in one launch, by rank: every workgroup holds all keys in LDS and counts, for
// VSORT_THREADS / VSORT_RANK_LANES of them, the pairs (key, index) below; that count is the pair's place.  (One workgroup sorting 2048 pairs
// by the bitonic network of k_vsort_buckets took 20 us, then 11: 66 steps on one compute unit.)
__global__ void __launch_bounds__(VSORT_THREADS) k_vsort_single(const uint32_t *__restrict__ keys, int n, int *__restrict__ overflow,
                                                               uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out) {
  __shared__ __attribute__((aligned(16))) uint32_t ss[VSORT_CAP];
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;
  const int S = (n + 3) & ~3;   // fillers behind the keys: equal to "no point", but with indices behind every key's
  for (int t = threadIdx.x; t < S; t += VSORT_THREADS) ss[t] = t < n ? keys[t] : VOX_KEY_NONE;
  __syncthreads();
  const int i = blockIdx.x * (VSORT_THREADS / VSORT_RANK_LANES) + int(threadIdx.x) / VSORT_RANK_LANES, part = int(threadIdx.x) % VSORT_RANK_LANES;
  const unsigned long long mine = i < n ? (static_cast<unsigned long long>(ss[i]) << 32) | uint32_t(i) : 0ull;
  const int rank = vsort_rank_of(ss, S, part, mine);
  if (part == 0 && i < n) { keys_out[rank] = uint32_t(mine >> 32); vals_out[rank] = uint32_t(i); }
}

// heads (first entry of a run of equal keys) in each VOX_TILE-entry tile of the sorted keys
__global__ void __launch_bounds__(VOX_TILE) k_vox_tile_heads(const uint32_t *__restrict__ keys, int n, int *__restrict__ tile_heads,
                                                             const float *__restrict__ partial, int npartial, float inv_leaf, VoxParams *__restrict__ params) {
  if (blockIdx.x == gridDim.x - 1) {
    // the extra block (fast path only: npartial > 0): bounds of the cloud from k_vox_keys_abs's per-block partials -> VoxParams
    if (npartial <= 0) return;
    VoxParams v;
    if (vox_fold_bounds(partial, npartial, inv_leaf, v)) *params = v;
    return;
  }
  vox_tile_head_count(keys, n, blockIdx.x, tile_heads + blockIdx.x);
}

// Centroids of the sorted runs (cloud_device.h: vox_centroid_tile).  The last tile's block knows the total and posts it (with the
// bounds) to the host's mailbox.
struct VoxMail { int count; VoxParams params; int range_overflow; int sort_overflow; };
__global__ void __launch_bounds__(VOX_TILE) k_vox_centroids(const float4 *__restrict__ pts, const uint32_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ vals, const int *__restrict__ tile_heads, int n,
                                                            float4 *__restrict__ out, int *__restrict__ count, const VoxParams *__restrict__ params,
                                                            int *__restrict__ range_overflow, const int *__restrict__ sort_overflow, VoxMail *mail,
                                                            HostSignal sig) {
  const VoxSlot r = vox_centroid_tile(pts, keys, vals, tile_heads, n, blockIdx.x, out);
  if (blockIdx.x == gridDim.x - 1) {   // the last tile knows the total
    __shared__ VoxMail smail;
    const int tid = threadIdx.x;
    if (tid == VOX_TILE - 1) {
      const int total = r.pos + (r.head ? 1 : 0);
      *count = total;
      smail.count = total; smail.params = *params; smail.range_overflow = *range_overflow; smail.sort_overflow = *sort_overflow;
      if (sig.flag) *range_overflow = 0;   // the mail carries it: leave the flag clear for the next run (no fill command in front of it)
    }
    if (sig.flag) {
      __syncthreads();
      if (tid < 64) post_host_mail(sig, mail, &smail, int(sizeof(VoxMail) / 4), tid);
    }
  }
}

// launch() enqueues the whole filter on `s` (no host sync); finish() waits for it and returns the output count.  Two
// filters launched on two streams overlap (the scan-to-map step filters its corner and surf stacks that way).
void VoxelGridDev::launch(const float4 *in, size_t n, float leaf, DBuf<float4> &out, hipStream_t s) {
  p_in_ = in; p_n_ = n; p_out_ = &out; p_stream_ = s; p_leaf_ = leaf;
  if (n == 0) return;
  enqueue(false, false);
}

// exact == false: absolute-cell keys, bounds folded on the side (4 stages: keys, sort, tile heads, centroids);
// exact == true: PCL's own index from the bounds (two more launches in front), used when the cloud leaves the key's range.
// library == true: the sort is the library's (a bucket of the sample sort overflowed).
void VoxelGridDev::enqueue(bool exact, bool library) {
  const float4 *in = p_in_;
  const size_t n = p_n_;
  DBuf<float4> &out = *p_out_;
  hipStream_t s = p_stream_;
  const int ni = int(n);
  const float inv_leaf = 1.0f / p_leaf_;
  const int nkb = cdiv(ni, VOX_TILE);
  partial_.reserve(size_t(std::max(nkb, 512)) * 8);
  params_.reserve(1);
  reserve_sort(n, s);
  out.reserve(n);
  if (!h_count_) {
    // coherent pinned memory: k_vox_centroids posts the count, the bounds and the range flag here (VoxMail), then the completion word
    h_mail_.alloc(256, hipHostMallocCoherent, true);
    static_assert(sizeof(VoxMail) <= 128, "mailbox layout");
    h_count_ = reinterpret_cast<int *>(h_mail_.p);
    h_params_ = reinterpret_cast<VoxParams *>(h_count_ + 1);
    h_flag_ = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(h_count_) + 128);
  }
  int *d_range = count_.p + 1;   // zero between runs: with the mailbox k_vox_centroids clears it after reading it (one fill command less)
  if (!use_signal_) LIO_HIP(hipMemsetAsync(d_range, 0, sizeof(int), s));   // copy-back path: the host reads the flag behind the kernels, so they cannot clear it
  int npartial = 0;
  if (exact) {
    const int nb = cloud_bounds_blocks(ni);
    hipLaunchKernelGGL(k_cloud_bounds, dim3(nb), dim3(VOX_TILE), 0, s, in, ni, partial_.p);
    hipLaunchKernelGGL(k_cloud_bounds_fold, dim3(1), dim3(VOX_TILE), 0, s, partial_.p, nb, inv_leaf, params_.p);
    hipLaunchKernelGGL(k_vox_keys, dim3(cdiv(ni, 256)), dim3(256), 0, s, in, ni, inv_leaf, params_.p, keys_.p, vals_.p);
  } else {
    hipLaunchKernelGGL(k_vox_keys_abs, dim3(nkb), dim3(VOX_TILE), 0, s, in, ni, inv_leaf, keys_.p, vals_.p, partial_.p, d_range);
    npartial = nkb;
  }
  last_path_ = enqueue_sort(n, s, library);
  const int ntiles = cdiv(ni, VOX_TILE);
  tile_heads_.reserve(ntiles);
  hipLaunchKernelGGL(k_vox_tile_heads, dim3(ntiles + 1), dim3(VOX_TILE), 0, s, keys2_.p, ni, tile_heads_.p, partial_.p, npartial, inv_leaf, params_.p);
  sig_ = HostSignal();
  if (use_signal_) { sig_.flag = h_flag_; sig_.seq = ++seq_; }

  hipLaunchKernelGGL(k_vox_centroids, dim3(ntiles), dim3(VOX_TILE), 0, s, in, keys2_.p, vals2_.p, tile_heads_.p, ni, out.p, count_.p, params_.p, d_range,
                     count_.p + 2, reinterpret_cast<VoxMail *>(h_count_), sig_);
  LIO_HIP(hipGetLastError());
  if (!sig_.flag) {
    VoxMail *m = reinterpret_cast<VoxMail *>(h_count_);
    LIO_HIP(hipMemcpyAsync(&m->count, count_.p, sizeof(int), hipMemcpyDeviceToHost, s));
    LIO_HIP(hipMemcpyAsync(&m->params, params_.p, sizeof(VoxParams), hipMemcpyDeviceToHost, s));
    LIO_HIP(hipMemcpyAsync(&m->range_overflow, d_range, sizeof(int), hipMemcpyDeviceToHost, s));
    LIO_HIP(hipMemcpyAsync(&m->sort_overflow, count_.p + 2, sizeof(int), hipMemcpyDeviceToHost, s));
  }
}

// count_: [0] the output count, [1] the range flag, [2] the sort's overflow word (put back to zero by whichever sort runs)
void VoxelGridDev::reserve_sort(size_t n, hipStream_t s) {
  keys_.reserve(n); keys2_.reserve(n); vals_.reserve(n); vals2_.reserve(n);
  if (count_.cap < 3) { count_.reserve(3); LIO_HIP(hipMemsetAsync(count_.p, 0, count_.cap * sizeof(int), s)); }
}

int VoxelGridDev::enqueue_sort(size_t n, hipStream_t s, bool library) {
  const int ni = int(n);
  int *d_overflow = count_.p + 2;
  if (library || n > size_t(VSORT_MAX_N)) {
    LIO_HIP(hipMemsetAsync(d_overflow, 0, sizeof(int), s));
    size_t tmp_bytes = 0;
    LIO_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_.p, keys2_.p, vals_.p, vals2_.p, n, 0, 32, s));
    tmp_.reserve(tmp_bytes + 256);
    LIO_HIP(rocprim::radix_sort_pairs(tmp_.p, tmp_bytes, keys_.p, keys2_.p, vals_.p, vals2_.p, n, 0, 32, s));
    return VSORT_PATH_LIBRARY;
  }
  if (ni <= VSORT_CAP) {
    hipLaunchKernelGGL(k_vsort_single, dim3(cdiv(ni, VSORT_THREADS / VSORT_RANK_LANES)), dim3(VSORT_THREADS), 0, s, keys_.p, ni, d_overflow, keys2_.p, vals2_.p);
    return VSORT_PATH_SINGLE;
  }
  const int NB = vsort_buckets(n);
  splitters_.reserve(NB); fill_.reserve(NB); pairs_.reserve(size_t(NB) * VSORT_CAP);
  hipLaunchKernelGGL(k_vsort_splitters, dim3(cdiv(VSORT_OVERSAMPLE * NB, VSORT_THREADS / VSORT_RANK_LANES)), dim3(VSORT_THREADS), 0, s, keys_.p, ni, NB,
                     splitters_.p, fill_.p, d_overflow);
  hipLaunchKernelGGL(k_vsort_scatter, dim3(cdiv(ni, VSORT_SCATTER_THREADS * VSORT_SCATTER_ITEMS)), dim3(VSORT_SCATTER_THREADS), 0, s, keys_.p, ni, NB,
                     splitters_.p, fill_.p, pairs_.p, d_overflow);
  hipLaunchKernelGGL(k_vsort_buckets, dim3(NB), dim3(VSORT_THREADS), 0, s, pairs_.p, fill_.p, NB, ni, d_overflow, keys2_.p, vals2_.p);
  return VSORT_PATH_SAMPLE;
}

int VoxelGridDev::sort_pairs_hook(const uint32_t *keys, size_t n, uint32_t *keys_out, uint32_t *vals_out, hipStream_t s) {
  reserve_sort(n, s);
  std::vector<uint32_t> iota(n);
  for (size_t i = 0; i < n; ++i) iota[i] = uint32_t(i);
  LIO_HIP(hipMemcpyAsync(keys_.p, keys, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  LIO_HIP(hipMemcpyAsync(vals_.p, iota.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  int path = enqueue_sort(n, s, false);
  LIO_HIP(hipGetLastError());
  int overflow = 0;
  LIO_HIP(hipMemcpyAsync(&overflow, count_.p + 2, sizeof(int), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
  if (overflow) path = enqueue_sort(n, s, true);   // what finish() does on the mail's word
  LIO_HIP(hipMemcpyAsync(keys_out, keys2_.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipMemcpyAsync(vals_out, vals2_.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
  return path;
}

size_t VoxelGridDev::finish(VoxParams *host_params) {
  if (p_n_ == 0) {
    if (host_params) std::memset(host_params, 0, sizeof(*host_params));
    return 0;
  }
  const VoxMail *m = reinterpret_cast<const VoxMail *>(h_count_);
  bool redone = false, exact = false, library = false;
  for (;;) {
    if (sig_.flag) wait_host_signal(sig_, p_stream_);   // the count is out; the centroids follow in stream order
    else LIO_HIP(hipStreamSynchronize(p_stream_));
    if (m->range_overflow == 1 && !exact) {
      exact = true;   // the cloud spans more cells than the absolute key holds
      enqueue(exact, library);
      redone = true;
      continue;
    }
    if (m->sort_overflow == 1 && !library) {
      library = true;   // a bucket of the sample sort was full: its keys2_ / vals2_ are not the sort
      enqueue(exact, library);
      redone = true;
      continue;
    }
    // cold path: a second pass was enqueued AFTER launch() returned, i.e. after the caller may have recorded the event other
    // streams wait on — those consumers are not ordered behind it, so the output must be complete before finish() returns
    if (redone) LIO_HIP(hipStreamSynchronize(p_stream_));
    break;
  }
  ++n_path_[last_path_];
  int count = m->count;
  const VoxParams hp = m->params;
  if (hp.overflow) {  // PCL: "Leaf size is too small for the input dataset" -> output = input
    p_out_->reserve(p_n_);  // the caller may have swapped the buffer since launch()
    LIO_HIP(hipMemcpyAsync(p_out_->p, p_in_, p_n_ * sizeof(float4), hipMemcpyDeviceToDevice, p_stream_));
    LIO_HIP(hipStreamSynchronize(p_stream_));  // cold path: consumers on OTHER streams read the output right after finish()
    count = int(p_n_);
  }
  if (host_params) *host_params = hp;
  return size_t(count);
}

size_t VoxelGridDev::run(const float4 *in, size_t n, float leaf, DBuf<float4> &out, hipStream_t s, VoxParams *host_params) {
  launch(in, n, leaf, out, s);
  return finish(host_params);
}

// ------------------------------------------------------------------------------------------------
// K-NN grid
// ------------------------------------------------------------------------------------------------
// Counting sort by cell: a histogram with atomics hands every point a slot inside its cell, an exclusive scan over the
// dense cell table turns the counts into run starts, and a scatter places the points.  The order INSIDE a cell depends on
// the atomics and is not reproducible — by design: every consumer ranks candidates by the total order (distance, original
// index), so results are identical whatever that order is.  (A radix/merge sort of the keys cost ~45 us of dependent
// launches for 77 k points; this is three short kernels.)
__global__ void k_cell_count(const float4 *__restrict__ pts, int n, GridDesc g, uint32_t *__restrict__ keys, uint32_t *__restrict__ slot,
                             int *__restrict__ cnt) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cell_count_point(pts, i, g, keys, slot, cnt);
}

// cnt: the histogram of k_cell_count, already scanned into `starts`; every point puts its cell's count back to zero (plain
// stores of the same value), so the table is all zeros again when the build ends and the next build needs no fill command
__global__ void k_cell_place(const float4 *__restrict__ pts, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ slot, int n,
                             const int *__restrict__ starts, float4 *__restrict__ sorted, int *__restrict__ cnt) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cell_place_point(pts, keys, slot, i, starts, sorted, cnt);
}

void KnnGrid::build(const float4 *pts, size_t n, const float mn[3], const float mx[3], float cell, hipStream_t s) {
  desc_.n_points = int(n);
  const size_t ncells = grid_extent(desc_, mn, mx, cell);
  if (ncells > (size_t(1) << 30)) throw DeviceError("KnnGrid: cell table too large");
  cells_.reserve(ncells + 1);
  if (cnt_.cap < ncells + 1 || cnt_dirty_) {   // a fresh table starts zeroed; after that k_cell_place leaves it zeroed (no fill per build)
    cnt_.reserve(ncells + 1);
    LIO_HIP(hipMemsetAsync(cnt_.p, 0, cnt_.cap * sizeof(int), s));
  }
  cnt_dirty_ = true;   // until k_cell_place has been enqueued: a build that throws in between leaves counts behind, the next one clears them
  keys_.reserve(std::max<size_t>(n, 1)); vals_.reserve(std::max<size_t>(n, 1)); sorted_.reserve(std::max<size_t>(n, 1));
  const int ni = int(n);
  if (ni) hipLaunchKernelGGL(k_cell_count, dim3(cdiv(ni, 256)), dim3(256), 0, s, pts, ni, desc_, keys_.p, vals_.p, cnt_.p);
  size_t tmp_bytes = 0;
  LIO_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, cnt_.p, cells_.p, 0, ncells + 1, rocprim::plus<int>(), s));
  tmp_.reserve(tmp_bytes + 256);
  LIO_HIP(rocprim::exclusive_scan(tmp_.p, tmp_bytes, cnt_.p, cells_.p, 0, ncells + 1, rocprim::plus<int>(), s));
  if (ni) hipLaunchKernelGGL(k_cell_place, dim3(cdiv(ni, 256)), dim3(256), 0, s, pts, keys_.p, vals_.p, ni, cells_.p, sorted_.p, cnt_.p);
  LIO_HIP(hipGetLastError());
  cnt_dirty_ = false;
}

// ---- GridBatch (cloud_kernels.h).  grid (cdiv(max points, 256), grids): k_cell_count's body with the grid's own record
__global__ void __launch_bounds__(256) k_seg_cell_count(const GridSeg *__restrict__ segs, uint32_t *__restrict__ keys, uint32_t *__restrict__ slot,
                                                        int *__restrict__ cnt) {
  const GridSeg &r = segs[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (r.pt_off < 0 || i >= r.g.n_points) return;
  cell_count_point(r.pts, i, r.g, keys + r.pt_off, slot + r.pt_off, cnt + r.cell_off);
}
// one workgroup per grid walks the grid's own count table: no block waits for another.  The run starts begin at the grid's first sorted entry
__global__ void __launch_bounds__(SEG_SCAN_THREADS) k_seg_cell_scan(const GridSeg *__restrict__ segs, const int *__restrict__ cnt, int *__restrict__ cells) {
  const GridSeg &r = segs[blockIdx.x];
  if (r.pt_off < 0) return;
  block_exclusive_scan(cnt + r.cell_off, cells + r.cell_off, r.ncells + 1, r.pt_off);
}
__global__ void __launch_bounds__(256) k_seg_cell_place(const GridSeg *__restrict__ segs, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ slot,
                                                        const int *__restrict__ cells, float4 *__restrict__ sorted, int *__restrict__ cnt) {
  const GridSeg &r = segs[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (r.pt_off < 0 || i >= r.g.n_points) return;
  cell_place_point(r.pts, keys + r.pt_off, slot + r.pt_off, i, cells + r.cell_off, sorted, cnt + r.cell_off);
}

void *GridBatch::begin(size_t head_bytes, int clouds) {
  off_g_ = head_bytes; off_b_ = off_g_ + size_t(clouds) * sizeof(GridSeg);
  h_tab_.assign(off_b_ + size_t(clouds) * sizeof(BoundsSeg), 0);
  d_tab_.reserve(std::max<size_t>(h_tab_.size(), 1));
  n_ = max_nb_ = max_pts_ = 0; part_total_ = 0;
  any_shared_ = false;   // until layout(): a call without clouds builds nothing
  return h_tab_.data();
}
void GridBatch::add(const float4 *pts, int n) {
  const int nb = cloud_bounds_blocks(n);
  bseg()[n_++] = BoundsSeg{pts, n, nb, int(part_total_)};
  part_total_ += size_t(nb);
  max_nb_ = std::max(max_nb_, nb); max_pts_ = std::max(max_pts_, n);
}
const VoxParams *GridBatch::bounds(hipStream_t s, float inv_leaf) {
  partial_.reserve(part_total_ * 8); d_bounds_.reserve(size_t(n_));
  if (h_bounds_.n < size_t(n_)) h_bounds_.alloc(size_t(n_) + size_t(n_) / 2, hipHostMallocDefault);
  LIO_HIP(hipMemcpyAsync(d_tab_.p + off_b_, h_tab_.data() + off_b_, size_t(n_) * sizeof(BoundsSeg), hipMemcpyHostToDevice, s));
  launch_seg_bounds(reinterpret_cast<const BoundsSeg *>(d_tab_.p + off_b_), n_, max_nb_, partial_.p, inv_leaf, d_bounds_.p, s);
  LIO_HIP(hipMemcpyAsync(h_bounds_.p, d_bounds_.p, size_t(n_) * sizeof(VoxParams), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
  return h_bounds_.p;
}
void GridBatch::layout(float cell, size_t cells_cap) {
  size_t cell_total = 0, pt_off = 0;
  for (int i = 0; i < n_; ++i) {
    VoxParams &b = h_bounds_.p[i];
    if (b.n_valid == 0)   // a cloud without a finite point (the test hooks allow empty ones) has no bounds
      for (int e = 0; e < 3; ++e) b.mn[e] = b.mx[e] = 0.f;
    GridSeg &g = gseg(i);
    g.pts = bseg()[i].pts; g.g.n_points = bseg()[i].n; g.pt_off = -1;
    const size_t ncells = grid_extent(g.g, b.mn, b.mx, cell);
    if (ncells > cells_cap) continue;
    g.pt_off = int(pt_off); g.cell_off = int(cell_total); g.ncells = int(ncells);
    pt_off += size_t(g.g.n_points); cell_total += ncells + 1;
    if (pt_off > size_t(INT_MAX) || cell_total > size_t(INT_MAX)) throw CapacityError("GridBatch: the points or the cell tables exceed 2^31 entries");
    any_shared_ = true;
  }
  cells_.reserve(std::max<size_t>(cell_total, 1));
  if (cnt_.cap < std::max<size_t>(cell_total, 1)) { cnt_.reserve(std::max<size_t>(cell_total, 1)); cnt_dirty_ = true; }
  keys_.reserve(std::max<size_t>(pt_off, 1)); slot_.reserve(std::max<size_t>(pt_off, 1)); sorted_.reserve(std::max<size_t>(pt_off, 1));
}
void GridBatch::build(hipStream_t s) {
  if (any_shared_ && cnt_dirty_) LIO_HIP(hipMemsetAsync(cnt_.p, 0, cnt_.cap * sizeof(int), s));
  LIO_HIP(hipMemcpyAsync(d_tab_.p, h_tab_.data(), off_b_, hipMemcpyHostToDevice, s));
  if (!any_shared_) return;
  // no point at all (the hooks' empty clouds): nothing to count or place, and no launch of zero blocks; the scan still runs, so every cell's
  // run starts (and ends) at its grid's base
  const GridSeg *segs = reinterpret_cast<const GridSeg *>(d_tab_.p + off_g_);
  const int pb = cdiv(max_pts_, 256);
  cnt_dirty_ = true;   // until k_seg_cell_place has been enqueued
  if (pb) hipLaunchKernelGGL(k_seg_cell_count, dim3(pb, n_), dim3(256), 0, s, segs, keys_.p, slot_.p, cnt_.p);
  hipLaunchKernelGGL(k_seg_cell_scan, dim3(n_), dim3(SEG_SCAN_THREADS), 0, s, segs, cnt_.p, cells_.p);
  if (pb) hipLaunchKernelGGL(k_seg_cell_place, dim3(pb, n_), dim3(256), 0, s, segs, keys_.p, slot_.p, cells_.p, sorted_.p, cnt_.p);
  LIO_HIP(hipGetLastError());
  cnt_dirty_ = false;
}

// The walk of the product, knn_scan_group (cloud_device.h), on its own: LPQ lanes per query in a 256-thread block, like the feature and
// round kernels; sub-lane 0 writes the query's list.  lio_knn (K = 1 / 5, 8 lanes, entries at or beyond radius_sq cut) and the test hook
// lio_knn_walk (K = 5, 1 / 4 / 8 lanes, the whole list and the points at sorted[bj[k]], the ones the plane fit loads) both run it.
#define KNN_WALK_THREADS 256
template <int K, int LPQ>
__global__ void __launch_bounds__(KNN_WALK_THREADS) k_nn_walk(const float4 *__restrict__ query, int m, int cut, float radius_sq,
                                                              const float4 *__restrict__ map, const int *__restrict__ cells, GridDesc g,
                                                              int32_t *__restrict__ idx, float *__restrict__ sqd, float *__restrict__ nbr) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;   // m * LPQ < 2^31: checked by the callers
  const int i = gt / LPQ, sub = gt % LPQ;
  const bool active = i < m;
  const float4 q4 = active ? query[i] : make_float4(0, 0, 0, 0);
  float bd[K]; int bi[K], bj[K];
  knn_scan_group<K, LPQ>(Vec3<float>(q4.x, q4.y, q4.z), active, sub, map, cells, g, bd, bi, bj);
  if (!active || sub != 0) return;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const bool ok = bi[k] != INT_MAX && !(cut && !(bd[k] < radius_sq));
    const size_t o = size_t(i) * K + k;
    idx[o] = ok ? bi[k] : -1;
    sqd[o] = ok ? bd[k] : INFINITY;
    if (nbr) {
      const float4 p = ok ? map[bj[k]] : make_float4(0, 0, 0, 0);
      nbr[3 * o + 0] = p.x; nbr[3 * o + 1] = p.y; nbr[3 * o + 2] = p.z;
    }
  }
}

template <int K, int LPQ>
static void launch_knn_walk_as(const float4 *query, int m, int cut, float radius_sq, const float4 *map_sorted, const int *cells, const GridDesc &g,
                               int32_t *idx, float *sqd, float *nbr, hipStream_t s) {
  hipLaunchKernelGGL((k_nn_walk<K, LPQ>), dim3(cdiv((long long)m * LPQ, KNN_WALK_THREADS)), dim3(KNN_WALK_THREADS), 0, s, query, m, cut, radius_sq,
                     map_sorted, cells, g, idx, sqd, nbr);
}

void launch_knn(const float4 *query, int m, int k, float radius_sq, const float4 *map_sorted, const int *cells, const GridDesc &g,
                int32_t *idx, float *sqd, hipStream_t s) {
  if (m <= 0) return;
  if (k == 1) launch_knn_walk_as<1, 8>(query, m, 1, radius_sq, map_sorted, cells, g, idx, sqd, nullptr, s);
  else if (k == 5) launch_knn_walk_as<5, 8>(query, m, 1, radius_sq, map_sorted, cells, g, idx, sqd, nullptr, s);
  else throw DeviceError("launch_knn: k is 1 or 5");
  LIO_HIP(hipGetLastError());
}

void launch_knn_walk(const float4 *query, int m, int lanes_per_query, const float4 *map_sorted, const int *cells, const GridDesc &g,
                     int32_t *idx, float *sqd, float *nbr_xyz, hipStream_t s) {
  if (m <= 0) return;
  if (lanes_per_query == 1) launch_knn_walk_as<5, 1>(query, m, 0, 0.f, map_sorted, cells, g, idx, sqd, nbr_xyz, s);
  else if (lanes_per_query == 4) launch_knn_walk_as<5, 4>(query, m, 0, 0.f, map_sorted, cells, g, idx, sqd, nbr_xyz, s);
  else if (lanes_per_query == 8) launch_knn_walk_as<5, 8>(query, m, 0, 0.f, map_sorted, cells, g, idx, sqd, nbr_xyz, s);
  else throw DeviceError("launch_knn_walk: lanes per query is 1, 4 or 8");
  LIO_HIP(hipGetLastError());
}

// CalculateFeatures for every frame of the launch (blockIdx.y)
template <bool MAPPING, int LPQ>
__global__ void __launch_bounds__(FEAT_THREADS) k_features(FeatArgs a, const float *__restrict__ transforms, const float4 *__restrict__ map,
                                                          const int *__restrict__ cells, GridDesc g, uint8_t *__restrict__ valid,
                                                          float4 *__restrict__ coef, float *__restrict__ score, const int *__restrict__ skip_flag,
                                                          float4 *__restrict__ abs_coef) {
  if (skip_flag && *skip_flag) return;
  features_block<MAPPING, LPQ>(a.fr[blockIdx.y], feat_scalars(a), int(blockIdx.x), transforms, map, cells, g, valid, coef, score, abs_coef);
}

// The fit half of a corner feature (PointMapping.cc:399-517) for ONE query whose five nearest map points are known: covariance of
// the five, line direction = eigenvector of the largest eigenvalue (accepted when it dominates 3x the middle one), point-to-line
// coefficients, score, FOV.  t: the frame's translation; pz: the FOV apex point; sel: the query's image; bd4 / bi4: distance and
// original index of the fifth neighbour; bj: positions of the five in `map`.  Returns ok; c is zeros when not ok.
__device__ __forceinline__ uint8_t line_features_fit(const Vec3<float> &t, const Vec3<float> &pz, const Vec3<float> &sel, float min_match_sq_dis,
                                                     float bd4, int bi4, const int (&bj)[5], const float4 *__restrict__ map, float4 &c) {
  uint8_t ok = 0;
  c = make_float4(0, 0, 0, 0);
  if (bi4 != INT_MAX && bd4 < min_match_sq_dis) {
    float nx[5], ny[5], nz[5];
    Vec3<float> vc(0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float4 pn = map[bj[j]];
      nx[j] = pn.x; ny[j] = pn.y; nz[j] = pn.z;
      vc.x += pn.x; vc.y += pn.y; vc.z += pn.z;
    }
    vc.x /= 5.0f; vc.y /= 5.0f; vc.z /= 5.0f;
    float a00 = 0, a10 = 0, a20 = 0, a11 = 0, a21 = 0, a22 = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float ax = nx[j] - vc.x, ay = ny[j] - vc.y, az = nz[j] - vc.z;
      a00 += ax * ax; a10 += ax * ay; a20 += ax * az; a11 += ay * ay; a21 += ay * az; a22 += az * az;
    }
    a00 /= 5.0f; a10 /= 5.0f; a20 /= 5.0f; a11 /= 5.0f; a21 /= 5.0f; a22 /= 5.0f;
    const float A1[9] = {a00, a10, a20, a10, a11, a21, a20, a21, a22};
    float D1[3]; double v[3];
    sym_eig3_top_closed(A1, D1, v);
    if (D1[2] > 3 * D1[1]) {
      const float x0 = sel.x, y0 = sel.y, z0 = sel.z;
      const float v0 = float(v[0]), v1 = float(v[1]), v2 = float(v[2]);  // mat_V1 is a float matrix
      const float x1 = float(double(vc.x) + 0.1 * double(v0)), y1 = float(double(vc.y) + 0.1 * double(v1)), z1 = float(double(vc.z) + 0.1 * double(v2));
      const float x2 = float(double(vc.x) - 0.1 * double(v0)), y2 = float(double(vc.y) - 0.1 * double(v1)), z2 = float(double(vc.z) - 0.1 * double(v2));
      Vec3<float> X0(x0, y0, z0), X1(x1, y1, z1), X2(x2, y2, z2);
      Vec3<float> a012v = cross(X0 - X1, X0 - X2);
      Vec3<float> nt = cross(X1 - X2, a012v);
      const float n2 = dot(nt, nt);
      if (n2 > 0.f) nt = nt / sqrtf(n2);
      const float a012 = norm(a012v), l12 = norm(X1 - X2);
      const float ld2 = a012 / l12;
      const float s = 1 - 0.9f * fabsf(ld2);
      float dx1 = t.x - sel.x, dy1 = t.y - sel.y, dz1 = t.z - sel.z;
      float side1 = dx1 * dx1 + dy1 * dy1 + dz1 * dz1;
      float dx2 = pz.x - sel.x, dy2 = pz.y - sel.y, dz2 = pz.z - sel.z;
      float side2 = dx2 * dx2 + dy2 * dy2 + dz2 * dz2;
      float check1 = 100.0f + side1 - side2 - 10.0f * sqrtf(3.0f) * sqrtf(side1);
      float check2 = 100.0f + side1 - side2 + 10.0f * sqrtf(3.0f) * sqrtf(side1);
      if (double(s) > 0.1 && check1 < 0 && check2 > 0) {
        ok = 1;
        c = make_float4(s * nt.x, s * nt.y, s * nt.z, s * ld2);
      }
    }
  }
  return ok;
}

// Corner branch of the scan-to-map step (PointMapping::OptimizeTransformTobeMapped, PointMapping.cc:377-517): one query per
// FEAT_LPQ lanes, 5-NN, then line_features_fit.
template <int LPQ = FEAT_LPQ>
__device__ __forceinline__ void line_features_body(int block_x, const float4 *__restrict__ stack, int M, int slot_off, const float *__restrict__ tp,
                                                   const Vec3<float> &pz, float min_match_sq_dis, const float4 *__restrict__ map,
                                                   const int *__restrict__ cells, const GridDesc &g, uint8_t *__restrict__ valid,
                                                   float4 *__restrict__ coef, const uint32_t *__restrict__ order = nullptr) {
  const int gt = block_x * blockDim.x + threadIdx.x;
  const int it = gt / LPQ, sub = gt % LPQ;
  const bool active = it < M;
  const int i = (active && order) ? int(order[it]) - slot_off : it;   // (processing order: FeatFrame::order)
  Quat<float> q(tp[3], tp[0], tp[1], tp[2]);
  Vec3<float> t(tp[4], tp[5], tp[6]);
  float4 po = active ? stack[i] : make_float4(0, 0, 0, 0);
  Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
  Vec3<float> sel(r.x + t.x, r.y + t.y, r.z + t.z);
  float bd[5]; int bi[5], bj[5];
  knn_scan_group<5, LPQ>(sel, active, sub, map, cells, g, bd, bi, bj);
  if (!active || sub != 0) return;
  const int slot = slot_off + i;
  float4 c;
  const uint8_t ok = line_features_fit(t, pz, sel, min_match_sq_dis, bd[4], bi[4], bj, map, c);
  valid[slot] = ok; coef[slot] = c;
}

// The two fit bodies on caller-given neighbours (lio_fit_five, include/lio_test_hooks.h): one query per lane, `nbr` holds the five
// neighbours of query i at 5 i .. 5 i + 4 and stands in for the cell-sorted map, fifth_sqd[i] for the walk's bd[4] (+inf: fewer than
// five found).  form 0 features_fit<false>, 1 / 2 features_fit<true> with mapping_mode 1 / 2, 3 line_features_fit.
__global__ void __launch_bounds__(256) k_fit_five(int form, FeatScalars fs, const float *__restrict__ tp, const float4 *__restrict__ stack, int m,
                                                  const float4 *__restrict__ nbr, const float *__restrict__ fifth_sqd, uint8_t *__restrict__ valid,
                                                  float4 *__restrict__ coef, float *__restrict__ score, float4 *__restrict__ abs_coef) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Quat<float> q(tp[3], tp[0], tp[1], tp[2]);
  const Vec3<float> t(tp[4], tp[5], tp[6]);
  const float4 po = stack[i];
  const Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
  const Vec3<float> sel(r.x + t.x, r.y + t.y, r.z + t.z);
  const float bd4 = fifth_sqd[i];
  const int bi4 = bd4 == INFINITY ? INT_MAX : 0;
  const int bj[5] = {5 * i, 5 * i + 1, 5 * i + 2, 5 * i + 3, 5 * i + 4};
  uint8_t ok; float4 c, ab = make_float4(0, 0, 0, 0); float sc = 0;
  if (form == 3) {
    ok = line_features_fit(t, Vec3<float>(fs.fixed_pz[0], fs.fixed_pz[1], fs.fixed_pz[2]), sel, fs.min_match_sq_dis, bd4, bi4, bj, nbr, c);
  } else {
    const FeatResult res = form == 0 ? features_fit<false>(fs, i, q, t, po, sel, bd4, bi4, bj, nbr) : features_fit<true>(fs, i, q, t, po, sel, bd4, bi4, bj, nbr);
    ok = res.ok; c = res.c; sc = form == 0 ? res.sc : 0.f; ab = res.abs;   // the mapping forms have no score output (their kernels pass no score array)
  }
  valid[i] = ok; coef[i] = c; score[i] = sc; abs_coef[i] = ab;
}

void launch_fit_five(int form, float min_match_sq_dis, float min_plane_dis, const float fixed_pz[3], const float *transform, const float4 *stack,
                     int m, const float4 *nbr, const float *fifth_sqd, uint8_t *valid, float4 *coef, float *score, float4 *abs_coef, hipStream_t s) {
  if (m <= 0) return;
  if (form < 0 || form > 3) throw DeviceError("launch_fit_five: form is 0 .. 3");
  const FeatScalars fs{min_match_sq_dis, min_plane_dis, form == 3 ? 0 : form, {fixed_pz[0], fixed_pz[1], fixed_pz[2]}};
  hipLaunchKernelGGL(k_fit_five, dim3(cdiv(m, 256)), dim3(256), 0, s, form, fs, transform, stack, m, nbr, fifth_sqd, valid, coef, score, abs_coef);
  LIO_HIP(hipGetLastError());
}

void launch_features(const FeatArgs &a, const float *transforms, const float4 *map_sorted, const int *cells, const GridDesc &g,
                     uint8_t *valid, float4 *coef, float *score, const int *skip_flag, hipStream_t s) {
  if (a.nframes <= 0 || a.max_M <= 0) return;
  if (a.mapping_mode) throw DeviceError("launch_features: the scan-to-map forms run through launch_kf_round");
  // lanes per query: 8 when the launch is small (latency-bound: shorter per-lane candidate walks), 4 when it already fills
  // the GPU several times over (throughput-bound: fewer shuffle-merge rounds per query)
  const bool big = (long long)a.max_M * a.nframes >= 50000;
  const dim3 grid(cdiv((long long)a.max_M * (big ? 4 : 8), FEAT_THREADS), a.nframes);
  float4 *const no_abs = nullptr;   // (the unsigned plane is an output of the scan-to-map forms only)
  if (big)
    hipLaunchKernelGGL((k_features<false, 4>), grid, dim3(FEAT_THREADS), 0, s, a, transforms, map_sorted, cells, g, valid, coef, score, skip_flag, no_abs);
  else
    hipLaunchKernelGGL((k_features<false, 8>), grid, dim3(FEAT_THREADS), 0, s, a, transforms, map_sorted, cells, g, valid, coef, score, skip_flag, no_abs);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// CalculateLaserOdom: rows of (mat_A | mat_B), reduced; then the 6x6 step
// ------------------------------------------------------------------------------------------------
#define ODOM_ROW_THREADS 256
// eight slots per thread: the 28 running sums of a wave meet through 28 x 6 shuffle steps of doubles, which at two slots per thread cost more
// than the rows themselves (k_kf_rows: 467 us per round of 1000 keyframes; round 6)
int odom_rows_blocks(int nslots) { return std::max(1, std::min(cdiv(nslots, ODOM_ROW_THREADS * 8), 256)); }

__device__ __forceinline__ void odom_rows_body(int block_x, int nblocks, const float4 *__restrict__ stack, int M, int nslots,
                                               const uint8_t *__restrict__ valid, const float4 *__restrict__ coef,
                                               const OdomState *__restrict__ st, double *__restrict__ partials, int b_from_coef) {
  Quat<float> q(st->T[3], st->T[0], st->T[1], st->T[2]);
  Vec3<float> t(st->T[4], st->T[5], st->T[6]);
  Mat3<float> Rm = toRot(q);
  Mat3<float> Rinv = toRot(qinverse(q));
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0;
  for (int sidx = block_x * blockDim.x + threadIdx.x; sidx < nslots; sidx += nblocks * blockDim.x) {
    if (!valid[sidx]) continue;
    odom_row_accumulate(stack[sidx % M], coef[sidx], q, t, Rm, Rinv, b_from_coef, acc);
  }
  // wave reduce (64 lanes) then cross-wave through LDS
  __shared__ double sm[ODOM_ROW_THREADS / 64][28];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 28; ++k) {
    double v = acc[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sm[wv][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 28) {
    double v = 0;
    for (int w = 0; w < ODOM_ROW_THREADS / 64; ++w) v += sm[w][threadIdx.x];
    partials[block_x * 28 + threadIdx.x] = v;
  }
}

__device__ __forceinline__ void odom_update_body(const double *__restrict__ partials, int nblocks, OdomState *st, int iter, int min_rows,
                                                 int left_update) {
  // column k of the partials is summed by lane k (fixed order), then lane 0 runs the scalar 6x6 step
  __shared__ double ssum[28];
  reduce_partials28(partials, nblocks, ssum);
  odom_update_from_sums(ssum, st, iter, min_rows, left_update);
}

template <int LPQ>
__global__ void __launch_bounds__(ODOM_ROUND_THREADS) k_odom_round(FeatArgs a, const OdomState *__restrict__ st, const float4 *__restrict__ map,
                                                                  const int *__restrict__ cells, GridDesc g, uint8_t *__restrict__ valid,
                                                                  float4 *__restrict__ coef, float *__restrict__ score, double *__restrict__ partials,
                                                                  int base_slot, int round, int keep) {
  if (st->converged) return;
  const float *tp = st->T;
  const Quat<float> q(tp[3], tp[0], tp[1], tp[2]);
  const Vec3<float> t(tp[4], tp[5], tp[6]);
  const double v = odom_round_block<LPQ>(feat_scalars(a), a.fr[0], q, t, map, cells, g, valid, coef, score, base_slot, round, keep, int(blockIdx.x));
  if (threadIdx.x < 28) partials[size_t(blockIdx.x) * 28 + threadIdx.x] = v;
}

__global__ void __launch_bounds__(1024) k_odom_update_wide(const double *__restrict__ partials, int nblocks, OdomState *st, int iter, int min_rows,
                                                           int left_update, OdomState *mail, HostSignal sig) {
  odom_update_wide_block(partials, nblocks, st, iter, min_rows, left_update, mail, sig);
}
__global__ void __launch_bounds__(256) k_solve_setup(SolveSetup a, float *__restrict__ d_transforms, OdomState *__restrict__ d_odom, uint8_t *__restrict__ valid,
                                                     size_t n_valid) {
  clear_valid_block(valid, n_valid);
  if (blockIdx.x == 0) {
    for (int k = threadIdx.x; k < a.ntf * 8; k += 256) d_transforms[k] = a.tf[k >> 3][k & 7];
    if (a.set_odom) odom_state_init(d_odom, a.odom_T, false);
  }
}
void launch_solve_setup(const SolveSetup &a, float *d_transforms, OdomState *d_odom, uint8_t *valid, size_t n_valid, hipStream_t s) {
  const int nb = std::max(1, cdiv((long long)n_valid, 256 * 16));
  hipLaunchKernelGGL(k_solve_setup, dim3(nb), dim3(256), 0, s, a, d_transforms, d_odom, valid, n_valid);
  LIO_HIP(hipGetLastError());
}

int odom_round_blocks(int M, int lpq) { return std::max(1, cdiv((long long)M * lpq, ODOM_ROUND_THREADS)); }
void launch_odom_round(const FeatArgs &a, int base_slot, int round, int keep, OdomState *st, const float4 *map_sorted, const int *cells, const GridDesc &g,
                       uint8_t *valid, float4 *coef, float *score, double *partials, hipStream_t s, OdomState *mail, const HostSignal &sig, int lpq) {
  const int M = a.fr[0].M;
  if (M <= 0) return;
  const int nb = odom_round_blocks(M, lpq);
  if (lpq == 4)
    hipLaunchKernelGGL(k_odom_round<4>, dim3(nb), dim3(ODOM_ROUND_THREADS), 0, s, a, st, map_sorted, cells, g, valid, coef, score, partials, base_slot, round, keep);
  else
    hipLaunchKernelGGL(k_odom_round<8>, dim3(nb), dim3(ODOM_ROUND_THREADS), 0, s, a, st, map_sorted, cells, g, valid, coef, score, partials, base_slot, round, keep);
  hipLaunchKernelGGL(k_odom_update_wide, dim3(1), dim3(1024), 0, s, partials, nb, st, round, 0, 0, mail, sig);
  LIO_HIP(hipGetLastError());
}

// ---- the Gauss-Newton test hooks (include/lio_test_hooks.h): small kernels around the production device functions
// lio_gn_rows_map: the row of every slot on its own, one query per lane, through the odom_row_form the rows kernels call; 7 floats per slot
// (a0 .. a5, b), zeros and ok = 0 where valid is 0
__global__ void __launch_bounds__(256) k_gn_rows_map(const float4 *__restrict__ stack, int m, const uint8_t *__restrict__ valid, const float4 *__restrict__ coef,
                                                     const OdomState *__restrict__ st, int b_from_coef, uint8_t *__restrict__ ok_out,
                                                     float *__restrict__ rows_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  Quat<float> q(st->T[3], st->T[0], st->T[1], st->T[2]);
  Vec3<float> t(st->T[4], st->T[5], st->T[6]);
  Mat3<float> Rm = toRot(q);
  Mat3<float> Rinv = toRot(qinverse(q));
  float a[6] = {0, 0, 0, 0, 0, 0}, bb = 0;
  const bool ok = valid[i] != 0;
  if (ok) odom_row_form(stack[i], coef[i], q, t, Rm, Rinv, b_from_coef, a, bb);
  ok_out[i] = ok ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) rows_out[size_t(i) * 7 + k] = a[k];
  rows_out[size_t(i) * 7 + 6] = bb;
}
void launch_gn_rows_map(const float4 *stack, int m, const uint8_t *valid, const float4 *coef, const OdomState *st, int b_from_coef, uint8_t *ok_out,
                        float *rows_out, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_gn_rows_map, dim3(cdiv(m, 256)), dim3(256), 0, s, stack, m, valid, coef, st, b_from_coef, ok_out, rows_out);
  LIO_HIP(hipGetLastError());
}
// lio_gn_fold: one block of the size production folds with; the 28 shared sums go out as they stand
__global__ void __launch_bounds__(256) k_gn_fold(const double *__restrict__ partials, int nblocks, double *__restrict__ sums_out) {
  __shared__ double ssum[28];
  reduce_partials28(partials, nblocks, ssum);
  if (threadIdx.x < 28) sums_out[threadIdx.x] = ssum[threadIdx.x];
}
__global__ void __launch_bounds__(1024) k_gn_fold_wide(const double *__restrict__ partials, int nblocks, double *__restrict__ sums_out) {
  __shared__ double ssum[28];
  fold_partials28_wide(partials, nblocks, ssum);
  if (threadIdx.x < 28) sums_out[threadIdx.x] = ssum[threadIdx.x];
}
void launch_gn_fold(const double *partials, int nblocks, int wide, double *sums_out, hipStream_t s) {
  if (wide) hipLaunchKernelGGL(k_gn_fold_wide, dim3(1), dim3(1024), 0, s, partials, nblocks, sums_out);
  else hipLaunchKernelGGL(k_gn_fold, dim3(1), dim3(256), 0, s, partials, nblocks, sums_out);
  LIO_HIP(hipGetLastError());
}
// lio_gn_step, family 0: thread 0 of one wave runs odom_update_from_sums on the state in place
__global__ void __launch_bounds__(64) k_gn_step(const double *__restrict__ sums, OdomState *st, int iter, int min_rows, int left_update) {
  odom_update_from_sums(sums, st, iter, min_rows, left_update);
}
void launch_gn_step(const double *sums, OdomState *st, int iter, int min_rows, int left_update, hipStream_t s) {
  hipLaunchKernelGGL(k_gn_step, dim3(1), dim3(64), 0, s, sums, st, iter, min_rows, left_update);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// The scan-to-map loop over a table of keyframes: B independent loops advance together, one launch per stage per round (kf_batch.hip: a batch,
// mapping.hip: a table of one).  blockIdx.y = 0 runs the corner (line) branch against the corner map, 1 the surf (plane) branch against the surf map.
// ------------------------------------------------------------------------------------------------
template <int LPQ>
__device__ __forceinline__ void kf_round_body(const KfDesc *__restrict__ kd, const KfMapDesc *__restrict__ md, const OdomState *__restrict__ st,
                                                 const float4 *__restrict__ stack_all, const uint32_t *__restrict__ order, float min_match_sq_dis, float min_plane_dis,
                                                 int mapping_mode, uint8_t *__restrict__ valid, float4 *__restrict__ coef, float4 *__restrict__ abs_coef) {
  const int k = blockIdx.z;
  if (st[k].converged) return;
  const KfDesc d = kd[k];
  const float *tp = st[k].T;
  if (blockIdx.y == 0) {
    if (int(blockIdx.x) * 128 >= d.Mc * LPQ) return;
    const KfMapDesc &m = md[d.map];
    // (the maps' pointers come from a descriptor: tied to a kernel argument they are global to the compiler, dev.h: rebase)
    line_features_body<LPQ>(blockIdx.x, stack_all + d.slot_off, d.Mc, d.slot_off, tp, Vec3<float>(d.pz[0], d.pz[1], d.pz[2]), min_match_sq_dis,
                       rebase(stack_all, m.corner_sorted), rebase(stack_all, m.corner_cells), m.corner_grid, valid, coef, order ? order + d.slot_off : nullptr);
  } else {
    if (int(blockIdx.x) * 128 >= d.Ms * LPQ) return;
    const KfMapDesc &m = md[d.map];
    const FeatFrame fr{stack_all + d.slot_off + d.Mc, d.Ms, d.slot_off + d.Mc, 0, order ? order + d.slot_off + d.Mc : nullptr};
    const FeatScalars fs{min_match_sq_dis, min_plane_dis, mapping_mode, {d.pz[0], d.pz[1], d.pz[2]}};
    features_body<true, LPQ>(fr, fs, blockIdx.x, tp, rebase(stack_all, m.surf_sorted), rebase(stack_all, m.surf_cells), m.surf_grid, valid, coef, nullptr, abs_coef);
  }
}

template <int LPQ>
__global__ void __launch_bounds__(128) k_kf_round(const KfDesc *__restrict__ kd, const KfMapDesc *__restrict__ md, const OdomState *__restrict__ st,
                                                 const float4 *__restrict__ stack_all, const uint32_t *__restrict__ order, float min_match_sq_dis, float min_plane_dis,
                                                 int mapping_mode, uint8_t *__restrict__ valid, float4 *__restrict__ coef, float4 *__restrict__ abs_coef) {
  kf_round_body<LPQ>(kd, md, st, stack_all, order, min_match_sq_dis, min_plane_dis, mapping_mode, valid, coef, abs_coef);
}
// the one-lane-per-query form is bound by gather latency: 8 waves per SIMD (64 VGPRs, the fit phase spills a little) beats
// the 5 waves the default allocation gives by 15% (54.4 -> 46.1 ms at 1000 HDL-64 keyframes)
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_kf_round1_w8(const KfDesc *__restrict__ kd, const KfMapDesc *__restrict__ md, const OdomState *__restrict__ st,
               const float4 *__restrict__ stack_all, const uint32_t *__restrict__ order, float min_match_sq_dis, float min_plane_dis,
               int mapping_mode, uint8_t *__restrict__ valid, float4 *__restrict__ coef, float4 *__restrict__ abs_coef) {
  kf_round_body<1>(kd, md, st, stack_all, order, min_match_sq_dis, min_plane_dis, mapping_mode, valid, coef, abs_coef);
}

__global__ void __launch_bounds__(ODOM_ROW_THREADS) k_kf_rows(const KfDesc *__restrict__ kd, const OdomState *__restrict__ st,
                                                              const float4 *__restrict__ stack_all, const uint8_t *__restrict__ valid,
                                                              const float4 *__restrict__ coef, double *__restrict__ partials, int b_from_coef) {
  const int k = blockIdx.y;
  if (st[k].converged) return;
  const KfDesc d = kd[k];
  if (int(blockIdx.x) >= d.nb) return;
  const int M = d.Mc + d.Ms;
  odom_rows_body(blockIdx.x, d.nb, stack_all + d.slot_off, M, M, valid + d.slot_off, coef + d.slot_off, st + k, partials + size_t(d.part_off) * 28,
                 b_from_coef);
}

__global__ void k_kf_update(const KfDesc *__restrict__ kd, OdomState *st, const double *__restrict__ partials, int iter, int min_rows, int left_update,
                            int *n_converged, char *mail, HostSignal sig) {
  const int k = blockIdx.x;
  if (!st[k].converged) {
    const KfDesc d = kd[k];
    odom_update_body(partials + size_t(d.part_off) * 28, d.nb, st + k, iter, min_rows, left_update);
    if (n_converged && threadIdx.x == 0 && st[k].converged) atomicAdd(n_converged, 1);
  }
  if (sig.flag) {   // the rounds at which the host looks post every keyframe's state to its own mailbox slot, then its own completion word (dev.h)
    __syncthreads();
    HostSignal mine = sig;
    char *slot = state_mail_slot(mail, mine, k);
    if (threadIdx.x < 64) post_host_mail(mine, slot, st + k, int(sizeof(OdomState) / 4), threadIdx.x);
  }
}

// the map cell of every query under its keyframe's current transform: the key the queries' processing order is sorted by (all ones: outside
// the map's grid — such a query finds nothing and costs nothing wherever it sits)
__global__ void __launch_bounds__(256) k_kf_query_keys(const KfDesc *__restrict__ kd, const KfMapDesc *__restrict__ md, const OdomState *__restrict__ st,
                                                      const float4 *__restrict__ stack_all, uint32_t *__restrict__ keys) {
  const int k = blockIdx.z;
  const KfDesc d = kd[k];
  const bool surf = blockIdx.y == 1;
  const int M = surf ? d.Ms : d.Mc, i = int(blockIdx.x) * 256 + threadIdx.x;
  if (i >= M) return;
  const int slot = d.slot_off + (surf ? d.Mc : 0) + i;
  const KfMapDesc &m = md[d.map];
  const GridDesc &g = surf ? m.surf_grid : m.corner_grid;
  const float *tp = st[k].T;
  const Quat<float> q(tp[3], tp[0], tp[1], tp[2]);
  const float4 po = stack_all[slot];
  const Vec3<float> r = rotate(q, Vec3<float>(po.x, po.y, po.z));
  int cx, cy, cz;
  const bool in = cell_of(r.x + tp[4], r.y + tp[5], r.z + tp[6], g, cx, cy, cz);
  keys[slot] = in ? cell_index(cx, cy, cz, g) : 0xFFFFFFFFu;
}
void launch_kf_query_keys(const KfDesc *kd, const KfMapDesc *md, const OdomState *st, int n_keyframes, int max_Mc, int max_Ms, const float4 *stack_all, uint32_t *keys,
                          hipStream_t s) {
  if (n_keyframes <= 0) return;
  hipLaunchKernelGGL(k_kf_query_keys, dim3(std::max(1, cdiv(std::max(max_Mc, max_Ms), 256)), 2, n_keyframes), dim3(256), 0, s, kd, md, st, stack_all, keys);
  LIO_HIP(hipGetLastError());
}

void launch_kf_round(const KfDesc *kd, const KfMapDesc *md, const OdomState *st, int n_keyframes, int max_Mc, int max_Ms, int lpq, const float4 *stack_all,
                     const uint32_t *order, float min_match_sq_dis, float min_plane_dis, int mapping_mode, uint8_t *valid, float4 *coef, float4 *abs_coef,
                     hipStream_t s) {
  if (lpq != 1 && lpq != 4 && lpq != 8) throw DeviceError("launch_kf_round: lanes per query is 1, 4 or 8");
  const int bx = std::max(1, cdiv((long long)std::max(max_Mc, max_Ms) * lpq, 128));
  const dim3 grid(bx, 2, n_keyframes);
  if (lpq == 1) hipLaunchKernelGGL(k_kf_round1_w8, grid, dim3(128), 0, s, kd, md, st, stack_all, order, min_match_sq_dis, min_plane_dis, mapping_mode, valid, coef, abs_coef);
  else if (lpq == 4) hipLaunchKernelGGL(k_kf_round<4>, grid, dim3(128), 0, s, kd, md, st, stack_all, order, min_match_sq_dis, min_plane_dis, mapping_mode, valid, coef, abs_coef);
  else hipLaunchKernelGGL(k_kf_round<8>, grid, dim3(128), 0, s, kd, md, st, stack_all, order, min_match_sq_dis, min_plane_dis, mapping_mode, valid, coef, abs_coef);
  LIO_HIP(hipGetLastError());
}
void launch_kf_rows(const KfDesc *kd, const OdomState *st, int n_keyframes, int max_nb, const float4 *stack_all, const uint8_t *valid, const float4 *coef,
                    double *partials, int b_from_coef, hipStream_t s) {
  hipLaunchKernelGGL(k_kf_rows, dim3(max_nb, n_keyframes), dim3(ODOM_ROW_THREADS), 0, s, kd, st, stack_all, valid, coef, partials, b_from_coef);
  LIO_HIP(hipGetLastError());
}
void launch_kf_update(const KfDesc *kd, OdomState *st, int n_keyframes, const double *partials, int iter, int min_rows, int left_update, int *n_converged,
                      char *mail, const HostSignal &sig, hipStream_t s) {
  hipLaunchKernelGGL(k_kf_update, dim3(n_keyframes), dim3(256), 0, s, kd, st, partials, iter, min_rows, left_update, n_converged, mail, sig);
  LIO_HIP(hipGetLastError());
}

}  // namespace lio
