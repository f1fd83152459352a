// mapping.hip — PointMapping on the GPU (see mapping.h for the layout).  No CPU path: every stage below is a HIP
// kernel or a rocPRIM primitive; the host only does the 6-DoF bookkeeping (transform algebra, cube-window shift,
// FOV test of <= 125 cubes).
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>

#include "mapping.h"
#include "cloud_device.h"

namespace lio {

namespace {

__host__ __device__ inline uint32_t pack_cube(int ai, int aj, int ak) {
  return (uint32_t(ai + 512) << 20) | (uint32_t(aj + 512) << 10) | uint32_t(ak + 512);
}
// what pack_cube holds per axis: the offsets of a window's cubes from its centre, [-cen, dim - cen), must lie inside (MappingDev::CenFits)
constexpr int kCubeOffsetMin = -512, kCubeOffsetMax = 511;
__host__ __device__ inline void unpack_cube(uint32_t k, int &ai, int &aj, int &ak) {
  ai = int((k >> 20) & 1023u) - 512; aj = int((k >> 10) & 1023u) - 512; ak = int(k & 1023u) - 512;
}

// int((v + 25.0) / 50.0) + cen, minus one for negative arguments (PointMapping.cc:810-817,1126-1132)
__host__ __device__ inline int cube_coord(float v, int cen) {
  int r = int((double(v) + 25.0) / 50.0) + cen;
  if (double(v) + 25.0 < 0) --r;
  return r;
}

__device__ inline uint32_t rank_of_key(uint32_t key, const MapValidSet &vs) {
  int ai, aj, ak;
  unpack_cube(key, ai, aj, ak);
  if (ai < vs.lo[0] || ai >= vs.hi[0] || aj < vs.lo[1] || aj >= vs.hi[1] || ak < vs.lo[2] || ak >= vs.hi[2]) return LIO_MAP_RANK_DROP;
  int lo = 0, hi = vs.n;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (vs.key[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < vs.n && vs.key[lo] == key) ? uint32_t(lo) : LIO_MAP_RANK_REST;
}

__device__ inline void count_classes(uint32_t r, bool active, int *n_valid, int *n_rest) {
  const unsigned long long bv = __ballot(active && r < LIO_MAP_RANK_REST);
  const unsigned long long br = __ballot(active && r == LIO_MAP_RANK_REST);
  if ((threadIdx.x & 63) == 0) {
    if (bv) atomicAdd(n_valid, __popcll(bv));
    if (br) atomicAdd(n_rest, __popcll(br));
  }
}

__global__ void k_map_rank(const uint32_t *__restrict__ pkey, int n, MapValidSet vs, uint32_t *__restrict__ rk, uint32_t *__restrict__ vals,
                           MapCounters *cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t r = LIO_MAP_RANK_DROP;
  if (i < n) {
    r = rank_of_key(pkey[i], vs);
    rk[i] = r; vals[i] = uint32_t(i);
  }
  count_classes(r, i < n, &cnt->n_valid, &cnt->n_rest);
}

// sorted order = [valid cubes by rank | rest | dropped]; written out as [rest | valid]
__global__ void k_map_gather(const float4 *__restrict__ pool, const uint32_t *__restrict__ pkey, const uint32_t *__restrict__ rk_sorted,
                             const uint32_t *__restrict__ src_sorted, int n, const MapCounters *__restrict__ cnt, float4 *__restrict__ pool_out,
                             uint32_t *__restrict__ pkey_out, uint32_t *__restrict__ vrank) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t r = rk_sorted[s];
  if (r == LIO_MAP_RANK_DROP) return;
  const int nv = cnt->n_valid, nr = cnt->n_rest;
  const uint32_t src = src_sorted[s];
  int dst;
  if (r < LIO_MAP_RANK_REST) { dst = nr + s; vrank[s] = r; }
  else dst = s - nv;
  pool_out[dst] = pool[src];
  pkey_out[dst] = pkey[src];
}

// PointAssociateToMap then the cube of the mapped point (PointMapping.cc:1122-1139)
__global__ void k_map_new(const float4 *__restrict__ sensor_pts, int n, Quat<float> q, Vec3<float> t, int c0, int c1, int c2, MapValidSet vs,
                          float4 *__restrict__ new_pts, uint32_t *__restrict__ new_key, uint32_t *__restrict__ rk, uint32_t *__restrict__ vals,
                          MapCounters *cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t r = LIO_MAP_RANK_DROP;
  if (i < n) {
    float4 p = sensor_pts[i];
    Vec3<float> v = rotate(q, Vec3<float>(p.x, p.y, p.z));
    p.x = v.x + t.x; p.y = v.y + t.y; p.z = v.z + t.z;
    const int ci = cube_coord(p.x, c0), cj = cube_coord(p.y, c1), ck = cube_coord(p.z, c2);
    uint32_t key = 0;
    if (ci >= 0 && ci < MappingDev::L && cj >= 0 && cj < MappingDev::Wd && ck >= 0 && ck < MappingDev::H) {
      key = pack_cube(ci - c0, cj - c1, ck - c2);
      r = rank_of_key(key, vs);
    }
    new_pts[i] = p; new_key[i] = key; rk[i] = r; vals[i] = uint32_t(i);
  }
  count_classes(r, i < n, &cnt->n_new_valid, &cnt->n_new_rest);
}

// new points, sorted [valid by rank | rest | dropped]: valid ones are appended to the voxel work list U behind the
// nV map points of those cubes, rest ones behind the untouched part of the pool
__global__ void k_new_scatter(const float4 *__restrict__ new_pts, const uint32_t *__restrict__ new_key, const uint32_t *__restrict__ rk_sorted,
                              const uint32_t *__restrict__ src_sorted, int n_new, const MapCounters *__restrict__ cnt, int nV, int n_rest,
                              float4 *__restrict__ u_pts, uint32_t *__restrict__ u_rank, float4 *__restrict__ pool, uint32_t *__restrict__ pkey) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_new) return;
  const int nnv = cnt->n_new_valid, nnr = cnt->n_new_rest;
  const uint32_t src = src_sorted[s];
  if (s < nnv) {
    u_pts[nV + s] = new_pts[src];
    u_rank[nV + s] = rk_sorted[s];
  } else {
    u_rank[nV + s] = 0xFFFFFFFFu;  // padding of the work list
    if (s < nnv + nnr) {
      pool[n_rest + (s - nnv)] = new_pts[src];
      pkey[n_rest + (s - nnv)] = new_key[src];
    }
  }
}

__device__ inline int f2ord(float f) { int b = __float_as_int(f); return b >= 0 ? b : b ^ 0x7FFFFFFF; }
__host__ __device__ inline float ord2f(int o) {
  int b = o >= 0 ? o : o ^ 0x7FFFFFFF;
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __int_as_float(b);
#else
  std::memcpy(&f, &b, sizeof(f));
#endif
  return f;
}

__global__ void k_cube_bounds_init(int *__restrict__ cb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < LIO_MAP_MAX_VALID * 6) cb[i] = (i % 6) < 3 ? INT_MAX : INT_MIN;
}

// per-cube bounding box of the work list (the min_p/max_p pcl::VoxelGrid computes per cube cloud); LDS atomics per
// block, one global atomic per touched (cube, component)
__global__ void __launch_bounds__(256) k_cube_bounds(const float4 *__restrict__ u_pts, const uint32_t *__restrict__ u_rank, int n, int *__restrict__ cb) {
  __shared__ int sm[LIO_MAP_MAX_VALID * 6];
  for (int k = threadIdx.x; k < LIO_MAP_MAX_VALID * 6; k += blockDim.x) sm[k] = (k % 6) < 3 ? INT_MAX : INT_MIN;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint32_t r = u_rank[i];
    if (r < LIO_MAP_MAX_VALID) {
      const float4 p = u_pts[i];
      int *b = sm + r * 6;
      atomicMin(b + 0, f2ord(p.x)); atomicMin(b + 1, f2ord(p.y)); atomicMin(b + 2, f2ord(p.z));
      atomicMax(b + 3, f2ord(p.x)); atomicMax(b + 4, f2ord(p.y)); atomicMax(b + 5, f2ord(p.z));
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < LIO_MAP_MAX_VALID * 6; k += blockDim.x) {
    const int v = sm[k];
    if ((k % 6) < 3) { if (v != INT_MAX) atomicMin(cb + k, v); }
    else if (v != INT_MIN) atomicMax(cb + k, v);
  }
}

__global__ void k_cube_vox_keys(const float4 *__restrict__ u_pts, const uint32_t *__restrict__ u_rank, int n, const int *__restrict__ cb,
                                float inv_leaf, unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = u_rank[i];
  unsigned long long key = ~0ull;
  if (r < LIO_MAP_MAX_VALID) {
    const int *b = cb + r * 6;
    const int minb0 = int(floorf(ord2f(b[0]) * inv_leaf)), minb1 = int(floorf(ord2f(b[1]) * inv_leaf)), minb2 = int(floorf(ord2f(b[2]) * inv_leaf));
    const int div0 = int(floorf(ord2f(b[3]) * inv_leaf)) - minb0 + 1, div1 = int(floorf(ord2f(b[4]) * inv_leaf)) - minb1 + 1;
    const float4 p = u_pts[i];
    const int i0 = int(floorf(p.x * inv_leaf) - float(minb0));
    const int i1 = int(floorf(p.y * inv_leaf) - float(minb1));
    const int i2 = int(floorf(p.z * inv_leaf) - float(minb2));
    const unsigned int vk = static_cast<unsigned int>(i0 + i1 * div0 + i2 * div0 * div1);
    key = (static_cast<unsigned long long>(r) << 32) | vk;
  }
  keys[i] = key;
  vals[i] = uint32_t(i);
}

__global__ void k_heads64(const unsigned long long *__restrict__ keys, int n, int *__restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  flags[i] = (k != ~0ull && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

// voxel centroids (x, y, z, intensity averaged; ascending (cube, voxel)) written behind the untouched pool part
__global__ void k_cube_centroids(const float4 *__restrict__ u_pts, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals,
                                 const int *__restrict__ flags, const int *__restrict__ pos, int n, MapValidSet vs, int n_rest, MapCounters *cnt,
                                 float4 *__restrict__ pool, uint32_t *__restrict__ pkey, uint32_t *__restrict__ vrank) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == n - 1) cnt->n_out = pos[i] + flags[i];
  if (!flags[i]) return;
  const unsigned long long k = keys[i];
  float ax = 0, ay = 0, az = 0, ai = 0;
  int e = i;
  while (e < n && keys[e] == k) {  // stable sort: map points first, then the new ones, each in their own order
    const float4 p = u_pts[vals[e]];
    ax += p.x; ay += p.y; az += p.z; ai += p.w;
    ++e;
  }
  const float c = float(e - i);
  const uint32_t r = uint32_t(k >> 32);
  const int dst = n_rest + cnt->n_new_rest + pos[i];
  pool[dst] = make_float4(ax / c, ay / c, az / c, ai / c);
  pkey[dst] = vs.key[r];
  vrank[pos[i]] = r;
}

// stack round trip of PointMapping::Process (:789-801 then :991-1003): to the map with the predicted transform and
// back again, in float, exactly as the reference does before it voxel-filters the stack
__device__ __forceinline__ float4 stack_roundtrip_point(const float4 p, const Quat<float> &q, const Vec3<float> &t) {
  Vec3<float> m = rotate(q, Vec3<float>(p.x, p.y, p.z));
  m = Vec3<float>(m.x + t.x, m.y + t.y, m.z + t.z);
  Vec3<float> v(m.x - t.x, m.y - t.y, m.z - t.z);
  Vec3<float> r = rotate(conj(q), v);
  return make_float4(r.x, r.y, r.z, p.w);
}

// ---- the kernels of ProcessBatch (include/lio_map_batch.h) around the keyframe chain of cloud_kernels.h: plain streaming kernels, 256 threads, one
// float4 per lane, every sensor (or cloud) with its own record of a device table.  A block beyond a record's own points leaves at once.
// One sensor's stack clouds (0 corner, 1 surf) and the transform_tobe_mapped_ its association left
struct MbStackRec { const float4 *in[2]; float4 *out[2]; int n[2]; Quat<float> q; Vec3<float> t; };
// grid (cdiv(max n, 256), 2, sensors): stack_roundtrip_point on every sensor's two clouds with the sensor's own T0
__global__ void __launch_bounds__(256) k_mb_roundtrip(const MbStackRec *__restrict__ recs) {
  const MbStackRec &r = recs[blockIdx.z];
  const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n[c]) return;
  r.out[c][i] = stack_roundtrip_point(r.in[c][i], r.q, r.t);
}
// One sensor of a step fed from the device (lio_map_process_batch_from_odom): its stack clouds where the odometry keeps them, and the full
// cloud it takes with them (cloud_kernels.h; n = 0: none) into the handle's full_
struct MbFromOdomRec { MbStackRec stack; FullTake full; };
// grid (cdiv(max n, 256), 3, sensors): y 0 and 1 are k_mb_roundtrip's, y 2 is full_take_body (cloud_device.h)
__global__ void __launch_bounds__(256) k_mb_from_odom(const MbFromOdomRec *__restrict__ recs) {
  const MbFromOdomRec &r = recs[blockIdx.z];
  const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (c < 2) {
    if (i >= r.stack.n[c]) return;
    r.stack.out[c][i] = stack_roundtrip_point(r.stack.in[c][i], r.stack.q, r.stack.t);
    return;
  }
  if (i >= r.full.n) return;
  full_take_body(r.full.in, r.full.out, i, r.full.to_end.st, r.full.to_end);
}
// One iterating sensor's slice [slot_off, slot_off + Mc + Ms) of the chain's arrays and where the handle keeps the same: its filtered stacks
// (taken), and its own stack_all_ / f_coef_ / f_abs_ / f_valid_ (given back)
struct MbSliceRec { const float4 *stack_ds[2]; int M[2]; int slot_off; float4 *stack_all; float4 *coef; float4 *abs_coef; uint8_t *valid; };
// grid (cdiv(max M, 256), 2, sensors): the filtered corner stack, then the surf stack, into the chain's stack_all
__global__ void __launch_bounds__(256) k_mb_take(const MbSliceRec *__restrict__ recs, float4 *__restrict__ stack_all) {
  const MbSliceRec &r = recs[blockIdx.z];
  const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= r.M[c]) return;
  stack_all[r.slot_off + (c ? r.M[0] : 0) + i] = r.stack_ds[c][i];
}
// grid (cdiv(max Mc + Ms, 256), 4, sensors): what the last executed round left at the sensor's slots, into the handle (array 0 the stack,
// 1 coef, 2 abs_coef, 3 the valid bytes)
__global__ void __launch_bounds__(256) k_mb_give(const MbSliceRec *__restrict__ recs, const float4 *__restrict__ stack_all, const float4 *__restrict__ coef,
                                                 const float4 *__restrict__ abs_coef, const uint8_t *__restrict__ valid) {
  const MbSliceRec &r = recs[blockIdx.z];
  const int a = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= r.M[0] + r.M[1]) return;
  const int slot = r.slot_off + i;
  if (a == 0) r.stack_all[i] = stack_all[slot];
  else if (a == 1) r.coef[i] = coef[slot];
  else if (a == 2) r.abs_coef[i] = abs_coef[slot];
  else r.valid[i] = valid[slot];
}

// Surround map, step 1: the bin of every point of [corner pool | surf pool].  A point of surround cube `slot` (list order) and class
// c gets bin 2 * slot + c, so ascending bins are PointMapping.cc:1225-1229's order (cube by cube, corner cloud then surf cloud); a point
// of any other cube gets LIO_MAP_SURROUND_DROP, which sorts behind every kept one.  The kept points are counted per wave.
__global__ void __launch_bounds__(256) k_surround_bins(const uint32_t *__restrict__ pkey_c, int n_c, const uint32_t *__restrict__ pkey_s, int n_s,
                                                       MapSurroundSet ss, uint32_t *__restrict__ bin, int *__restrict__ n_kept) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n_c + n_s;
  uint32_t b = LIO_MAP_SURROUND_DROP;
  if (in) {
    const uint32_t cls = i >= n_c ? 1u : 0u;
    const uint32_t key = cls ? pkey_s[i - n_c] : pkey_c[i];
    int lo = 0, hi = ss.n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ss.key[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < ss.n && ss.key[lo] == key) b = 2u * uint32_t(lo) + cls;
    bin[i] = b;
  }
  const unsigned long long kept = __ballot(in && b != LIO_MAP_SURROUND_DROP);
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(n_kept, __popcll(kept));
}

// step 3 (step 2 is the stable 8-bit seg_sort pass on the bins): the kept points, which the sort left in front, in sorted order
__global__ void __launch_bounds__(256) k_surround_gather(const float4 *__restrict__ pool_c, int n_c, const float4 *__restrict__ pool_s, int n_s,
                                                         const uint32_t *__restrict__ bin_sorted, const uint32_t *__restrict__ src_sorted,
                                                         float4 *__restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_c + n_s) return;
  if (bin_sorted[s] == LIO_MAP_SURROUND_DROP) return;
  const uint32_t src = src_sorted[s];
  if (src >= uint32_t(n_c + n_s)) return;
  out[s] = src < uint32_t(n_c) ? pool_c[src] : pool_s[src - uint32_t(n_c)];
}

// math_utils.h:186-203 (degrees)
inline Vec3<double> r2ypr_deg(const Mat3<double> &R) {
  const double y = std::atan2(R(1, 0), R(0, 0));
  const double p = std::atan2(-R(2, 0), R(0, 0) * std::cos(y) + R(1, 0) * std::sin(y));
  const double r = std::atan2(R(0, 2) * std::sin(y) - R(1, 2) * std::cos(y), -R(0, 1) * std::sin(y) + R(1, 1) * std::cos(y));
  return Vec3<double>(y / M_PI * 180.0, p / M_PI * 180.0, r / M_PI * 180.0);
}
inline Mat3<double> to_double(const Mat3<float> &m) { Mat3<double> r; for (int k = 0; k < 9; ++k) r.m[k] = double(m.m[k]); return r; }

}  // namespace

// The launch chain of ProcessBatch and its scratch, kept by the first handle of a call (Process: the handle itself).  No results live here: poses,
// clouds, maps and the score list's arrays are the handles' own.  The members below the buffers are the call's steps in their order; the work of
// a handle stays on its own streams but for the launches that serve every sensor at once, which run on the first handle's stream s0.
struct MapChain {
  MappingDev *const *m = nullptr;       // the call's handles
  int n = 0;
  hipStream_t s0 = nullptr;
  std::vector<MappingDev::Step> steps;
  std::vector<MbStackRec> h_stack;
  DBuf<MbStackRec> d_stack;
  std::vector<MbFromOdomRec> h_from;    // a step fed from the device: this table in the place of h_stack
  DBuf<MbFromOdomRec> d_from;
  bool any_stack = false;               // some handle brought a cloud: the round trip (fed from the device: k_mb_from_odom) ran
  std::vector<int> act;                 // the handles (indices into the call) whose rounds run: the keyframe table's order
  GridBatch clouds;                     // the from-map clouds of `act` (2 * nA): their bounds side by side; the grids are the handles' own
  DBuf<float4> stack_all, coef, abs_coef;
  DBuf<uint8_t> valid;
  DBuf<double> partials;
  HostBuf<char> h_table;                // pinned: nA KfMapDesc, nA KfDesc, nA OdomState, nA MbSliceRec, one behind the other: one upload
  DBuf<char> d_table;
  size_t off_kd = 0, off_st = 0, off_sl = 0;
  int max_Mc = 0, max_Ms = 0, max_nb = 0;
  StateMail mail;                       // the sensors' states at the peeks
  hipEvent_t ev = nullptr;              // behind the round trip of the stacks: every other handle's filters wait for it
  MapChain() { LIO_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); }
  ~MapChain() { if (ev) (void)hipEventDestroy(ev); }
  MapChain(const MapChain &) = delete;
  MapChain &operator=(const MapChain &) = delete;

  int nA() const { return int(act.size()); }
  MappingDev &dev(int j) const { return *m[act[size_t(j)]]; }
  void Prepare(MappingDev *const *handles, int n_handles, const OdomSweep *sweep);
  void Filter();
  void MakeGrids();
  void FillTable();
  void Iterate();
  void GiveBack();
  void Update();
};

// ------------------------------------------------------------------------------------------------
MappingDev::MappingDev(const lio_map_config &cfg) : cfg_(cfg) {
  int nd = 0;
  LIO_HIP(hipGetDeviceCount(&nd));
  if (nd <= 0) throw DeviceError("no HIP device: the product has no CPU path");
  LIO_HIP(hipStreamCreate(&stream_));
  LIO_HIP(hipStreamCreateWithFlags(&stream2_, hipStreamNonBlocking));
  LIO_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
  LIO_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
  LIO_HIP(hipEventCreateWithFlags(&ev_full_, hipEventDisableTiming));
  LIO_HIP(hipEventCreateWithFlags(&ev_full_read_, hipEventDisableTiming));
  for (ClassMap &m : cls_) {
    m.h_counters.alloc(1, hipHostMallocDefault, true);
    m.counters.reserve(1);
    m.cube_bounds.reserve(LIO_MAP_MAX_VALID * 6);
  }
  sur_count_.reserve(1); sur_desc_.reserve(1);
  h_sur_count_.alloc(1, hipHostMallocDefault, true);
  h_sur_desc_.alloc(1, hipHostMallocDefault, true);
  prepare_seg_sort_kernels();
}

MappingDev::~MappingDev() {
  if (ev_fork_) (void)hipEventDestroy(ev_fork_);
  if (ev_join_) (void)hipEventDestroy(ev_join_);
  if (ev_full_) (void)hipEventDestroy(ev_full_);
  if (ev_full_read_) (void)hipEventDestroy(ev_full_read_);
  if (stream2_) (void)hipStreamDestroy(stream2_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

// cen_ moves by one per cube the window shifts (StepWindow), without bound; the keys keep ten bits per axis
bool MappingDev::CenFits(const int cen[3]) {
  const int dims[3] = {L, Wd, H};
  for (int d = 0; d < 3; ++d)
    if (-cen[d] < kCubeOffsetMin || dims[d] - 1 - cen[d] > kCubeOffsetMax) return false;
  return true;
}

MapValidSet MappingDev::MakeValidSet(const uint32_t *valid_idx, size_t n, const int cen_of_idx[3]) const {
  if (!CenFits(cen_)) throw CapacityError("PointMapping: the cube window lies beyond the range of the packed cube keys");
  MapValidSet vs;
  std::memset(&vs, 0, sizeof(vs));
  const int dims[3] = {L, Wd, H};
  for (int d = 0; d < 3; ++d) { vs.lo[d] = -cen_[d]; vs.hi[d] = dims[d] - cen_[d]; }
  std::vector<uint32_t> keys;
  for (size_t k = 0; k < n; ++k) {
    // FromIndex (PointMapping.h:153-160), re-based on the current centre (:1165-1179)
    const int residual = int(valid_idx[k] % uint32_t(L * Wd));
    const int ck = int(valid_idx[k] / uint32_t(L * Wd)), cj = residual / L, ci = residual % L;
    const int a[3] = {ci - cen_of_idx[0], cj - cen_of_idx[1], ck - cen_of_idx[2]};
    bool inside = true;
    for (int d = 0; d < 3; ++d) inside = inside && a[d] >= vs.lo[d] && a[d] < vs.hi[d];
    if (inside) keys.push_back(pack_cube(a[0], a[1], a[2]));
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  if (keys.size() > LIO_MAP_MAX_VALID) throw CapacityError("PointMapping: more than 125 valid cubes");
  vs.n = int(keys.size());
  for (int k = 0; k < vs.n; ++k) vs.key[k] = keys[k];
  return vs;
}

bool MappingDev::LayoutMatches(const ClassMap &m, const MapValidSet &vs) const {
  if (!m.layout_ok || int(m.layout_keys.size()) != vs.n) return false;
  for (int d = 0; d < 3; ++d) if (m.layout_lo[d] != vs.lo[d] || m.layout_hi[d] != vs.hi[d]) return false;
  return std::equal(m.layout_keys.begin(), m.layout_keys.end(), vs.key);
}

void MappingDev::LayoutLaunch(ClassMap &m, const MapValidSet &vs) {
  hipStream_t s = stream_;
  std::memset(m.h_counters.p, 0, sizeof(MapCounters));
  if (m.n == 0) return;
  const size_t n = m.n;
  const int ni = int(n);
  m.rk.reserve(n); m.rk2.reserve(n); m.vals.reserve(n); m.vals2.reserve(n);
  m.pool2.reserve(n); m.pkey2.reserve(n); m.vrank.reserve(n);
  LIO_HIP(hipMemsetAsync(m.counters.p, 0, sizeof(MapCounters), s));
  hipLaunchKernelGGL(k_map_rank, dim3(cdiv(ni, 256)), dim3(256), 0, s, m.pkey.p, ni, vs, m.rk.p, m.vals.p, m.counters.p);
  size_t tb = 0;
  LIO_HIP(rocprim::radix_sort_pairs(nullptr, tb, m.rk.p, m.rk2.p, m.vals.p, m.vals2.p, n, 0, 8, s));
  m.tmp.reserve(tb + 256);
  LIO_HIP(rocprim::radix_sort_pairs(m.tmp.p, tb, m.rk.p, m.rk2.p, m.vals.p, m.vals2.p, n, 0, 8, s));
  hipLaunchKernelGGL(k_map_gather, dim3(cdiv(ni, 256)), dim3(256), 0, s, m.pool.p, m.pkey.p, m.rk2.p, m.vals2.p, ni, m.counters.p, m.pool2.p,
                     m.pkey2.p, m.vrank.p);
  LIO_HIP(hipGetLastError());
  LIO_HIP(hipMemcpyAsync(m.h_counters.p, m.counters.p, sizeof(MapCounters), hipMemcpyDeviceToHost, s));
}

void MappingDev::LayoutFinish(ClassMap &m, const MapValidSet &vs) {
  if (m.n != 0) {
    std::swap(m.pool, m.pool2);
    std::swap(m.pkey, m.pkey2);
  }
  m.n_valid = size_t(m.h_counters.p->n_valid);
  m.n_rest = size_t(m.h_counters.p->n_rest);
  m.n = m.n_valid + m.n_rest;
  m.layout_ok = true;
  m.layout_keys.assign(vs.key, vs.key + vs.n);
  for (int d = 0; d < 3; ++d) { m.layout_lo[d] = vs.lo[d]; m.layout_hi[d] = vs.hi[d]; }
}

// pool must already be laid out for vs.  new_sensor_pts: device, sensor frame.
void MappingDev::UpdateLaunch(ClassMap &m, const float4 *new_sensor_pts, size_t n_new, const MapValidSet &vs, const Rigid<float> &T, float leaf) {
  hipStream_t s = stream_;
  std::memset(m.h_counters.p, 0, sizeof(MapCounters));
  const size_t nV = m.n_valid, nU = nV + n_new;
  m.h_counters.p->n_out = int(nV);
  if (nU == 0) return;
  m.pool.reserve(m.n_rest + n_new + nU, s, true, m.n);
  m.pkey.reserve(m.n_rest + n_new + nU, s, true, m.n);
  m.u_pts.reserve(nU); m.u_rank.reserve(nU); m.k64.reserve(nU); m.k64b.reserve(nU); m.flags.reserve(nU); m.pos.reserve(nU);
  m.vals.reserve(nU); m.vals2.reserve(nU); m.vrank.reserve(nU, s, true, nV);
  LIO_HIP(hipMemsetAsync(m.counters.p, 0, sizeof(MapCounters), s));
  if (nV) {
    LIO_HIP(hipMemcpyAsync(m.u_pts.p, m.pool.p + m.n_rest, nV * sizeof(float4), hipMemcpyDeviceToDevice, s));
    LIO_HIP(hipMemcpyAsync(m.u_rank.p, m.vrank.p, nV * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  }
  if (n_new) {
    const int nn = int(n_new);
    m.new_pts.reserve(n_new); m.new_key.reserve(n_new); m.rk.reserve(n_new); m.rk2.reserve(n_new);
    hipLaunchKernelGGL(k_map_new, dim3(cdiv(nn, 256)), dim3(256), 0, s, new_sensor_pts, nn, T.rot, T.pos, cen_[0], cen_[1], cen_[2], vs, m.new_pts.p,
                       m.new_key.p, m.rk.p, m.vals.p, m.counters.p);
    size_t tb = 0;
    LIO_HIP(rocprim::radix_sort_pairs(nullptr, tb, m.rk.p, m.rk2.p, m.vals.p, m.vals2.p, n_new, 0, 8, s));
    m.tmp.reserve(tb + 256);
    LIO_HIP(rocprim::radix_sort_pairs(m.tmp.p, tb, m.rk.p, m.rk2.p, m.vals.p, m.vals2.p, n_new, 0, 8, s));
    hipLaunchKernelGGL(k_new_scatter, dim3(cdiv(nn, 256)), dim3(256), 0, s, m.new_pts.p, m.new_key.p, m.rk2.p, m.vals2.p, nn, m.counters.p, int(nV),
                       int(m.n_rest), m.u_pts.p, m.u_rank.p, m.pool.p, m.pkey.p);
  }
  const int nu = int(nU);
  const float inv_leaf = 1.0f / leaf;
  hipLaunchKernelGGL(k_cube_bounds_init, dim3(cdiv(LIO_MAP_MAX_VALID * 6, 256)), dim3(256), 0, s, m.cube_bounds.p);
  hipLaunchKernelGGL(k_cube_bounds, dim3(cdiv(nu, 256)), dim3(256), 0, s, m.u_pts.p, m.u_rank.p, nu, m.cube_bounds.p);
  hipLaunchKernelGGL(k_cube_vox_keys, dim3(cdiv(nu, 256)), dim3(256), 0, s, m.u_pts.p, m.u_rank.p, nu, m.cube_bounds.p, inv_leaf,
                     reinterpret_cast<unsigned long long *>(m.k64.p), m.vals.p);
  size_t tb2 = 0, tb3 = 0;
  LIO_HIP(rocprim::radix_sort_pairs(nullptr, tb2, m.k64.p, m.k64b.p, m.vals.p, m.vals2.p, nU, 0, 40, s));
  LIO_HIP(rocprim::exclusive_scan(nullptr, tb3, m.flags.p, m.pos.p, 0, nU, rocprim::plus<int>(), s));
  m.tmp.reserve(std::max(tb2, tb3) + 256);
  LIO_HIP(rocprim::radix_sort_pairs(m.tmp.p, tb2, m.k64.p, m.k64b.p, m.vals.p, m.vals2.p, nU, 0, 40, s));
  hipLaunchKernelGGL(k_heads64, dim3(cdiv(nu, 256)), dim3(256), 0, s, reinterpret_cast<unsigned long long *>(m.k64b.p), nu, m.flags.p);
  LIO_HIP(rocprim::exclusive_scan(m.tmp.p, tb3, m.flags.p, m.pos.p, 0, nU, rocprim::plus<int>(), s));
  hipLaunchKernelGGL(k_cube_centroids, dim3(cdiv(nu, 256)), dim3(256), 0, s, m.u_pts.p, reinterpret_cast<unsigned long long *>(m.k64b.p), m.vals2.p,
                     m.flags.p, m.pos.p, nu, vs, int(m.n_rest), m.counters.p, m.pool.p, m.pkey.p, m.vrank.p);
  LIO_HIP(hipGetLastError());
  LIO_HIP(hipMemcpyAsync(m.h_counters.p, m.counters.p, sizeof(MapCounters), hipMemcpyDeviceToHost, s));
}

void MappingDev::UpdateFinish(ClassMap &m) {
  m.n_rest += size_t(m.h_counters.p->n_new_rest);
  m.n_valid = size_t(m.h_counters.p->n_out);
  m.n = m.n_rest + m.n_valid;
}

// laser_cloud_*_from_map_ stay what the last Process selected until the next Process (GetCloud).  They lie in the pool's valid tail or, after
// that Process's own update, at the head of the work list; an update from outside a Process rewrites both, so its first one copies them out.
void MappingDev::KeepFromMap() {
  if (from_map_kept_) return;
  for (int c = 0; c < 2; ++c) {
    const size_t n = n_from_map_[c];
    if (!n) continue;
    const ClassMap &m = cls_[c];
    from_map_keep_[c].reserve(n);
    LIO_HIP(hipMemcpyAsync(from_map_keep_[c].p, from_map_in_u_ ? m.u_pts.p : m.pool.p + m.n_rest, n * sizeof(float4), hipMemcpyDeviceToDevice, stream_));
  }
  from_map_kept_ = true;
}

void MappingDev::UpdateMapDatabase(const float *corner_ds, size_t n_corner, const float *surf_ds, size_t n_surf, const uint32_t *valid_idx,
                                   size_t n_valid, const Rigid<float> &T, const int cube_center[3]) {
  (void)MakeValidSet(valid_idx, n_valid, cube_center);   // a list or a window the keys cannot hold is refused before the first copy
  const float *src[2] = {corner_ds, surf_ds};
  const size_t cnt[2] = {n_corner, n_surf};
  for (int c = 0; c < 2; ++c) {
    if (!cnt[c]) continue;
    cls_[c].in.reserve(cnt[c]);
    LIO_HIP(hipMemcpyAsync(cls_[c].in.p, src[c], cnt[c] * sizeof(float4), hipMemcpyHostToDevice, stream_));
  }
  UpdateMapDatabase(cls_[0].in.p, n_corner, cls_[1].in.p, n_surf, valid_idx, n_valid, T, cube_center, nullptr);
}

void MappingDev::UpdateMapDatabase(const float4 *d_corner_ds, size_t n_corner, const float4 *d_surf_ds, size_t n_surf, const uint32_t *valid_idx,
                                   size_t n_valid, const Rigid<float> &T, const int cube_center[3], hipStream_t producer) {
  hipStream_t s = stream_;
  if (producer && producer != s) {
    LIO_HIP(hipEventRecord(ev_fork_, producer));
    LIO_HIP(hipStreamWaitEvent(s, ev_fork_, 0));
  }
  const MapValidSet vs = MakeValidSet(valid_idx, n_valid, cube_center);   // (throws before anything of the handle has changed)
  KeepFromMap();
  bool relayout[2];
  for (int c = 0; c < 2; ++c) {
    relayout[c] = !LayoutMatches(cls_[c], vs);
    if (relayout[c]) LayoutLaunch(cls_[c], vs);
  }
  if (relayout[0] || relayout[1]) LIO_HIP(hipStreamSynchronize(s));
  for (int c = 0; c < 2; ++c) if (relayout[c]) LayoutFinish(cls_[c], vs);
  const float4 *src[2] = {d_corner_ds, d_surf_ds};
  const size_t cnt[2] = {n_corner, n_surf};
  const float leaf[2] = {cfg_.corner_filter_size, cfg_.surf_filter_size};
  for (int c = 0; c < 2; ++c) UpdateLaunch(cls_[c], src[c], cnt[c], vs, T, leaf[c]);
  LIO_HIP(hipStreamSynchronize(s));
  for (int c = 0; c < 2; ++c) UpdateFinish(cls_[c]);
}

// PointMapping.cc:1223-1234
size_t MappingDev::GetSurround(float leaf, float *out) {
  hipStream_t s = stream_;
  if (surround_idx_.empty()) return 0;   // before the first Process
  const size_t n_c = cls_[0].n, n_s = cls_[1].n, n = n_c + n_s;
  if (n == 0) return 0;
  if (n > size_t(INT_MAX)) throw std::runtime_error("PointMapping: map pools beyond 2^31 points");
  MapSurroundSet ss;
  std::memset(&ss, 0, sizeof(ss));
  {
    std::vector<uint32_t> keys;
    for (uint32_t idx : surround_idx_) {   // FromIndex (PointMapping.h:153-160); cen_ only moves in Process, which also rewrites the list
      const int residual = int(idx % uint32_t(L * Wd));
      const int ck = int(idx / uint32_t(L * Wd)), cj = residual / L, ci = residual % L;
      keys.push_back(pack_cube(ci - cen_[0], cj - cen_[1], ck - cen_[2]));
    }
    std::sort(keys.begin(), keys.end());   // (the list is i-major already: ascending keys)
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (keys.size() > LIO_MAP_MAX_VALID) throw std::runtime_error("PointMapping: more than 125 surround cubes");
    ss.n = int(keys.size());
    for (int k = 0; k < ss.n; ++k) ss.key[k] = keys[size_t(k)];
  }
  const int nc = int(n_c), ns = int(n_s), ni = int(n);
  SegDesc desc{0, ni, 0};
  const SegSortPlan plan = seg_sort_plan(&desc, 1, 8);
  *h_sur_desc_.p = desc;
  sur_bin_.reserve(n); sur_bin2_.reserve(n); sur_src_.reserve(n); sur_hist_.reserve(std::max<size_t>(plan.hist_entries, 1)); sur_cloud_.reserve(n);
  LIO_HIP(hipMemcpyAsync(sur_desc_.p, h_sur_desc_.p, sizeof(SegDesc), hipMemcpyHostToDevice, s));
  LIO_HIP(hipMemsetAsync(sur_count_.p, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_surround_bins, dim3(cdiv(ni, 256)), dim3(256), 0, s, cls_[0].pkey.p, nc, cls_[1].pkey.p, ns, ss, sur_bin_.p, sur_count_.p);
  // a stable multi-split into <= 250 bins IS one 8-bit pass of the segmented sort over one segment (values: the points' positions)
  const SegSortPair sorted = seg_sort_passes(sur_desc_.p, 1, plan, sur_bin_.p, nullptr, {sur_bin2_.p, sur_src_.p}, {sur_bin_.p, sur_src_.p}, sur_hist_.p, 8, 1, nullptr, s);
  hipLaunchKernelGGL(k_surround_gather, dim3(cdiv(ni, 256)), dim3(256), 0, s, cls_[0].pool.p, nc, cls_[1].pool.p, ns, sorted.keys, sorted.vals, sur_cloud_.p);
  LIO_HIP(hipGetLastError());
  LIO_HIP(hipMemcpyAsync(h_sur_count_.p, sur_count_.p, sizeof(int), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));   // the one wait of the assembly: the VoxelGrid is launched over the kept points
  const size_t n_kept = size_t(*h_sur_count_.p);
  if (n_kept == 0) return 0;
  const size_t m = sur_vox_.run(sur_cloud_.p, n_kept, leaf, sur_out_, s);
  if (out && m) {
    LIO_HIP(hipMemcpyAsync(out, sur_out_.p, m * sizeof(float4), hipMemcpyDeviceToHost, s));
    LIO_HIP(hipStreamSynchronize(s));
  }
  return m;
}

void MappingDev::FullBegin(size_t n) {
  n_full_ = n; full_mapped_ = false; full_event_ = false;
  if (n) full_.reserve(n);
}
float4 *MappingDev::FullTake(size_t n, hipStream_t writer) {
  FullBegin(n);
  if (!n) return nullptr;
  if (full_read_) LIO_HIP(hipStreamWaitEvent(writer, ev_full_read_, 0));
  return full_.p;
}
void MappingDev::SetFullCloud(const float *xyzi, size_t n) {
  float4 *dst = FullTake(n, stream_);
  if (!dst) return;
  LIO_HIP(hipMemcpyAsync(dst, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, stream_));
  LIO_HIP(hipStreamSynchronize(stream_));   // the caller may reuse the source right after the call
}
// a reader of FullDevice() on another stream is ordered behind the registration: no host wait
void MappingDev::FullWaitOn(hipStream_t consumer) {
  if (full_event_) LIO_HIP(hipStreamWaitEvent(consumer, ev_full_, 0));
}
// ... and the next writer of the buffers behind that reader's copy
void MappingDev::FullReadBy(hipStream_t consumer) {
  LIO_HIP(hipEventRecord(ev_full_read_, consumer));
  full_read_ = true;
}
size_t MappingDev::GetFullCloud(float *out) {
  if (out && n_full_) {
    LIO_HIP(hipMemcpyAsync(out, full_.p, n_full_ * sizeof(float4), hipMemcpyDeviceToHost, stream_));
    LIO_HIP(hipStreamSynchronize(stream_));
  }
  return n_full_;
}

// ------------------------------------------------------------------------------------------------
// One step of a handle is a chain of one: the only route through the file
void MappingDev::Process(const float *corner_last, size_t n_corner, const float *surf_last, size_t n_surf, const Rigid<float> &sum) {
  MappingDev *self = this;
  const OdomSweep sweep{CloudSrc::host(corner_last, n_corner), CloudSrc::host(surf_last, n_surf), sum, MapFullSource{}};
  ProcessBatch(&self, 1, &sweep);
}

// ---- what a step does on the handle alone, called by the chain's steps below
void MappingDev::StepBegin(const Rigid<float> &sum, Step &st) {
  transform_sum_ = sum;
  score_ready_ = false;
  iterations_ = 0; num_selected_ = 0; degenerate_ = false; kz_ = 0;
  st.T0 = AssociatedPose(sum);
  if (cfg_.map_builder && !system_init_) {  // MapBuilder::ProcessMap (MapBuilder.cc:227-232)
    system_init_ = true;
    transform_bef_mapped_ = transform_aft_mapped_ = transform_sum_;
  }
  transform_tobe_mapped_ = st.T0;
}

Rigid<float> MappingDev::AssociatedPose(const Rigid<float> &sum) const {
  const bool builder = cfg_.map_builder != 0;
  Rigid<float> bef = transform_bef_mapped_, tobe = transform_tobe_mapped_;
  if (builder && !system_init_) bef = tobe = sum;  // MapBuilder::ProcessMap (MapBuilder.cc:227-232)
  if (builder || !imu_inited_) {  // TransformAssociateToMap (:755-758) / Transform4DAssociateToMap (MapBuilder.cc:55-75)
    const Rigid<float> sumT = fromAffine(linearOf(sum), sum.pos);
    const Rigid<float> incre = compose(rinverse(bef), sumT);
    const Rigid<float> full = compose(tobe, incre);
    if (builder && cfg_.enable_4d) {
      // keep the odometry's roll/pitch, take only the yaw of the increment
      const Vec3<double> r0 = r2ypr_deg(to_double(toRot(normalized(full.rot))));
      const Vec3<double> r00 = r2ypr_deg(to_double(toRot(normalized(sum.rot))));
      const float y = float(double(float(r0.x - r00.x)) / 180.0 * M_PI);
      Mat3<float> Rz = Mat3<float>::identity();
      Rz(0, 0) = std::cos(y); Rz(0, 1) = -std::sin(y); Rz(1, 0) = std::sin(y); Rz(1, 1) = std::cos(y);
      tobe.pos = full.pos;
      tobe.rot = fromRot(Rz * toRot(normalized(sum.rot)));
    } else {
      tobe = full;
    }
  }
  return tobe;
}

// sensor cube and window shift (:808-925); absolute keys make the shift a change of the centre only
void MappingDev::WindowAt(const Rigid<float> &T0, int cen[3], int cc[3]) const {
  const float posv[3] = {T0.pos.x, T0.pos.y, T0.pos.z};
  const int dims[3] = {L, Wd, H};
  for (int d = 0; d < 3; ++d) {
    cen[d] = cen_[d];
    cc[d] = cube_coord(posv[d], cen[d]);
    while (cc[d] < 3) { ++cc[d]; ++cen[d]; }
    while (cc[d] >= dims[d] - 3) { --cc[d]; --cen[d]; }
  }
}

void MappingDev::StepWindow(Step &st) {
  const Rigid<float> &T0 = st.T0;
  point_on_z_axis(T0, pz_);
  const float posv[3] = {T0.pos.x, T0.pos.y, T0.pos.z};
  int cc[3], cen[3];
  WindowAt(T0, cen, cc);
  for (int d = 0; d < 3; ++d) cen_[d] = cen[d];
  // cubes of the 5x5x5 neighbourhood with a corner inside the +-60 deg cone (:938-989)
  valid_idx_.clear();
  surround_idx_.clear();
  auto sqdiff = [](const float a[3], const float b[3]) {
    float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return dx * dx + dy * dy + dz * dz;
  };
  for (int i = cc[0] - 2; i <= cc[0] + 2; ++i)
    for (int j = cc[1] - 2; j <= cc[1] + 2; ++j)
      for (int k = cc[2] - 2; k <= cc[2] + 2; ++k) {
        if (!(i >= 0 && i < L && j >= 0 && j < Wd && k >= 0 && k < H)) continue;
        const float cx = 50.0f * (i - cen_[0]), cy = 50.0f * (j - cen_[1]), cz = 50.0f * (k - cen_[2]);
        bool fov = false;
        for (int ii = -1; ii <= 1; ii += 2)
          for (int jj = -1; jj <= 1; jj += 2)
            for (int kk = -1; kk <= 1; kk += 2) {
              const float corner[3] = {cx + 25.0f * ii, cy + 25.0f * jj, cz + 25.0f * kk};
              const float s1 = sqdiff(posv, corner), s2 = sqdiff(pz_, corner);
              const float check1 = 100.0f + s1 - s2 - 10.0f * std::sqrt(3.0f) * std::sqrt(s1);
              const float check2 = 100.0f + s1 - s2 + 10.0f * std::sqrt(3.0f) * std::sqrt(s1);
              if (check1 < 0 && check2 > 0) fov = true;
            }
        if (fov) valid_idx_.push_back(uint32_t(i + L * j + L * Wd * k));
        surround_idx_.push_back(uint32_t(i + L * j + L * Wd * k));   // :984
      }
  st.vs = MakeValidSet(valid_idx_.data(), valid_idx_.size(), cen_);

  // laser_cloud_*_from_map_ = tail of the pool after the layout pass
  for (int c = 0; c < 2; ++c) {
    st.relayout[c] = !LayoutMatches(cls_[c], st.vs);
    if (st.relayout[c]) LayoutLaunch(cls_[c], st.vs);
  }
}

// VoxelGrid of the stacks (:1005-1015)
void MappingDev::StepFilterLaunch(const Step &st) {
  hipStream_t s = stream_;
  const float leaf[2] = {cfg_.corner_filter_size, cfg_.surf_filter_size};
  // the two filters are independent: the surf one goes to a second stream, forked after the round trip of the stacks
  LIO_HIP(hipEventRecord(ev_fork_, s));
  LIO_HIP(hipStreamWaitEvent(stream2_, ev_fork_, 0));
  hipStream_t vs_stream[2] = {s, stream2_};
  for (int c = 0; c < 2; ++c) cls_[c].vox.launch(cls_[c].stack_raw.p, st.cnt[c], leaf[c], cls_[c].stack_ds, vs_stream[c]);
  // finish() only waits for the output COUNT (posted to the host's mailbox); the consumers on `s` wait for the surf filter's
  // stream through an event
  LIO_HIP(hipEventRecord(ev_join_, stream2_));
  LIO_HIP(hipStreamWaitEvent(s, ev_join_, 0));
}
// TransformUpdate (:760-763)
void MappingDev::TransformUpdate() {
  transform_bef_mapped_ = transform_sum_;
  transform_aft_mapped_ = transform_tobe_mapped_;
}

// MapBuilder.cc:527-558: optimise every skip_count-th call, always update the map
bool MappingDev::StepOptimizes() {
  if (!cfg_.map_builder) return true;
  const bool optimise = odom_count_ % cfg_.skip_count == 0;
  if (!optimise) {
    n_from_map_[0] = cls_[0].n_valid; n_from_map_[1] = cls_[1].n_valid; from_map_in_u_ = from_map_kept_ = false;
    TransformUpdate();
  }
  ++odom_count_;
  return optimise;
}

// the state the rounds ended with; M: the slots the score list's arrays hold
void MappingDev::OptimizeEnd(const OdomState &st, int M, bool four_dof) {
  transform_tobe_mapped_.rot = Quat<float>(st.T[3], st.T[0], st.T[1], st.T[2]);
  transform_tobe_mapped_.pos = Vec3<float>(st.T[4], st.T[5], st.T[6]);
  iterations_ = st.iters;
  num_selected_ = st.nsel;
  degenerate_ = st.degenerate != 0;
  kz_ = degenerate_ ? st.kz : 0;
  TransformUpdate();
  n_score_slots_ = size_t(M);
  score_ready_ = !four_dof;  // OptimizeMap keeps no score list
}

// PublishResults (:1105 -> :1244-1248): PointAssociateToMap on full_cloud_, in place
void MappingDev::StepRegisterFull() {
  if (imu_inited_ || !n_full_ || full_mapped_) return;
  hipStream_t s = stream_;
  const Rigid<float> &T = transform_tobe_mapped_;
  const float q[4] = {T.rot.x, T.rot.y, T.rot.z, T.rot.w}, p[3] = {T.pos.x, T.pos.y, T.pos.z};
  std::swap(full_, full_in_);
  full_.reserve(n_full_);
  if (full_read_) LIO_HIP(hipStreamWaitEvent(s, ev_full_read_, 0));
  launch_rigid_map(full_in_.p, int(n_full_), q, p, full_.p, s);
  LIO_HIP(hipEventRecord(ev_full_, s));
  full_mapped_ = true; full_event_ = true;
}

MapChain &MappingDev::Chain() {
  if (!chain_) chain_.reset(new MapChain);
  return *chain_;
}

// ------------------------------------------------------------------------------------------------
// include/lio_map_batch.h.  Every step of the chain runs for all handles before the next one starts, so a wait is one pass over the handles
// instead of one stop per handle.  Every handle is idle when the call starts (each lio_map_* call returns synchronised).

// ---- 1. prepare: association, uploads, cube bookkeeping and the layout pass per handle, no wait in between; one launch for every round trip.
// Fed from the device: no staging buffer, no upload and no event per handle — the sources are complete; the one launch reads the stack
// clouds where they lie and takes every handle's full cloud beside them.
void MapChain::Prepare(MappingDev *const *handles, int n_handles, const OdomSweep *sweep) {
  m = handles; n = n_handles; s0 = m[0]->stream_;
  const bool on_device = clouds_on_device(size_t(2) * size_t(n), [&](size_t i) { return i & 1 ? sweep[i / 2].surf : sweep[i / 2].corner; });
  steps.assign(size_t(n), MappingDev::Step());
  h_stack.assign(on_device ? 0 : size_t(n), MbStackRec());
  h_from.assign(on_device ? size_t(n) : 0, MbFromOdomRec());
  size_t max_in = 0;
  for (int k = 0; k < n; ++k) {
    MappingDev &d = *m[k];
    MappingDev::Step &st = steps[size_t(k)];
    const OdomSweep &sw = sweep[k];
    d.StepBegin(sw.transform_sum, st);
    // the stack clouds go up while the host does the cube bookkeeping; stack_raw is sized for their round trip
    const CloudSrc src[2] = {sw.corner, sw.surf};
    st.cnt[0] = sw.corner.n; st.cnt[1] = sw.surf.n;
    MbStackRec &r = on_device ? h_from[size_t(k)].stack : h_stack[size_t(k)];
    for (int c = 0; c < 2; ++c) {
      MappingDev::ClassMap &cm = d.cls_[c];
      cm.n_stack = 0;
      if (st.cnt[c] && !on_device) cm.in.reserve(st.cnt[c]);
      if (st.cnt[c]) cm.stack_raw.reserve(st.cnt[c]);
      if (st.cnt[c] && !on_device) LIO_HIP(hipMemcpyAsync(cm.in.p, src[c].p, st.cnt[c] * sizeof(float4), src[c].to_device(), d.stream_));
      r.in[c] = on_device ? src[c].p : cm.in.p; r.out[c] = cm.stack_raw.p; r.n[c] = int(st.cnt[c]);
      max_in = std::max(max_in, st.cnt[c]);
    }
    r.q = st.T0.rot; r.t = st.T0.pos;
    if (!on_device && k && (st.cnt[0] || st.cnt[1])) {   // the round trip on s0 reads what this stream uploads
      LIO_HIP(hipEventRecord(d.ev_join_, d.stream_));
      LIO_HIP(hipStreamWaitEvent(s0, d.ev_join_, 0));
    }
    if (on_device && sw.full.set) {   // SetFullCloud, the points written by the launch below
      const MapFullSource &f = sw.full;
      d.FullBegin(f.n);
      if (f.n) {
        if (d.full_read_) LIO_HIP(hipStreamWaitEvent(s0, d.ev_full_read_, 0));
        h_from[size_t(k)].full = FullTake{f.pts, d.full_.p, int(f.n), f.to_end};
        max_in = std::max(max_in, f.n);
      }
    }
    d.StepWindow(st);
  }
  // the filters (Filter) and the full clouds' registration (Update) run on the handles' own streams: those wait for `ev` in Filter
  any_stack = max_in != 0;
  if (any_stack) {
    if (on_device) {
      d_from.reserve(size_t(n));
      LIO_HIP(hipMemcpyAsync(d_from.p, h_from.data(), size_t(n) * sizeof(MbFromOdomRec), hipMemcpyHostToDevice, s0));
      hipLaunchKernelGGL(k_mb_from_odom, dim3(cdiv(max_in, 256), 3, n), dim3(256), 0, s0, d_from.p);
    } else {
      d_stack.reserve(size_t(n));
      LIO_HIP(hipMemcpyAsync(d_stack.p, h_stack.data(), size_t(n) * sizeof(MbStackRec), hipMemcpyHostToDevice, s0));
      hipLaunchKernelGGL(k_mb_roundtrip, dim3(cdiv(max_in, 256), 2, n), dim3(256), 0, s0, d_stack.p);
    }
    LIO_HIP(hipGetLastError());
    if (n > 1) LIO_HIP(hipEventRecord(ev, s0));
  }
  for (int k = 0; k < n; ++k) {   // one pass of waits over the handles that re-laid out
    MappingDev &d = *m[k];
    const MappingDev::Step &st = steps[size_t(k)];
    if (st.relayout[0] || st.relayout[1]) LIO_HIP(hipStreamSynchronize(d.stream_));
    for (int c = 0; c < 2; ++c) if (st.relayout[c]) d.LayoutFinish(d.cls_[c], st.vs);
  }
}

// ---- 2. filter: every handle's two VoxelGrids in flight before the first count is waited for
void MapChain::Filter() {
  for (int k = 0; k < n; ++k) {
    MappingDev &d = *m[k];
    if (k && any_stack) LIO_HIP(hipStreamWaitEvent(d.stream_, ev, 0));
    d.StepFilterLaunch(steps[size_t(k)]);
  }
  for (int k = 0; k < n; ++k)
    for (MappingDev::ClassMap &cm : m[k]->cls_) cm.n_stack = cm.vox.finish();
}

// ---- 3. who iterates (`act`); the bounds of their from-map clouds in two launches, one copy back, one wait; their grids on their own streams
void MapChain::MakeGrids() {
  act.clear();
  for (int k = 0; k < n; ++k) {
    MappingDev &d = *m[k];
    if (!d.StepOptimizes()) continue;   // a skipped MapBuilder call
    d.n_from_map_[0] = d.cls_[0].n_valid; d.n_from_map_[1] = d.cls_[1].n_valid;
    d.from_map_in_u_ = d.from_map_kept_ = false;
    if (!(d.cls_[0].n_valid > 10 && d.cls_[1].n_valid > 100)) continue;   // :327-329 (no TransformUpdate either)
    if (d.cls_[0].n_stack + d.cls_[1].n_stack == 0) {   // every round has < 50 rows: the loop runs dry, then TransformUpdate
      d.iterations_ = d.cfg_.num_max_iterations;
      d.TransformUpdate();
      continue;
    }
    act.push_back(k);
  }
  const int na = nA();
  if (!na) return;
  clouds.begin(0, 2 * na);
  for (int j = 0; j < na; ++j)
    for (int c = 0; c < 2; ++c) {
      const MappingDev::ClassMap &cm = dev(j).cls_[c];
      if (cm.n_valid > size_t(INT_MAX) - 255) throw CapacityError("lio_map_process_batch: a from-map cloud exceeds 2^31 points");
      clouds.add(cm.pool.p + cm.n_rest, int(cm.n_valid));
    }
  const VoxParams *bounds = clouds.bounds(s0);
  const float cell = scan_to_map_cell_edge(m[0]->cfg_.min_match_sq_dis);
  for (int j = 0; j < na; ++j)
    for (int c = 0; c < 2; ++c) {
      MappingDev::ClassMap &cm = dev(j).cls_[c];
      const VoxParams &b = bounds[2 * j + c];
      cm.grid.build(cm.pool.p + cm.n_rest, cm.n_valid, b.mn, b.mx, cell, dev(j).stream_);
    }
}

// ---- 4. the keyframe table of cloud_kernels.h over `act`: every sensor's two grids, its whole stack as one keyframe, its starting state, and
// where its slice of the chain's arrays lies in the handle — one upload; then the filtered stacks into the chain's stack_all
void MapChain::FillTable() {
  const int na = nA();
  size_t slots = 0, part_total = 0;
  max_Mc = max_Ms = max_nb = 0;
  auto up8 = [](size_t b) { return (b + 7) & ~size_t(7); };
  off_kd = size_t(na) * sizeof(KfMapDesc);
  off_st = off_kd + up8(size_t(na) * sizeof(KfDesc));
  off_sl = off_st + up8(size_t(na) * sizeof(OdomState));
  const size_t table_bytes = off_sl + size_t(na) * sizeof(MbSliceRec);
  if (h_table.n < table_bytes) h_table.alloc(table_bytes + table_bytes / 2, hipHostMallocDefault);
  d_table.reserve(table_bytes);
  KfMapDesc *h_md = reinterpret_cast<KfMapDesc *>(h_table.p);
  KfDesc *h_kd = reinterpret_cast<KfDesc *>(h_table.p + off_kd);
  OdomState *h_st = reinterpret_cast<OdomState *>(h_table.p + off_st);
  MbSliceRec *h_sl = reinterpret_cast<MbSliceRec *>(h_table.p + off_sl);
  for (int j = 0; j < na; ++j) {
    MappingDev &d = dev(j);
    MappingDev::ClassMap &mc = d.cls_[0], &ms = d.cls_[1];
    if (mc.n_stack + ms.n_stack + slots > size_t(INT_MAX) - 255) throw CapacityError("lio_map_process_batch: the filtered stacks exceed 2^31 points");
    const int Mc = int(mc.n_stack), Ms = int(ms.n_stack), M = Mc + Ms;
    const int nb = odom_rows_blocks(M);
    h_md[j] = KfMapDesc{mc.grid.sorted(), mc.grid.cells(), mc.grid.desc(), ms.grid.sorted(), ms.grid.cells(), ms.grid.desc()};
    h_kd[j] = KfDesc{int(slots), Mc, Ms, j, nb, int(part_total), {d.pz_[0], d.pz_[1], d.pz_[2]}};
    h_st[j] = odom_state_at(d.transform_tobe_mapped_);
    d.stack_all_.reserve(size_t(M)); d.f_valid_.reserve(size_t(M)); d.f_coef_.reserve(size_t(M)); d.f_abs_.reserve(size_t(M));
    h_sl[j] = MbSliceRec{{mc.stack_ds.p, ms.stack_ds.p}, {Mc, Ms}, int(slots), d.stack_all_.p, d.f_coef_.p, d.f_abs_.p, d.f_valid_.p};
    slots += size_t(M); part_total += size_t(nb);
    max_Mc = std::max(max_Mc, Mc); max_Ms = std::max(max_Ms, Ms); max_nb = std::max(max_nb, nb);
    if (act[size_t(j)]) {   // s0 behind its filters (the surf one joined in) and its grids
      LIO_HIP(hipEventRecord(d.ev_join_, d.stream_));
      LIO_HIP(hipStreamWaitEvent(s0, d.ev_join_, 0));
    }
  }
  stack_all.reserve(slots); valid.reserve(slots); coef.reserve(slots); abs_coef.reserve(slots);
  partials.reserve(part_total * 28);
  LIO_HIP(hipMemcpyAsync(d_table.p, h_table.p, table_bytes, hipMemcpyHostToDevice, s0));
  const int max_M = std::max(max_Mc, max_Ms);   // (> 0: every sensor of the table has a stack)
  hipLaunchKernelGGL(k_mb_take, dim3(cdiv(max_M, 256), 2, na), dim3(256), 0, s0, reinterpret_cast<const MbSliceRec *>(d_table.p + off_sl), stack_all.p);
  LIO_HIP(hipGetLastError());
}

// ---- 5. the rounds (:325-753), three launches each over the whole table.  Convergence is read back behind rounds 6, 8 and 10 only: a peek costs
// a wait and a relaunch bubble (~35 us), a round that runs after convergence costs three no-op launches (~18 us), and the loop typically needs
// 5-7 rounds.  The last round before a peek posts every sensor's state to its own mailbox slot (dev.h: HostSignal); the peek ends the loop
// only when EVERY sensor has converged (one that converged earlier stays frozen: its blocks leave at once).  Leaves the last states in the mailbox.
void MapChain::Iterate() {
  const int na = nA();
  const lio_map_config &cfg = m[0]->cfg_;
  const bool four_dof = m[0]->FourDof();
  mail.reserve(na);
  const OdomState *h_st = reinterpret_cast<const OdomState *>(h_table.p + off_st);
  for (int j = 0; j < na; ++j) mail.slot(j) = h_st[j];   // (what the loop's end reads when no round runs)
  const KfMapDesc *d_md = reinterpret_cast<const KfMapDesc *>(d_table.p);
  const KfDesc *d_kd = reinterpret_cast<const KfDesc *>(d_table.p + off_kd);
  OdomState *d_st = reinterpret_cast<OdomState *>(d_table.p + off_st);
  const int mode = four_dof ? 2 : 1;
  const int max_it = cfg.num_max_iterations;
  static const int kPeek[] = {6, 8, 10};
  int iter = 0, peek_i = 0;
  bool done = false;
  while (iter < max_it && !done) {
    int until = max_it;
    while (peek_i < 3 && kPeek[peek_i] <= iter) ++peek_i;
    if (peek_i < 3) until = std::min(max_it, kPeek[peek_i]);
    for (; iter < until; ++iter) {
      // eight lanes per query; no processing order (every stack is one sweep's, a few thousand queries)
      launch_kf_round(d_kd, d_md, d_st, na, max_Mc, max_Ms, 8, stack_all.p, nullptr, cfg.min_match_sq_dis, cfg.min_plane_dis, mode, valid.p, coef.p, abs_coef.p, s0);
      launch_kf_rows(d_kd, d_st, na, max_nb, stack_all.p, valid.p, coef.p, partials.p, mode, s0);
      HostSignal sg{};
      if (iter == until - 1) sg = mail.arm(na);
      launch_kf_update(d_kd, d_st, na, partials.p, iter, 50, four_dof ? 1 : 0, nullptr, mail.base(), sg, s0);
    }
    mail.wait(s0);   // until > iter: the inner loop ran and its last round posted
    done = mail.all_converged(na);
  }
}

// ---- 6. give back: every sensor's slice of the chain's arrays into its handle (nobody waits for it before the call's last pass), the states
// from the mailbox
void MapChain::GiveBack() {
  const int na = nA();
  hipLaunchKernelGGL(k_mb_give, dim3(cdiv(max_Mc + max_Ms, 256), 4, na), dim3(256), 0, s0, reinterpret_cast<const MbSliceRec *>(d_table.p + off_sl), stack_all.p,
                     coef.p, abs_coef.p, valid.p);
  LIO_HIP(hipGetLastError());
  for (int j = 0; j < na; ++j) dev(j).OptimizeEnd(mail.slot(j), int(dev(j).cls_[0].n_stack + dev(j).cls_[1].n_stack), m[0]->FourDof());
}

// ---- 7. update: the map update and the full cloud's registration per handle on its own stream (the poses are on the host), then one pass of
// waits: the call returns synchronised
void MapChain::Update() {
  for (int k = 0; k < n; ++k) {
    MappingDev &d = *m[k];
    const float leaf[2] = {d.cfg_.corner_filter_size, d.cfg_.surf_filter_size};
    if (d.StepUpdates())
      for (int c = 0; c < 2; ++c) d.UpdateLaunch(d.cls_[c], d.cls_[c].stack_ds.p, d.cls_[c].n_stack, steps[size_t(k)].vs, d.transform_tobe_mapped_, leaf[c]);
    d.StepRegisterFull();
  }
  for (int k = 0; k < n; ++k) {
    MappingDev &d = *m[k];
    LIO_HIP(hipStreamSynchronize(d.stream_));
    if (!d.StepUpdates()) continue;
    for (int c = 0; c < 2; ++c) d.UpdateFinish(d.cls_[c]);
    d.from_map_in_u_ = true;
  }
}

void MappingDev::ProcessBatch(MappingDev *const *m, int n, const OdomSweep *sweep) {
  for (int k = 0; k < n; ++k)
    if (sweep[k].corner.n > size_t(INT_MAX) - 255 || sweep[k].surf.n > size_t(INT_MAX) - 255 || (sweep[k].full.set && sweep[k].full.n > size_t(INT_MAX) - 255))
      throw CapacityError("lio_map_process_batch: a cloud exceeds 2^31 points");
  // a pose whose window the packed cube keys cannot hold is refused before any handle changes and before the first launch
  for (int k = 0; k < n; ++k) {
    int cen[3], cc[3];
    m[k]->WindowAt(m[k]->AssociatedPose(sweep[k].transform_sum), cen, cc);
    if (!CenFits(cen)) throw CapacityError("lio_map_process_batch: a sensor's cube window lies beyond the range of the packed cube keys");
  }
  // the round launches carry these as launch parameters: without common values there is no common chain, a chain of one per handle
  for (int k = 1; k < n; ++k) {
    const lio_map_config &a = m[0]->cfg_, &b = m[k]->cfg_;
    if (a.min_match_sq_dis == b.min_match_sq_dis && a.min_plane_dis == b.min_plane_dis && a.num_max_iterations == b.num_max_iterations &&
        m[0]->FourDof() == m[k]->FourDof())
      continue;
    for (int j = 0; j < n; ++j) ProcessBatch(m + j, 1, sweep + j);
    return;
  }
  MapChain &ch = m[0]->Chain();
  ch.Prepare(m, n, sweep);
  ch.Filter();
  ch.MakeGrids();
  if (ch.nA()) {
    ch.FillTable();
    ch.Iterate();
    ch.GiveBack();
  }
  ch.Update();
}

// ------------------------------------------------------------------------------------------------
size_t MappingDev::GetCloud(int which, float *out) {
  hipStream_t s = stream_;
  const ClassMap &m = cls_[which & 1];
  const float4 *src = nullptr;
  size_t n = 0;
  if (which < 2) { src = m.stack_ds.p; n = m.n_stack; }
  else {
    n = n_from_map_[which & 1];
    src = from_map_kept_ ? from_map_keep_[which & 1].p : from_map_in_u_ ? m.u_pts.p : m.pool.p + m.n_rest;
  }
  if (out && n) {
    LIO_HIP(hipMemcpyAsync(out, src, n * sizeof(float4), hipMemcpyDeviceToHost, s));
    LIO_HIP(hipStreamSynchronize(s));
  }
  return n;
}

size_t MappingDev::GetCube(int cls, uint32_t cube_idx, float *out) {
  hipStream_t s = stream_;
  const ClassMap &m = cls_[cls];
  if (m.n == 0) return 0;
  const int residual = int(cube_idx % uint32_t(L * Wd));
  const int ck = int(cube_idx / uint32_t(L * Wd)), cj = residual / L, ci = residual % L;
  const uint32_t key = pack_cube(ci - cen_[0], cj - cen_[1], ck - cen_[2]);
  std::vector<uint32_t> keys(m.n);
  std::vector<float4> pts(m.n);
  LIO_HIP(hipMemcpyAsync(keys.data(), m.pkey.p, m.n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipMemcpyAsync(pts.data(), m.pool.p, m.n * sizeof(float4), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
  size_t cnt = 0;
  for (size_t i = 0; i < m.n; ++i)
    if (keys[i] == key) {
      if (out) std::memcpy(out + 4 * cnt, &pts[i], sizeof(float4));
      ++cnt;
    }
  return cnt;
}

// score_point_coeff_ (:725-750): surf selections of the last executed round, descending score
size_t MappingDev::GetScorePointCoeff(float *score, float *point, float *coeff) {
  if (!score_ready_) return 0;
  hipStream_t s = stream_;
  const size_t Mc = cls_[0].n_stack, Ms = cls_[1].n_stack;
  if (Ms == 0) return 0;
  std::vector<uint8_t> valid(Ms);
  std::vector<float4> coef(Ms), absc(Ms), pts(Ms);
  LIO_HIP(hipMemcpyAsync(valid.data(), f_valid_.p + Mc, Ms, hipMemcpyDeviceToHost, s));
  LIO_HIP(hipMemcpyAsync(coef.data(), f_coef_.p + Mc, Ms * sizeof(float4), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipMemcpyAsync(absc.data(), f_abs_.p + Mc, Ms * sizeof(float4), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipMemcpyAsync(pts.data(), stack_all_.p + Mc, Ms * sizeof(float4), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
  struct E { float sc; uint32_t i; };
  std::vector<E> e;
  for (size_t i = 0; i < Ms; ++i)
    if (valid[i]) e.push_back({std::sqrt(coef[i].x * coef[i].x + coef[i].y * coef[i].y + coef[i].z * coef[i].z), uint32_t(i)});
  if (e.size() < 50) return 0;
  std::stable_sort(e.begin(), e.end(), [](const E &a, const E &b) { return a.sc > b.sc; });
  for (size_t k = 0; k < e.size(); ++k) {
    if (score) score[k] = e[k].sc;
    if (point) std::memcpy(point + 4 * k, &pts[e[k].i], sizeof(float4));
    if (coeff) std::memcpy(coeff + 4 * k, &absc[e[k].i], sizeof(float4));
  }
  return e.size();
}

}  // namespace lio
