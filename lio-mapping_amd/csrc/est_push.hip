// est_push.hip — see est_push.h.  gfx950 kernels; blockIdx.y = the cloud (or the window of a slide), blockIdx.x = a block of 256 of its points,
// blocks past a cloud's own range leave at once.  Every kernel is a caller of the bodies of cloud_device.h; pointers read from a record are
// tied to a kernel-argument pointer (dev.h: rebase).  No atomics, no block waits for another: plain dependent launches on the part's stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "est_push.h"
#include "cloud_device.h"

namespace lio {

// ------------------------------------------------------------------------------------------------
// TransformToEnd (Estimator.cc:62-103, where the record says so) and, from the point still in registers, the filter's sort key in absolute
// cells and the block's share of the bounds (batch_kernels.hip: k_bw_concat_keys does the same behind its concat).  One point per lane: one
// 16-byte load from a clamped address, one 16-byte store.
// ------------------------------------------------------------------------------------------------
// the body behind the load: R's point `p` of lane `gid` (p: the cloud's last point in the lanes past it)
__device__ __forceinline__ void bp_take_keys_body(const BpCloud &R, const int c, float4 p, const int gid, float4 *__restrict__ in_all, uint32_t *__restrict__ keys,
                                                  float *__restrict__ partial, int *__restrict__ flag) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float cnt = 0;
  if (gid < R.vox.n) {
    if (R.deskew) p = deskew_to_end_point<false>(p, Quat<float>(R.qe[3], R.qe[0], R.qe[1], R.qe[2]), Vec3<float>(R.te[0], R.te[1], R.te[2]), R.time_factor);
    in_all[R.vox.off + gid] = p;
    // (a cloud beyond the absolute key is flagged: the handle's own filter has that form)
    keys[R.vox.off + gid] = vox_take_point<9, BW_KEY_NONE>(p, R.vox.inv_leaf, mn, mx, cnt, flag + c);
  }
  vox_block_partial(mn, mx, cnt, partial + (size_t(R.vox.off / VOX_TILE) + blockIdx.x) * 8);
}
__global__ void __launch_bounds__(VOX_TILE) k_bp_take_keys(const BpCloud *__restrict__ rec, const float4 *__restrict__ staging, float4 *__restrict__ in_all,
                                                          uint32_t *__restrict__ keys, float *__restrict__ partial, int *__restrict__ flag) {
  const int c = blockIdx.y;
  const BpCloud &R = rec[c];
  const int base = int(blockIdx.x) * VOX_TILE;
  if (base >= R.vox.cap) return;
  const int gid = base + threadIdx.x;
  bp_take_keys_body(R, c, staging[R.src_off + min(gid, max(R.vox.n - 1, 0))], gid, in_all, keys, partial, flag);
}
void launch_bp_take_keys(const BpCloud *rec, int nclouds, int max_n, const float4 *staging, float4 *in_all, uint32_t *keys, float *partial, int *flag, hipStream_t s) {
  if (nclouds <= 0) return;
  hipLaunchKernelGGL(k_bp_take_keys, dim3(std::max(1, cdiv(max_n, VOX_TILE)), nclouds), dim3(VOX_TILE), 0, s, rec, staging, in_all, keys, partial, flag);
  LIO_HIP(hipGetLastError());
}

// The device-fed form (include/lio_est_from_odom.h).  Rows < nclouds: the same body, the point read from the record's source (an odometry's
// last_corner_ / last_surf_; a cloud of no points has a source all the same: PushChain::run).  Rows >= nclouds: the full clouds, one FullTake each,
// through full_take_body (cloud_device.h) straight into a map's full cloud.
__global__ void __launch_bounds__(VOX_TILE) k_bp_take_keys_dev(const BpCloud *__restrict__ rec, const int nclouds, const FullTake *__restrict__ full,
                                                              float4 *__restrict__ in_all, uint32_t *__restrict__ keys, float *__restrict__ partial,
                                                              int *__restrict__ flag) {
  const int c = blockIdx.y;
  const int base = int(blockIdx.x) * VOX_TILE;
  const int gid = base + threadIdx.x;
  if (c >= nclouds) {
    const FullTake &F = full[c - nclouds];
    if (gid >= F.n) return;
    full_take_body(rebase(full, F.in), rebase(full, F.out), gid, rebase(full, F.to_end.st), F.to_end);
    return;
  }
  const BpCloud &R = rec[c];
  if (base >= R.vox.cap) return;
  bp_take_keys_body(R, c, rebase(rec, R.src)[min(gid, max(R.vox.n - 1, 0))], gid, in_all, keys, partial, flag);
}
void launch_bp_take_keys_dev(const BpCloud *rec, int nclouds, const FullTake *full, int nfull, int max_n, float4 *in_all, uint32_t *keys, float *partial, int *flag,
                             hipStream_t s) {
  if (nclouds + nfull <= 0) return;
  hipLaunchKernelGGL(k_bp_take_keys_dev, dim3(std::max(1, cdiv(max_n, VOX_TILE)), nclouds + nfull), dim3(VOX_TILE), 0, s, rec, nclouds, full, in_all, keys, partial,
                     flag);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// SlideWindow (Estimator.cc:2602-2615) of every window: what is left of the pivot's stack mapped into the next frame, then that frame's
// own stack, into the handle's scratch cloud (cloud_kernels.hip: k_transform_concat for one window)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bp_slide(const BpSlide *__restrict__ rec) {
  const BpSlide &S = rec[blockIdx.y];
  const int base = int(blockIdx.x) * 256;
  if (base >= S.total) return;
  const int gid = base + threadIdx.x;
  const float4 o = concat_point(S.seg, 2, min(gid, S.total - 1), rec);
  if (gid < S.total) rebase(rec, S.dst)[gid] = o;
}
void launch_bp_slide(const BpSlide *rec, int nwin, int max_total, hipStream_t s) {
  if (nwin <= 0 || max_total <= 0) return;
  hipLaunchKernelGGL(k_bp_slide, dim3(cdiv(max_total, 256), nwin), dim3(256), 0, s, rec);
  LIO_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// the chain
// ------------------------------------------------------------------------------------------------
void PushChain::begin(int max_clouds, int max_full, bool device_fed) {
  n_ = 0; total_ = 0; max_n_ = 0; staged_ = 0; nfull_ = 0; uploads_ = 0;
  device_fed_ = device_fed;
  src_.clear();
  if (max_clouds > cap_) {
    const size_t c = size_t(max_clouds) + size_t(max_clouds) / 2;
    h_rec_.alloc(c, hipHostMallocDefault, true);
    cap_ = int(c);
  }
  if (max_full > cap_full_) {
    const size_t c = size_t(max_full) + size_t(max_full) / 2;
    h_full_.alloc(c, hipHostMallocDefault, true);
    cap_full_ = int(c);
  }
}

int PushChain::add(CloudSrc src, float leaf, bool deskew, const float q[4], const float p[3], float time_factor, float4 *dst) {
  if (n_ >= cap_) throw std::runtime_error("PushChain: more clouds than the call announced");
  if (src.on_device != device_fed_) throw std::logic_error("PushChain: a cloud does not lie where the call announced");
  const size_t n = src.n;
  const int cap = int((std::max<size_t>(n, 1) + 255) / 256 * 256);
  if (size_t(total_) + size_t(cap) > size_t(INT_MAX) / 2) throw CapacityError("lio_est_batch_push_frames: the call's clouds exceed 2^30 points");
  BpCloud &R = h_rec_.p[n_];
  R.src_off = device_fed_ ? 0 : staged_;   // (a device source takes no range of the staging array)
  R.vox = VoxSeg{int(n), total_, cap, 1.0f / leaf, dst};
  R.deskew = deskew ? 1 : 0;
  for (int k = 0; k < 4; ++k) R.qe[k] = q[k];
  for (int k = 0; k < 3; ++k) R.te[k] = p[k];
  R.time_factor = time_factor;
  R.src = device_fed_ && n ? src.p : nullptr;
  src_.push_back(src.p);
  total_ += cap;
  if (!device_fed_) staged_ += cap;
  max_n_ = std::max(max_n_, int(n));
  return n_++;
}

void PushChain::add_full(const FullTake &f) {
  if (!device_fed_ || nfull_ >= cap_full_) throw std::runtime_error("PushChain: more full clouds than the call announced");
  h_full_.p[nfull_++] = f;
  max_n_ = std::max(max_n_, f.n);
}

bool PushChain::run(SegVoxFilter &vox, int passes, hipStream_t s) {
  if (n_ == 0 && nfull_ == 0) return false;
  const size_t N = size_t(total_), C = size_t(n_);
  staging_.reserve(size_t(staged_), s); in_all_.reserve(N, s); d_rec_.reserve(C, s);
  if (n_) vox.reserve(N, n_, s);
  if (device_fed_) {
    // no cloud goes up: the records carry the sources.  The one load per lane is unconditional, so a cloud of no points reads (and drops) the
    // first point of its own range of the input array
    for (int i = 0; i < n_; ++i)
      if (!h_rec_.p[i].src) h_rec_.p[i].src = in_all_.p + h_rec_.p[i].vox.off;
    if (nfull_) {
      d_full_.reserve(size_t(nfull_), s);
      LIO_HIP(hipMemcpyAsync(d_full_.p, h_full_.p, sizeof(FullTake) * size_t(nfull_), hipMemcpyHostToDevice, s));
    }
  } else {
    // the clouds into the staging array
    for (int i = 0; i < n_; ++i) {
      const BpCloud &R = h_rec_.p[i];
      if (R.vox.n) {
        LIO_HIP(hipMemcpyAsync(staging_.p + R.src_off, src_[size_t(i)], size_t(R.vox.n) * sizeof(float4), hipMemcpyHostToDevice, s));
        ++uploads_;
      }
    }
  }
  // the records in one table
  if (n_) LIO_HIP(hipMemcpyAsync(d_rec_.p, h_rec_.p, sizeof(BpCloud) * C, hipMemcpyHostToDevice, s));
  if (device_fed_) launch_bp_take_keys_dev(d_rec_.p, n_, d_full_.p, nfull_, max_n_, in_all_.p, vox.keys(), vox.partial(), vox.flag(), s);
  else launch_bp_take_keys(d_rec_.p, n_, max_n_, staging_.p, in_all_.p, vox.keys(), vox.partial(), vox.flag(), s);
  if (n_) vox.finish(&d_rec_.p->vox, &h_rec_.p->vox, sizeof(BpCloud), n_, passes, in_all_.p, nullptr, s);
  LIO_HIP(hipStreamSynchronize(s));   // the call's one wait
  return true;
}

}  // namespace lio
