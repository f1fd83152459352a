// odometry.hip — gfx950 kernels + host chain of the LOAM scan-to-scan step (see odometry.h).
//
// One launch chain serves one sensor and a batch of them alike: every sensor has a record of a device table (OdoBatchRec) with its own clouds,
// state, grids and slices, and lio_odom_process is a batch of one.  The device bodies are stated once (odo_*_body); per iteration
//   k_ob_corr    one wavefront per feature point: TransformToStart, exact nearest neighbour over the previous sweep's cloud (the 27 cells of
//                a 5 m grid around the query), then the +-2.5-ring window scan of PointOdometry.cc:353-380 / :451-488 in 64-wide chunks.  The
//                sequential "first strictly smaller wins" selection is reproduced as argmin over (distance, scan order); the early `break`
//                on the ring bound is reproduced with a ballot inside the chunk.  Every fifth iteration.
//   k_ob_rows    edge / plane coefficients (:391-435, :497-531), weights (A.7), rows of A and B (:548-571), reduced to per-block partials.
//   k_ob_update  6x6 solve, degeneracy mask (threshold 10, A.6), update, abort test (:573-650).
// and around them k_ob_take (the clouds from the feature extraction), GridBatch (cloud_kernels.h: the grids over the previous clouds, all
// sensors' side by side) and k_ob_to_end (TransformToEnd, :262-292).  k_odo_to_end is TransformToEnd of a caller's cloud (FullToEnd).
// The <= 25 rounds run without a host round trip except a convergence peek every 5 rounds.
// The test hooks (include/lio_test_hooks.h) build the same table for one sensor and launch k_ob_corr or k_ob_rows once over it; k_odo_sel and
// k_gn_rows_odom give them every query's sel and row on its own, k_gn_odo_step the 6x6 step on caller-given sums.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstring>

#include "odometry.h"
#include "../../include/lio_frontend_batch.h"
#include "cloud_device.h"

namespace lio {

struct OdoArgs {
  const float4 *sharp; int nc;
  const float4 *flat; int ns;
  const float4 *lastc; int nlc;
  const float4 *lasts; int nls;
  float time_factor; int no_deskew;
  // 5 m uniform grids over the previous sweep's clouds (cell-sorted copies, original index in .w): every point within the
  // 25 m^2 acceptance gate of a query (PointOdometry.cc:349,448) lies in the 27 cells around it
  const float4 *gc_sorted; const int *gc_cells; GridDesc gc;
  const float4 *gs_sorted; const int *gs_cells; GridDesc gs;
};

__device__ inline bool odo_to_start(const float4 &pi, const Quat<float> &qe, const Vec3<float> &te, float time_factor, int no_deskew,
                                    Vec3<float> &out) {
  float s = time_factor * (pi.w - int(pi.w));
  if (no_deskew) s = 0;
  if (s < 0 || double(s) > 1.001) { out = Vec3<float>(pi.x, pi.y, pi.z); return false; }
  Vec3<float> p(pi.x - s * te.x, pi.y - s * te.y, pi.z - s * te.z);
  Quat<float> qid;
  Quat<float> qs = slerp(qid, s, qe, FLT_EPSILON);
  out = rotate(conj(qs), p);
  return true;
}

__device__ inline float odo_sqdiff(const float4 &a, const Vec3<float> &b) {
  float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return dx * dx + dy * dy + dz * dz;
}

// wave-wide argmin over (d, key); returns the winning key (INT_MAX when nobody has d < limit)
__device__ inline void wave_argmin(float &d, int &key) {
  for (int off = 32; off > 0; off >>= 1) {
    float od = __shfl_xor(d, off, 64);
    int ok = __shfl_xor(key, off, 64);
    if (od < d || (od == d && ok < key)) { d = od; key = ok; }
  }
}

// The device bodies below take one sensor's arguments, state and slices: the k_ob_* kernels run them for every sensor of a table, so a sensor
// computes the same bits alone and in any batch.
// query qi of one sensor by one wavefront (lane = 0 .. 63)
__device__ __forceinline__ void odo_corr_body(const OdoArgs &a, const OdomState *__restrict__ st, int *__restrict__ idx, const int qi, const int lane) {
  if (st->converged) return;
  const bool corner = qi < a.nc;
  const float4 pi = corner ? a.sharp[qi] : a.flat[qi - a.nc];
  const float4 *cloud = corner ? a.lastc : a.lasts;
  const int n = corner ? a.nlc : a.nls;
  Quat<float> qe(st->T[3], st->T[0], st->T[1], st->T[2]);
  Vec3<float> te(st->T[4], st->T[5], st->T[6]);
  Vec3<float> sel;
  odo_to_start(pi, qe, te, a.time_factor, a.no_deskew, sel);
  // ---- exact 1-NN inside the 25 m^2 gate, ties -> lower index: lanes stride over the nine x-runs of the 27 neighbouring
  // cells (a nearest neighbour farther than one cell away is rejected by the gate anyway)
  float bd = INFINITY; int bi = INT_MAX;
  {
    const float4 *gmap = corner ? a.gc_sorted : a.gs_sorted;
    const int *gcells = corner ? a.gc_cells : a.gs_cells;
    const GridDesc &g = corner ? a.gc : a.gs;
    const int cx = int(floorf(sel.x * g.inv_cell)) - g.origin[0], cy = int(floorf(sel.y * g.inv_cell)) - g.origin[1],
              cz = int(floorf(sel.z * g.inv_cell)) - g.origin[2];
    if (cx >= 0 && cy >= 0 && cz >= 0 && cx < g.dims[0] && cy < g.dims[1] && cz < g.dims[2]) {
      for (int r = 0; r < 9; ++r) {
        const int z = cz + (r / 3 - 1), y = cy + (r % 3 - 1);
        if (z < 0 || z >= g.dims[2] || y < 0 || y >= g.dims[1]) continue;
        const int row = g.dims[0] * (y + g.dims[1] * z);
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dims[0] - 1);
        const int rs = gcells[row + x0], re = gcells[row + x1 + 1];
        if (re <= rs) continue;
        for (int j = rs + lane; j < re; j += 64) {
          const float4 p = gmap[j];
          const float d = odo_sqdiff(p, sel);
          const int id = __float_as_int(p.w);
          if (d < bd || (d == bd && id < bi)) { bd = d; bi = id; }
        }
      }
    }
  }
  wave_argmin(bd, bi);
  int closest = -1, second = -1, third = -1;
  if (bi != INT_MAX && bd < 25.f) {
    closest = bi;
    const int cs = int(cloud[closest].w);
    float d2 = 25.f, d3 = 25.f;     // best "second" / "third" squared distances so far
    int k2 = INT_MAX, k3 = INT_MAX;  // their scan-order keys
    // The two window scans walk up to 2.5 rings (~1 500 points of an HDL-64E sweep) in chunks of 64.  A chunk's decision to go on depends
    // on its rings, but its LOADS do not: four chunks' points are requested together and then examined in scan order, stopping at the
    // first ring violation as before (one memory round trip per 256 candidates instead of one per 64: the scan was a chain of ~48
    // dependent L2 round trips per query).
    // upward scan; scan-order key = j - closest (1, 2, ...)
    for (int base4 = closest + 1; base4 < n; base4 += 256) {
      float4 pj[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int j = base4 + 64 * q + lane; pj[q] = cloud[j < n ? j : n - 1]; }
      bool stop = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (stop || base4 + 64 * q >= n) continue;   // (uniform)
        const int j = base4 + 64 * q + lane;
        const bool in = j < n;
        const int ring = in ? int(pj[q].w) : INT_MAX;
        const bool viol = in && (double(ring) > double(cs) + 2.5);
        const unsigned long long vm = __ballot(viol);
        const int first_viol = vm ? (__ffsll((long long)vm) - 1) : 64;
        if (in && lane < first_viol) {
          const float d = odo_sqdiff(pj[q], sel);
          const int key = j - closest;
          if (corner) {
            if (ring > cs && (d < d2 || (d == d2 && key < k2 && d < 25.f))) { d2 = d; k2 = key; }
          } else {
            if (ring <= cs) { if (d < d2 || (d == d2 && key < k2 && d < 25.f)) { d2 = d; k2 = key; } }
            else { if (d < d3 || (d == d3 && key < k3 && d < 25.f)) { d3 = d; k3 = key; } }
          }
        }
        if (vm) stop = true;
      }
      if (stop) break;
    }
    // downward scan; keys continue after every possible upward key
    const int KOFF = 1 << 24;
    for (int base4 = closest - 1; base4 >= 0; base4 -= 256) {
      float4 pj[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int j = base4 - 64 * q - lane; pj[q] = cloud[j >= 0 ? j : 0]; }
      bool stop = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (stop || base4 - 64 * q < 0) continue;   // (uniform)
        const int j = base4 - 64 * q - lane;
        const bool in = j >= 0;
        const int ring = in ? int(pj[q].w) : INT_MIN;
        const bool viol = in && (double(ring) < double(cs) - 2.5);
        const unsigned long long vm = __ballot(viol);
        const int first_viol = vm ? (__ffsll((long long)vm) - 1) : 64;
        if (in && lane < first_viol) {
          const float d = odo_sqdiff(pj[q], sel);
          const int key = KOFF + (closest - j);
          if (corner) {
            if (ring < cs && (d < d2 || (d == d2 && key < k2 && d < 25.f))) { d2 = d; k2 = key; }
          } else {
            if (ring >= cs) { if (d < d2 || (d == d2 && key < k2 && d < 25.f)) { d2 = d; k2 = key; } }
            else { if (d < d3 || (d == d3 && key < k3 && d < 25.f)) { d3 = d; k3 = key; } }
          }
        }
        if (vm) stop = true;
      }
      if (stop) break;
    }
    wave_argmin(d2, k2);
    if (k2 != INT_MAX && d2 < 25.f) second = k2 < KOFF ? closest + k2 : closest - (k2 - KOFF);
    if (!corner) {
      wave_argmin(d3, k3);
      if (k3 != INT_MAX && d3 < 25.f) third = k3 < KOFF ? closest + k3 : closest - (k3 - KOFF);
    }
  }
  if (lane == 0) {
    if (corner) { idx[2 * qi] = closest; idx[2 * qi + 1] = second; }
    else { int o = 2 * a.nc + 3 * (qi - a.nc); idx[o] = closest; idx[o + 1] = second; idx[o + 2] = third; }
  }
}

// sel of every query (sharp first), as odo_corr_body and odo_row_coeff see it: 3 floats per query
__global__ void __launch_bounds__(256) k_odo_sel(OdoArgs a, const OdomState *__restrict__ st, float *__restrict__ sel_out) {
  const int qi = blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= a.nc + a.ns) return;
  const float4 pi = qi < a.nc ? a.sharp[qi] : a.flat[qi - a.nc];
  Quat<float> qe(st->T[3], st->T[0], st->T[1], st->T[2]);
  Vec3<float> te(st->T[4], st->T[5], st->T[6]);
  Vec3<float> sel;
  odo_to_start(pi, qe, te, a.time_factor, a.no_deskew, sel);
  sel_out[3 * qi] = sel.x; sel_out[3 * qi + 1] = sel.y; sel_out[3 * qi + 2] = sel.z;
}

#define ODO_ROW_THREADS 256

// The row of query qi (sharp first) at transform_es_ = (qe, te) on the correspondences `idx`, in the two halves the loop of odo_rows_body has
// around its `continue`; the test hook lio_gn_rows_odom calls the same two.
// odo_row_coeff: TransformToStart, edge / plane coefficients (:391-435, :497-531) and weight (A.7).  false: the query has no row.
__device__ __forceinline__ bool odo_row_coeff(const OdoArgs &a, const Quat<float> &qe, const Vec3<float> &te, const int *__restrict__ idx, int iter, int qi,
                                              float4 &pi_out, float4 &c_out) {
  const bool corner = qi < a.nc;
  const float4 pi = corner ? a.sharp[qi] : a.flat[qi - a.nc];
  Vec3<float> sel;
  odo_to_start(pi, qe, te, a.time_factor, a.no_deskew, sel);
  float c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  bool ok = false;
  if (corner) {
    int i1 = idx[2 * qi], i2 = idx[2 * qi + 1];
    if (i2 >= 0) {
      float4 t1 = a.lastc[i1], t2 = a.lastc[i2];
      float x0 = sel.x, y0 = sel.y, z0 = sel.z, x1 = t1.x, y1 = t1.y, z1 = t1.z, x2 = t2.x, y2 = t2.y, z2 = t2.z;
      float a012 = sqrtf(((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) * ((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) +
                         ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)) * ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)) +
                         ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)) * ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)));
      float l12 = sqrtf((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2));
      float la = ((y1 - y2) * ((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) + (z1 - z2) * ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1))) / a012 / l12;
      float lb = -((x1 - x2) * ((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) - (z1 - z2) * ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1))) / a012 / l12;
      float lc = -((x1 - x2) * ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)) + (y1 - y2) * ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1))) / a012 / l12;
      float ld2 = a012 / l12;
      float s = 1;
      if (iter >= 5) s = 1 - 1.8f * fabsf(ld2);
      if (double(s) > 0.1 && ld2 != 0) { ok = true; c0 = s * la; c1 = s * lb; c2 = s * lc; c3 = s * ld2; }
    }
  } else {
    int o = 2 * a.nc + 3 * (qi - a.nc);
    int i1 = idx[o], i2 = idx[o + 1], i3 = idx[o + 2];
    if (i2 >= 0 && i3 >= 0) {
      float4 t1 = a.lasts[i1], t2 = a.lasts[i2], t3 = a.lasts[i3];
      float pa = (t2.y - t1.y) * (t3.z - t1.z) - (t3.y - t1.y) * (t2.z - t1.z);
      float pb = (t2.z - t1.z) * (t3.x - t1.x) - (t3.z - t1.z) * (t2.x - t1.x);
      float pc = (t2.x - t1.x) * (t3.y - t1.y) - (t3.x - t1.x) * (t2.y - t1.y);
      float pd = -(pa * t1.x + pb * t1.y + pc * t1.z);
      float ps = sqrtf(pa * pa + pb * pb + pc * pc);
      pa /= ps; pb /= ps; pc /= ps; pd /= ps;
      float pd2 = pa * sel.x + pb * sel.y + pc * sel.z + pd;
      float s = 1;
      if (iter >= 5) s = 1 - 1.8f * fabsf(pd2) / sqrtf(sqrtf(sel.x * sel.x + sel.y * sel.y + sel.z * sel.z));
      if (double(s) > 0.1 && pd2 != 0) { ok = true; c0 = s * pa; c1 = s * pb; c2 = s * pc; c3 = s * pd2; }
    }
  }
  pi_out = pi; c_out = make_float4(c0, c1, c2, c3);
  return ok;
}
// odo_row_of: r[6] and b of a selected query (:548-571), Rt = R(qe)^T
__device__ __forceinline__ void odo_row_of(const float4 pi, const float4 c, const Quat<float> &qe, const Vec3<float> &te, const Mat3<float> &Rt, float (&r)[6],
                                           float &bb) {
  const float c0 = c.x, c1 = c.y, c2 = c.z, c3 = c.w;
  Vec3<float> p(pi.x, pi.y, pi.z), w(c0, c1, c2);
  Vec3<float> pmt = p - te;
  Vec3<float> cc = rotate(conj(qe), pmt);
  Mat3<float> S = skew(cc);
  r[0] = w.x * S(0, 0) + w.y * S(1, 0) + w.z * S(2, 0);
  r[1] = w.x * S(0, 1) + w.y * S(1, 1) + w.z * S(2, 1);
  r[2] = w.x * S(0, 2) + w.y * S(1, 2) + w.z * S(2, 2);
  r[3] = -(w.x * Rt(0, 0) + w.y * Rt(1, 0) + w.z * Rt(2, 0));
  r[4] = -(w.x * Rt(0, 1) + w.y * Rt(1, 1) + w.z * Rt(2, 1));
  r[5] = -(w.x * Rt(0, 2) + w.y * Rt(1, 2) + w.z * Rt(2, 2));
  bb = float(-0.1 * double(c3));
}

// block `block` of the `nblocks` (ODO_ROW_THREADS threads each) that share one sensor's queries; 28 doubles to partials[block * 28 ...]
__device__ __forceinline__ void odo_rows_body(const OdoArgs &a, const OdomState *__restrict__ st, const int *__restrict__ idx, int iter,
                                              double *__restrict__ partials, const int block, const int nblocks) {
  if (st->converged) return;
  Quat<float> qe(st->T[3], st->T[0], st->T[1], st->T[2]);
  Vec3<float> te(st->T[4], st->T[5], st->T[6]);
  Mat3<float> Rt = transpose(toRot(qe));
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0;
  const int total = a.nc + a.ns;
  for (int qi = block * ODO_ROW_THREADS + threadIdx.x; qi < total; qi += nblocks * ODO_ROW_THREADS) {
    float4 pi, c;
    if (!odo_row_coeff(a, qe, te, idx, iter, qi, pi, c)) continue;
    float r[6], bb;
    odo_row_of(pi, c, qe, te, Rt, r, bb);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) acc[k++] += double(r[i] * r[j]);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += double(r[i] * bb);
    acc[27] += 1.0;
  }
  __shared__ double sm[ODO_ROW_THREADS / 64][28];
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
    for (int w = 0; w < ODO_ROW_THREADS / 64; ++w) v += sm[w][threadIdx.x];
    partials[block * 28 + threadIdx.x] = v;
  }
}
// the row of every query on its own (lio_gn_rows_odom): one query per lane through odo_row_coeff and odo_row_of; 7 floats (r0 .. r5, b), zeros and ok = 0
// where the query has no row
__global__ void __launch_bounds__(256) k_gn_rows_odom(OdoArgs a, const OdomState *__restrict__ st, const int *__restrict__ idx, int iter,
                                                      uint8_t *__restrict__ ok_out, float *__restrict__ rows_out) {
  const int qi = blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= a.nc + a.ns) return;
  Quat<float> qe(st->T[3], st->T[0], st->T[1], st->T[2]);
  Vec3<float> te(st->T[4], st->T[5], st->T[6]);
  Mat3<float> Rt = transpose(toRot(qe));
  float4 pi, c;
  float r[6] = {0, 0, 0, 0, 0, 0}, bb = 0;
  const bool ok = odo_row_coeff(a, qe, te, idx, iter, qi, pi, c);
  if (ok) odo_row_of(pi, c, qe, te, Rt, r, bb);
  ok_out[qi] = ok ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) rows_out[size_t(qi) * 7 + k] = ok ? r[k] : 0.f;
  rows_out[size_t(qi) * 7 + 6] = ok ? bb : 0.f;
}

// the serial 6x6 step of one iteration (thread 0); see odo_update_body
__device__ __forceinline__ void odo_update_step(const double *ssum, OdomState *st, int iter);
// mail / sig: at the iterations where the host looks at the convergence flag (every fifth) the state is posted to its mailbox
// (dev.h: HostSignal) instead of being fetched with a copy + stream synchronisation
// one 256-thread block
__device__ __forceinline__ void odo_update_body(const double *__restrict__ partials, int nblocks, OdomState *st, int iter, OdomState *mail,
                                                const HostSignal &sig, float *__restrict__ trace) {
  if (!st->converged) {
    __shared__ double ssum[28];
    reduce_partials28(partials, nblocks, ssum);
    if (threadIdx.x == 0) {
      odo_update_step(ssum, st, iter);
      // per-iteration record of transform_es_ (lio_odom_get_iteration_trace); 32 B, read back once per sweep
      for (int k = 0; k < 7; ++k) trace[iter * 8 + k] = st->T[k];
    }
  }
  if (sig.flag) {
    __syncthreads();
    if (threadIdx.x < 64) post_host_mail(sig, mail, st, int(sizeof(OdomState) / 4), threadIdx.x);
  }
}
__device__ __forceinline__ void odo_update_step(const double *ssum, OdomState *st, int iter) {
  double sum[28];
  for (int k = 0; k < 28; ++k) sum[k] = ssum[k];
  st->iters = iter + 1;
  st->kz = st->kz;  // (kept from round 0)
  const int nsel = int(sum[27]);
  st->T[7] = float(nsel);  // pad slot carries the selected-correspondence count back to the host
  if (nsel < 10) return;   // PointOdometry.cc:535
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
    const int kz = count_eigs_below<6>(AtA, 10.0);
    st->kz = kz;
    st->degenerate = kz > 0;
  }
  if (st->degenerate)
    for (int i = 0; i < st->kz; ++i) X[i] = 0.f;
  Quat<float> q(st->T[3], st->T[0], st->T[1], st->T[2]);
  Quat<float> R0 = normalized(q);
  Vec3<float> t(st->T[4], st->T[5], st->T[6]);
  t.x += X[3]; t.y += X[4]; t.z += X[5];
  q = q * deltaQ(Vec3<float>(X[0], X[1], X[2]));
  if (!isfinite(t.x)) t.x = 0;
  if (!isfinite(t.y)) t.y = 0;
  if (!isfinite(t.z)) t.z = 0;
  st->T[0] = q.x; st->T[1] = q.y; st->T[2] = q.z; st->T[3] = q.w; st->T[4] = t.x; st->T[5] = t.y; st->T[6] = t.z;
  Quat<float> d = R0 * conj(q);
  float ang = 2.f * atan2f(norm(d.vec()), fabsf(d.w));
  float delta_r = float(double(ang) * 180.0 / M_PI);
  double dt0 = double(X[3] * 100), dt1 = double(X[4] * 100), dt2 = double(X[5] * 100);
  float delta_t = float(sqrt(dt0 * dt0 + dt1 * dt1 + dt2 * dt2));
  if (double(delta_r) < 0.1 && double(delta_t) < 0.1) st->converged = 1;
}

// lio_gn_step, family 1 (include/lio_test_hooks.h): thread 0 runs odo_update_step on the state in place; the row count it leaves in the pad
// slot is also written to nsel
__global__ void __launch_bounds__(64) k_gn_odo_step(const double *__restrict__ sums, OdomState *st, int iter) {
  if (threadIdx.x != 0) return;
  odo_update_step(sums, st, iter);
  st->nsel = int(st->T[7]);
}
void launch_gn_odo_step(const double *sums, OdomState *st, int iter, hipStream_t s) {
  hipLaunchKernelGGL(k_gn_odo_step, dim3(1), dim3(64), 0, s, sums, st, iter);
  LIO_HIP(hipGetLastError());
}

// TransformToEnd (:261-292) of a caller's cloud: odo_to_end_body (cloud_device.h)
__global__ void __launch_bounds__(256) k_odo_to_end(const float4 *in, float4 *out, int n, const OdomState *__restrict__ st, float time_factor, int no_deskew) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  odo_to_end_body(in, out, i, st, time_factor, no_deskew);
}

// ---- the chain's kernels: the bodies above, every sensor with its own record of a device table
// One sensor of a call (lio_odom_process: the only one).  Iterating sensors come first in the table (the k_ob_corr / k_ob_rows / k_ob_update launches cover only them);
// behind them those that only carry their clouds to the sweep's end (previous clouds too small to iterate: `a` holds time_factor and
// no_deskew alone).
struct OdoBatchRec {
  OdoArgs a;
  OdomState *st;              // the handle's own state
  float4 *ls; int n_ls;       // its less-sharp / less-flat clouds of this sweep (k_ob_to_end, in place)
  float4 *lf; int n_lf;
  int idx_off;                // first of its 2 * nc + 3 * ns entries in the batch's index table
  int nb;                     // its row blocks: max(1, min(cdiv(nq, ODO_ROW_THREADS), 64)), the partition it has alone
  int part_off;               // its first row (28 doubles each) of the batch's partials
  int trace_off;              // its first float of the batch's trace table (8 per iteration)
};

// grid (max nq, sensors) x 64: one wavefront per query; the blocks beyond a sensor's own queries leave at once
__global__ void __launch_bounds__(64) k_ob_corr(const OdoBatchRec *__restrict__ recs, int *__restrict__ idx_all) {
  const OdoBatchRec &r = recs[blockIdx.y];
  if (int(blockIdx.x) >= r.a.nc + r.a.ns) return;
  odo_corr_body(r.a, r.st, idx_all + r.idx_off, blockIdx.x, threadIdx.x);
}
// grid (max nb, sensors): sensor k is served by its first nb_k blocks with the stride nb_k * ODO_ROW_THREADS — its partition alone, NOT the
// grid's width: the order in which a thread adds its rows, and so every bit of the sums, hangs on it
__global__ void __launch_bounds__(ODO_ROW_THREADS) k_ob_rows(const OdoBatchRec *__restrict__ recs, const int *__restrict__ idx_all, int iter,
                                                             double *__restrict__ partials_all) {
  const OdoBatchRec &r = recs[blockIdx.y];
  if (int(blockIdx.x) >= r.nb) return;
  odo_rows_body(r.a, r.st, idx_all + r.idx_off, iter, partials_all + size_t(r.part_off) * 28, blockIdx.x, r.nb);
}
// one 256-thread block per sensor; at the iterations the host looks at, every sensor (a converged one too) posts its state to its own
// mailbox slot and then stores sig.seq into its own completion word
__global__ void k_ob_update(const OdoBatchRec *__restrict__ recs, const double *__restrict__ partials_all, int iter, char *mail, HostSignal sig,
                            float *__restrict__ trace_all) {
  const OdoBatchRec &r = recs[blockIdx.x];
  HostSignal mine = sig;
  char *slot = state_mail_slot(mail, mine, blockIdx.x);
  odo_update_body(partials_all + size_t(r.part_off) * 28, r.nb, r.st, iter, reinterpret_cast<OdomState *>(slot), mine, trace_all + r.trace_off);
}
// grid (cdiv(max(n_ls + n_lf), 256), sensors): the less-sharp points of a sensor, then its less-flat points, each in place
__global__ void __launch_bounds__(256) k_ob_to_end(const OdoBatchRec *__restrict__ recs) {
  const OdoBatchRec &r = recs[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.n_ls + r.n_lf) return;
  float4 *c = i < r.n_ls ? r.ls : r.lf;
  odo_to_end_body(c, c, i < r.n_ls ? i : i - r.n_ls, r.st, r.a.time_factor, r.a.no_deskew);
}

// ---- the hand-over from the feature extraction (lio_odom_process_batch_from_pp): one sensor's four clouds, where the processor left them on
// the device, into the handle's sharp_ / less_sharp_ / flat_ / less_flat_, and the state its iterations start from
struct OdoTakeRec {
  const float4 *src[4]; float4 *dst[4]; int n[4];   // sharp, less sharp, flat, less flat; n = 0: not taken
  OdomState *st;                                    // null: the sensor only stores or packs its clouds
  OdomState init;
};
// grid (cdiv(max n, 256), 4, sensors): one float4 per thread
__global__ void __launch_bounds__(256) k_ob_take(const OdoTakeRec *__restrict__ recs) {
  const OdoTakeRec &r = recs[blockIdx.z];
  const int c = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && c == 0 && r.st && threadIdx.x < sizeof(OdomState) / 4)
    reinterpret_cast<int *>(r.st)[threadIdx.x] = reinterpret_cast<const int *>(&r.init)[threadIdx.x];
  if (i < r.n[c]) r.dst[c][i] = r.src[c][i];
}

// One call's chain over the table, and its scratch, kept by the first handle of the call.  No results live here: the states and clouds are the
// handles' own, and the grids of a call are rebuilt by every call from the handles' previous clouds.  The steps run in the order they are
// declared in; ProcessBatch runs all five, the test hooks the table and the grids in front of one launch of their own.
struct OdoChain {
  // ---- the call
  OdometryDev *const *o = nullptr;   // its handles; the chain runs on o[0]'s stream (the other handles are idle: every entry point returns synchronised)
  hipStream_t s = nullptr;
  int max_iter = 0;
  std::vector<int> act, idle;        // who iterates, and who only carries its clouds to the sweep's end; the table holds `act`, then `idle`
  std::vector<OdomState> st, got;    // per handle: the state it starts from and ends with; per iterating sensor: the state its mailbox held
  int max_nq = 0, max_nb = 0, max_np = 0;   // the launches' widths: queries, row blocks, points to the end
  size_t idx_total = 0, part_total = 0;
  int nA() const { return int(act.size()); }
  int nE() const { return int(act.size() + idle.size()); }
  int who(int j) const { return j < nA() ? act[size_t(j)] : idle[size_t(j - nA())]; }   // the handle (index into o) of table record j
  OdometryDev &dev(int j) const { return *o[who(j)]; }
  // ---- the scratch
  GridBatch grids;            // the grids over the previous clouds of `act`: 2 * j over a.lastc, 2 * j + 1 over a.lasts of record j
  OdoBatchRec *h_recs = nullptr;         // the table, in front of the grids' own records in their staging table: one upload carries both
  const OdoBatchRec *d_recs = nullptr;
  DBuf<int> d_idx;
  DBuf<double> d_partials;
  DBuf<float> d_trace;
  std::vector<float> h_trace;
  StateMail mail;
  std::vector<OdoTakeRec> h_take;
  DBuf<OdoTakeRec> d_take;

  void Begin(OdometryDev *const *handles, int n);
  void TakeClouds(int n, const OdometryDev::Clouds *in);
  void FillTable(const OdometryDev::Clouds *in);
  void MakeGrids();
  void Iterate();
  void Finish();
};

// ------------------------------------------------------------------------------------------------
OdometryDev::OdometryDev(float scan_period, int io_ratio, int max_iter, bool no_deskew)
    : scan_period_(scan_period), time_factor_(1 / scan_period), io_ratio_(io_ratio), max_iter_(max_iter), no_deskew_(no_deskew) {
  int nd = 0;
  LIO_HIP(hipGetDeviceCount(&nd));
  if (nd <= 0) throw DeviceError("no HIP device: the product has no CPU path");
  LIO_HIP(hipStreamCreate(&stream_));
  d_state_.reserve(1);
}
OdometryDev::~OdometryDev() {
  if (stream_) (void)hipStreamDestroy(stream_);
}
OdoChain &OdometryDev::Chain() {
  if (!chain_) chain_.reset(new OdoChain);
  return *chain_;
}

static void upload(DBuf<float4> &b, CloudSrc src, hipStream_t s) {
  b.reserve(std::max<size_t>(src.n, 1));
  if (src.n) LIO_HIP(hipMemcpyAsync(b.p, src.p, src.n * sizeof(float4), src.to_device(), s));
}

// What the host keeps of the state the iterations ended with: :654-656 accumulate, :663 normalise.  TransformToEnd (:660-661) runs on the
// device with the state's own, not normalised transform_es_.
void OdometryDev::Accumulate(const OdomState &st) {
  iterations_done_ = st.iters;
  last_kz_ = st.degenerate ? st.kz : 0;
  last_num_sel_ = int(st.T[7]);
  transform_es_ = Rigid<float>(Quat<float>(st.T[3], st.T[0], st.T[1], st.T[2]), Vec3<float>(st.T[4], st.T[5], st.T[6]));
  transform_sum_ = compose(transform_sum_, rinverse(transform_es_));
  transform_es_.rot = normalized(transform_es_.rot);
  to_end_ready_ = true;
}

void OdoChain::Begin(OdometryDev *const *handles, int n) {
  o = handles; s = handles[0]->stream_; max_iter = handles[0]->max_iter_;
  act.clear(); idle.clear();
  st.assign(size_t(n), OdomState{});
}

// ---- step 1: the clouds and the starting state, per sensor: uploads from the host, or (clouds on the device) one record of the take table
// each; who iterates (`act`: previous clouds of more than 10 corner and 100 surf points), who only carries its clouds to the end (`idle`),
// who only stores them (neither: the first sweep, :302-310, and the packer)
void OdoChain::TakeClouds(int n, const OdometryDev::Clouds *in) {
  const bool on_device = clouds_on_device(size_t(4) * size_t(n), [&](size_t i) { return in[i / 4].c[i % 4]; });
  if (on_device) h_take.assign(size_t(n), OdoTakeRec{});
  size_t max_take = 0;
  // cloud i of sensor k: sharp, less sharp, flat, less flat
  auto take = [&](int k, int i, DBuf<float4> &b) {
    const CloudSrc &src = in[k].c[i];
    if (!on_device) { upload(b, src, s); return; }
    if (src.n > size_t(INT_MAX)) throw CapacityError("lio_odom_process_batch_from_pp: a cloud exceeds 2^31 points");
    b.reserve(std::max<size_t>(src.n, 1));
    OdoTakeRec &r = h_take[size_t(k)];
    r.src[i] = src.p; r.dst[i] = b.p; r.n[i] = int(src.n);
    max_take = std::max(max_take, src.n);
  };
  for (int k = 0; k < n; ++k) {
    OdometryDev &d = *o[k];
    d.iterations_done_ = 0; d.last_num_sel_ = 0; d.last_kz_ = 0; d.es_trace_.clear();
    take(k, 1, d.less_sharp_);
    take(k, 3, d.less_flat_);
    if (!d.inited_ || !d.enable_odom_) continue;
    OdomState &t = st[size_t(k)];
    t = odom_state_at(d.transform_es_);
    if (on_device) { h_take[size_t(k)].st = d.d_state_.p; h_take[size_t(k)].init = t; }
    else LIO_HIP(hipMemcpyAsync(d.d_state_.p, &t, sizeof(t), hipMemcpyHostToDevice, s));
    if (d.n_last_corner_ > 10 && d.n_last_surf_ > 100) {
      take(k, 0, d.sharp_);
      take(k, 2, d.flat_);
      act.push_back(k);
    } else {
      idle.push_back(k);
    }
  }
  if (on_device) {   // every sensor's clouds and state in one launch behind one upload
    d_take.reserve(size_t(n));
    LIO_HIP(hipMemcpyAsync(d_take.p, h_take.data(), size_t(n) * sizeof(OdoTakeRec), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ob_take, dim3(std::max(1, cdiv(max_take, 256)), 4, n), dim3(256), 0, s, d_take.p);
    LIO_HIP(hipGetLastError());
  }
}

// ---- step 2: the table of `act` and `idle`, all of it but the grids (the host does not know the previous clouds' bounds yet), and the buffers
// whose sizes it states.  in[k]: the counts of o[k]'s clouds; the clouds themselves lie in the handles.
void OdoChain::FillTable(const OdometryDev::Clouds *in) {
  const int na = nA(), ne = nE();
  h_recs = static_cast<OdoBatchRec *>(grids.begin(size_t(ne) * sizeof(OdoBatchRec), 2 * na));
  d_recs = static_cast<const OdoBatchRec *>(grids.head_dev());
  idx_total = part_total = 0;
  max_nq = max_nb = max_np = 0;
  for (int j = 0; j < ne; ++j) {
    const int k = who(j);
    OdometryDev &d = *o[k];
    const size_t n_sharp = in[k].c[0].n, n_ls = in[k].c[1].n, n_flat = in[k].c[2].n, n_lf = in[k].c[3].n;
    OdoBatchRec &r = h_recs[j];
    r.a.time_factor = d.time_factor_; r.a.no_deskew = d.no_deskew_ ? 1 : 0;
    r.st = d.d_state_.p;
    r.ls = d.less_sharp_.p; r.n_ls = int(n_ls); r.lf = d.less_flat_.p; r.n_lf = int(n_lf);
    if (n_ls + n_lf > size_t(INT_MAX)) throw CapacityError("scan-to-scan odometry: a sensor's clouds exceed 2^31 points");
    max_np = std::max(max_np, r.n_ls + r.n_lf);
    if (j >= na) continue;
    if (n_sharp + n_flat > (size_t(1) << 25)) throw CapacityError("scan-to-scan odometry: a sensor's queries exceed 2^25");   // one 64-thread block each
    if (d.n_last_corner_ + d.n_last_surf_ > size_t(INT_MAX)) throw CapacityError("scan-to-scan odometry: a sensor's previous clouds exceed 2^31 points");
    const int nq = int(n_sharp + n_flat);
    r.idx_off = int(idx_total); r.part_off = int(part_total); r.trace_off = j * max_iter * 8;
    r.nb = std::max(1, std::min(cdiv(nq, ODO_ROW_THREADS), 64));
    idx_total += 2 * n_sharp + 3 * n_flat; part_total += size_t(r.nb);
    if (idx_total > size_t(INT_MAX)) throw CapacityError("scan-to-scan odometry: the index table exceeds 2^31 entries");
    max_nq = std::max(max_nq, nq); max_nb = std::max(max_nb, r.nb);
    r.a.sharp = d.sharp_.p; r.a.nc = int(n_sharp); r.a.flat = d.flat_.p; r.a.ns = int(n_flat);
    r.a.lastc = d.last_corner_.p; r.a.nlc = int(d.n_last_corner_); r.a.lasts = d.last_surf_.p; r.a.nls = int(d.n_last_surf_);
    grids.add(r.a.lastc, r.a.nlc);
    grids.add(r.a.lasts, r.a.nls);
  }
  if (!na) return;
  d_idx.reserve(std::max<size_t>(idx_total, 1));
  if (idx_total) LIO_HIP(hipMemsetAsync(d_idx.p, 0xFF, idx_total * sizeof(int), s));
  d_partials.reserve(part_total * 28);
}

// ---- step 3: kdtree_corner_last_ / kdtree_surf_last_->setInputCloud (PointOdometry.cc:673-676) as 5 m grids over the previous clouds of `act`,
// and the finished table on the device.  The bounds of all 2 * nA clouds come back in one read-back behind the upload of the clouds' own
// records; every grid of at most LIO_ODOM_BATCH_GRID_CELLS_MAX cells is then built by `grids` behind the second upload, a larger
// one by its sensor's own KnnGrid.
void OdoChain::MakeGrids() {
  const int na = nA();
  if (na) {
    const VoxParams *b = grids.bounds(s);
    const float cell = 5.0f * 1.0001f;
    grids.layout(cell, size_t(LIO_ODOM_BATCH_GRID_CELLS_MAX));
    for (int j = 0; j < na; ++j) {
      OdometryDev &d = dev(j);
      OdoArgs &a = h_recs[j].a;
      for (int c = 0; c < 2; ++c) {
        const int i = 2 * j + c;
        KnnGrid &own = c ? d.grid_s_ : d.grid_c_;
        if (!grids.shared(i)) own.build(c ? a.lasts : a.lastc, size_t(c ? a.nls : a.nlc), b[i].mn, b[i].mx, cell, s);
        (c ? a.gs : a.gc) = grids.desc(i);
        (c ? a.gs_sorted : a.gc_sorted) = grids.shared(i) ? grids.sorted(i) : own.sorted();
        (c ? a.gs_cells : a.gc_cells) = grids.shared(i) ? grids.cells(i) : own.cells();
      }
    }
  }
  grids.build(s);
}

// ---- step 4: the <= max_iter iterations of `act` (:325-651).  The host looks at the sensors' mailboxes where the reference refreshes the
// correspondences (iter % 5 == 0); the look ends the loop only when EVERY sensor has converged (one that converged earlier stays frozen: its
// kernels leave at once).  Leaves every sensor's last state in `got`.
void OdoChain::Iterate() {
  const int na = nA();
  d_trace.reserve(size_t(na) * size_t(max_iter) * 8);
  mail.reserve(na);
  got.assign(size_t(na), OdomState{});
  auto read_mail = [&] {
    for (int j = 0; j < na; ++j) got[size_t(j)] = mail.slot(j);
    return mail.all_converged(na);
  };
  bool have_state = false;
  for (int iter = 0; iter < max_iter; ++iter) {
    if (iter > 0 && iter % 5 == 0) {
      mail.wait(s);
      if (read_mail()) { have_state = true; break; }
    }
    if (iter % 5 == 0 && max_nq > 0) hipLaunchKernelGGL(k_ob_corr, dim3(max_nq, na), dim3(64), 0, s, d_recs, d_idx.p);
    hipLaunchKernelGGL(k_ob_rows, dim3(max_nb, na), dim3(ODO_ROW_THREADS), 0, s, d_recs, d_idx.p, iter, d_partials.p);
    HostSignal sg{};
    if (iter % 5 == 4 || iter == max_iter - 1) sg = mail.arm(na);
    hipLaunchKernelGGL(k_ob_update, dim3(na), dim3(256), 0, s, d_recs, d_partials.p, iter, mail.base(), sg, d_trace.p);
  }
  LIO_HIP(hipGetLastError());
  if (!have_state) {   // the last iteration posted (max_iter >= 1)
    mail.wait(s);
    read_mail();
  }
}

// ---- step 5: the iterations' records (lio_odom_get_iteration_trace), what the host keeps of the states (:654-663), TransformToEnd of the
// less-sharp and less-flat clouds (:660-661)
void OdoChain::Finish() {
  const int na = nA(), ne = nE();
  if (na) {
    // every sensor's records in one copy (every launch behind them is complete: the states came back; iters >= 1 for each)
    h_trace.resize(size_t(na) * size_t(max_iter) * 8);
    LIO_HIP(hipMemcpyAsync(h_trace.data(), d_trace.p, h_trace.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    LIO_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < na; ++j) {
      st[size_t(act[size_t(j)])] = got[size_t(j)];
      for (int i = 0; i < got[size_t(j)].iters; ++i) {
        const float *T = &h_trace[size_t(h_recs[j].trace_off) + size_t(i) * 8];
        dev(j).es_trace_.push_back(Rigid<float>(Quat<float>(T[3], T[0], T[1], T[2]), Vec3<float>(T[4], T[5], T[6])));
      }
    }
  }
  // (a sensor of `idle` keeps the state it was given: nothing ran on it)
  for (int j = 0; j < ne; ++j) dev(j).Accumulate(st[size_t(who(j))]);
  if (max_np) hipLaunchKernelGGL(k_ob_to_end, dim3(cdiv(max_np, 256), ne), dim3(256), 0, s, d_recs);
  LIO_HIP(hipGetLastError());
}

void OdometryDev::Process(const float *sharp, size_t n_sharp, const float *less_sharp, size_t n_ls, const float *flat, size_t n_flat,
                          const float *less_flat, size_t n_lf) {
  OdometryDev *self = this;
  const Clouds in{{CloudSrc::host(sharp, n_sharp), CloudSrc::host(less_sharp, n_ls), CloudSrc::host(flat, n_flat), CloudSrc::host(less_flat, n_lf)}};
  ProcessBatch(&self, 1, &in);
}

void OdometryDev::ProcessBatch(OdometryDev *const *o, int n, const Clouds *in) {
  for (int k = 1; k < n; ++k)
    if (o[k]->max_iter_ != o[0]->max_iter_) {   // no common iteration count: no common chain, a chain of one per handle
      for (int j = 0; j < n; ++j) ProcessBatch(o + j, 1, in + j);
      return;
    }
  OdoChain &ch = o[0]->Chain();
  ch.Begin(o, n);
  ch.TakeClouds(n, in);
  if (ch.nE()) {
    ch.FillTable(in);
    ch.MakeGrids();
    if (ch.nA()) ch.Iterate();
    ch.Finish();
  }
  LIO_HIP(hipStreamSynchronize(ch.s));
  for (int k = 0; k < n; ++k) {
    OdometryDev &d = *o[k];
    std::swap(d.last_corner_, d.less_sharp_); std::swap(d.last_surf_, d.less_flat_);
    d.n_last_corner_ = in[k].c[1].n; d.n_last_surf_ = in[k].c[3].n;
    d.inited_ = true;
  }
}

// The test hooks' table (include/lio_test_hooks.h): the given clouds as this handle's queries and previous clouds, the given transform_es_
// as its state, and the table and grids of a chain of one that iterates — whatever the previous clouds' sizes: the gate on them is
// TakeClouds's, for Process alone.  Meant for a handle of its own: the clouds it leaves behind are the caller's.  Returns synchronised (the
// bounds' read-back): `T` and the caller's arrays have been read.
OdoChain &OdometryDev::HookTable(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_lc,
                                 const float *last_surf, size_t n_lsf, const Rigid<float> &T) {
  OdometryDev *self = this;
  OdoChain &ch = Chain();
  ch.Begin(&self, 1);
  const Clouds in{{CloudSrc::host(sharp, n_sharp), CloudSrc(), CloudSrc::host(flat, n_flat), CloudSrc()}};   // (no less-sharp, no less-flat cloud)
  upload(sharp_, in.c[0], ch.s);
  upload(flat_, in.c[2], ch.s);
  upload(last_corner_, CloudSrc::host(last_corner, n_lc), ch.s);
  upload(last_surf_, CloudSrc::host(last_surf, n_lsf), ch.s);
  n_last_corner_ = n_lc; n_last_surf_ = n_lsf;
  ch.st[0] = odom_state_at(T);
  LIO_HIP(hipMemcpyAsync(d_state_.p, &ch.st[0], sizeof(OdomState), hipMemcpyHostToDevice, ch.s));
  ch.act.push_back(0);
  ch.FillTable(&in);
  ch.MakeGrids();
  return ch;
}

// lio_odom_correspondences (include/lio_test_hooks.h): ONE launch of k_ob_corr over the hook's table, as the first iteration of Process
// launches it, and sel of every query from k_odo_sel
void OdometryDev::Correspondences(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_lc,
                                  const float *last_surf, size_t n_lsf, const Rigid<float> &T, int32_t *corner_idx, int32_t *surf_idx,
                                  float *sel_out) {
  OdoChain &ch = HookTable(sharp, n_sharp, flat, n_flat, last_corner, n_lc, last_surf, n_lsf, T);
  hipStream_t s = ch.s;
  const size_t nq = n_sharp + n_flat;
  if (ch.max_nq > 0) hipLaunchKernelGGL(k_ob_corr, dim3(ch.max_nq, 1), dim3(64), 0, s, ch.d_recs, ch.d_idx.p);
  d_sel_.reserve(std::max<size_t>(3 * nq, 1));
  if (nq) hipLaunchKernelGGL(k_odo_sel, dim3(cdiv(nq, 256)), dim3(256), 0, s, ch.h_recs[0].a, d_state_.p, d_sel_.p);
  LIO_HIP(hipGetLastError());
  static_assert(sizeof(int) == sizeof(int32_t), "index layout");
  if (n_sharp) LIO_HIP(hipMemcpyAsync(corner_idx, ch.d_idx.p, 2 * n_sharp * sizeof(int), hipMemcpyDeviceToHost, s));
  if (n_flat) LIO_HIP(hipMemcpyAsync(surf_idx, ch.d_idx.p + 2 * n_sharp, 3 * n_flat * sizeof(int), hipMemcpyDeviceToHost, s));
  if (nq) LIO_HIP(hipMemcpyAsync(sel_out, d_sel_.p, 3 * nq * sizeof(float), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
}

// lio_gn_rows_odom (include/lio_test_hooks.h): the given correspondences in the place of the search's, ONE launch of k_ob_rows over the hook's
// table at the given iteration, as Process launches it, and the row of every query from k_gn_rows_odom.  The caller has checked the indices
// against the clouds' sizes.
void OdometryDev::Rows(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_lc,
                       const float *last_surf, size_t n_lsf, const int32_t *corner_idx, const int32_t *surf_idx, const Rigid<float> &T, int iter,
                       uint8_t *ok_out, float *rows_out, int32_t *nb_out, double *partials_out) {
  OdoChain &ch = HookTable(sharp, n_sharp, flat, n_flat, last_corner, n_lc, last_surf, n_lsf, T);
  hipStream_t s = ch.s;
  const size_t nq = n_sharp + n_flat;
  static_assert(sizeof(int) == sizeof(int32_t), "index layout");
  if (n_sharp) LIO_HIP(hipMemcpyAsync(ch.d_idx.p, corner_idx, 2 * n_sharp * sizeof(int), hipMemcpyHostToDevice, s));
  if (n_flat) LIO_HIP(hipMemcpyAsync(ch.d_idx.p + 2 * n_sharp, surf_idx, 3 * n_flat * sizeof(int), hipMemcpyHostToDevice, s));
  const int nb = ch.max_nb;
  hipLaunchKernelGGL(k_ob_rows, dim3(nb, 1), dim3(ODO_ROW_THREADS), 0, s, ch.d_recs, ch.d_idx.p, iter, ch.d_partials.p);
  d_sel_.reserve(std::max<size_t>(7 * nq, 1));
  DBuf<uint8_t> ok_dev;
  ok_dev.reserve(std::max<size_t>(nq, 1));
  if (nq) hipLaunchKernelGGL(k_gn_rows_odom, dim3(cdiv(nq, 256)), dim3(256), 0, s, ch.h_recs[0].a, d_state_.p, ch.d_idx.p, iter, ok_dev.p, d_sel_.p);
  LIO_HIP(hipGetLastError());
  if (nq) {
    LIO_HIP(hipMemcpyAsync(ok_out, ok_dev.p, nq, hipMemcpyDeviceToHost, s));
    LIO_HIP(hipMemcpyAsync(rows_out, d_sel_.p, 7 * nq * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  LIO_HIP(hipMemcpyAsync(partials_out, ch.d_partials.p, size_t(nb) * 28 * sizeof(double), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));   // the caller's index arrays have been read
  *nb_out = nb;
}

// TransformToEnd(full_cloud_) of a publishing step (:725-730): the same kernel and the same device-side transform_es_ as the
// less-sharp / less-flat clouds of the last Process.  A byte copy while the odometry is disabled (:727) and before the first
// publishing step: the first Process returns at :302-310 without publishing, so nothing has touched the cloud.
void OdometryDev::FullToEnd(const float *xyzi, size_t n, float *out) {
  if (!n) return;
  if (!enable_odom_ || !to_end_ready_) {
    if (out != xyzi) std::memmove(out, xyzi, n * sizeof(float4));
    return;
  }
  hipStream_t s = stream_;
  upload(full_, CloudSrc::host(xyzi, n), s);
  hipLaunchKernelGGL(k_odo_to_end, dim3(cdiv(n, 256)), dim3(256), 0, s, full_.p, full_.p, int(n), d_state_.p, time_factor_, no_deskew_ ? 1 : 0);
  LIO_HIP(hipGetLastError());
  LIO_HIP(hipMemcpyAsync(out, full_.p, n * sizeof(float4), hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
}

size_t OdometryDev::GetLastCloud(int which, float *out) {
  const DBuf<float4> &b = which == 0 ? last_corner_ : last_surf_;
  const size_t n = which == 0 ? n_last_corner_ : n_last_surf_;
  if (out && n) {
    LIO_HIP(hipMemcpyAsync(out, b.p, n * sizeof(float4), hipMemcpyDeviceToHost, stream_));
    LIO_HIP(hipStreamSynchronize(stream_));
  }
  return n;
}

}  // namespace lio
