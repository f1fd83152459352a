// est_batch.hip — host orchestration of the batched solve (see est_batch.h).  The kernels: batch_kernels.hip (map / feature stages),
// seg_vox.hip (the voxel filter of the local maps and of the pushed sweeps), solve_kernels.hip (launch A / launch B of the trust-region loop), marg_kernels.hip (marginalization).
#include "est_batch.h"
#include "../../include/lio_test_hooks.h"

#include <algorithm>
#include <atomic>
#include <exception>
#include <string>
#include <thread>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace lio {

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

EstimatorBatch::EstimatorBatch(const std::vector<Estimator *> &members) : m_(members) {
  // the argument checks come before anything is created: Close() walks m_ and the pinned staging is sized by B >= 1
  if (m_.empty()) throw std::runtime_error("EstimatorBatch: no windows");
  for (Estimator *e : m_) if (!e) throw std::runtime_error("EstimatorBatch: null window");
  try { Init(); } catch (...) { Close(); throw; }   // (a constructor that throws does not run the destructor)
}
void EstimatorBatch::Init() {
  const size_t B = m_.size();
  // one device per batch: the members' buffers, this batch's streams and the kernels' per-device attributes (hipFuncSetAttribute
  // applies to the current device only) all belong to the device the windows were created on
  device_id_ = m_[0]->device_id_;
  for (Estimator *e : m_) if (e->device_id_ != device_id_) throw std::runtime_error("EstimatorBatch: windows of different devices");
  LIO_HIP(hipSetDevice(device_id_));
  prepare_bw_step_kernel();
  prepare_bw_marg_kernel();
  prepare_seg_sort_kernels();
  ok_.assign(B, 0);
  LIO_HIP(hipStreamCreate(&stream_));
  for (hipEvent_t &e : ev_) LIO_HIP(hipEventCreate(&e));
  for (hipEvent_t &e : ev_wait_) LIO_HIP(hipEventCreate(&e));
  for (hipStream_t &g : stream_grp_) LIO_HIP(hipStreamCreate(&g));
  LIO_HIP(hipStreamCreate(&stream_marg_));
  LIO_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
  LIO_HIP(hipEventCreateWithFlags(&ev_marg_, hipEventDisableTiming));
  for (hipEvent_t &e : ev_grp_) LIO_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  win_.resize(B);
  for (size_t w = 0; w < B; ++w) { win_[w].e = m_[w]; m_[w]->AdoptStream(stream_); }
  const auto pin = [](auto &h, size_t n) { h.alloc(n, hipHostMallocDefault, true); };   // zero-filled; B >= 1: no empty allocation
  pin(h_win_, B); pin(h_grid_, B); pin(h_odom_, B); pin(h_bs_, B); pin(h_pb_, B); pin(h_st_, B); pin(h_mg_, B);
  pin(h_prior_, B * ds_prior_mats_size(MARG_MAX_N)); pin(h_nconv_, 4); pin(h_seg_, B);
  d_win_.reserve(B); d_grid_.reserve(B); d_odom_.reserve(B); d_bs_.reserve(B); d_pb_.reserve(B); d_st_.reserve(B); d_mg_.reserve(B);
  nconv_.reserve(4); d_seg_.reserve(B);
  vox_.reserve(0, 2 * int(B), stream_);   // (the tables of a push with the map refresh on: no pinned allocation inside a call)
  LIO_HIP(hipMemsetAsync(d_mg_.p, 0, sizeof(DevMarg) * d_mg_.cap, stream_));
  // the scratch slab of a window (doubles)
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 7) & ~size_t(7); return at; };
  lay_.prior[0] = take(ds_prior_mats_size(MARG_MAX_N)); lay_.prior[1] = take(ds_prior_mats_size(MARG_MAX_N));
  lay_.imu = take(size_t(DS_MAX_WO) * DS_IMU_OUT); lay_.lmap = take(size_t(DS_MAX_WO) * DS_LMAP_OUT);
  lay_.prior_out = take(MARG_MAX_N + 8); lay_.exprior = take(DS_EXP_OUT);
  lay_.Hcur = take(size_t(DS_MAX_NPAD) * (DS_MAX_NPAD + 1)); lay_.Sbuf = take(size_t(2) * DS_MAX_WO * LIO_MOMENT_OUT); lay_.prof = take(96);
  lay_.marg_imu = take(DS_IMU_OUT); lay_.marg_lmap = take(size_t(DS_MAX_WO) * DS_LMAP_OUT); lay_.marg_prior_out = take(MARG_MAX_N + 8);
  { const size_t N = MARG_MAX_M + MARG_MAX_N; lay_.marg_A = take(N * N + N); }
  lay_.marg_info = take(MARG_MAX_N + 8 + 16);   // sweeps (2) | eigenvalues | 8 phase stamps | 4 per-phase sums of the eigensolver (LIO_MARG_PROF builds)
  lay_.total = o;
  slab_.reserve(B * lay_.total);
  LIO_HIP(hipMemsetAsync(slab_.p, 0, sizeof(double) * slab_.cap, stream_));
  LIO_HIP(hipStreamSynchronize(stream_));
}

EstimatorBatch::~EstimatorBatch() { Close(); }
void EstimatorBatch::Close() noexcept {   // (the pinned and device buffers are members: they go after this, when both streams have drained)
  try {
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (stream_marg_) (void)hipStreamSynchronize(stream_marg_);
    for (size_t w = 0; w < win_.size(); ++w)
      for (int k = 0; k < 2; ++k) if (win_[w].dev_prior[k]) win_[w].dev_prior[k]->materialize();   // nobody may be left holding a shell
    for (Estimator *e : m_) {   // (after a partial Init(): ReleaseAdoptedStream is a no-op for a member that was never adopted)
      e->solve_hook_ = nullptr; e->ReleaseAdoptedStream();
      if (e->feat_batch_ == this) { e->feat_batch_ = nullptr; e->feat_batch_w_ = -1; }   // (its getter falls back to the handle's own slots)
    }
  } catch (...) {}
  for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_wait_) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_k_) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_grp_) if (e) (void)hipEventDestroy(e);
  if (ev_fork_) (void)hipEventDestroy(ev_fork_);
  if (ev_marg_) (void)hipEventDestroy(ev_marg_);
  if (ev_slide_) (void)hipEventDestroy(ev_slide_);
  for (hipStream_t g : stream_grp_) if (g) (void)hipStreamDestroy(g);
  if (stream_marg_) (void)hipStreamDestroy(stream_marg_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

bool EstimatorBatch::SetOption(const char *name, int v) {
  if (!name) return false;
  const std::string n(name);
  if (n == "lanes_per_query") { if (v != 0 && v != 1 && v != 4 && v != 8) return false; knobs_.lanes_per_query = v; }
  else if (n == "loop_groups") { if (v < 0 || v > kGroups) return false; knobs_.loop_groups = v; }
  else if (n == "aux_threads") { if (v != 0 && v != 64 && v != 128 && v != 256) return false; knobs_.aux_threads = v; }
  else if (n == "finish_threads") { if (v < 0 || v > 8) return false; knobs_.finish_threads = v; }
  else if (n == "time_kernels") { if (v != 0 && v != 1) return false; knobs_.time_kernels = v; }
  else return false;
  return true;
}

const BatchClock &EstimatorBatch::clock() {
  if (ev_valid_) {
    LIO_HIP(hipStreamSynchronize(stream_));
    LIO_HIP(hipStreamSynchronize(stream_marg_));
    for (int k = 0; k < 6; ++k) {
      float ms = 0;
      clk_.dev[k] = hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]) == hipSuccess ? double(ms) : 0.0;
    }
    clk_.dev_marg_wait = 0;
    if (ev_wait_valid_) {   // the rounds' stage minus the wait for the previous marginalization: what the rounds themselves took
      float ms = 0;
      clk_.dev_marg_wait = hipEventElapsedTime(&ms, ev_wait_[0], ev_wait_[1]) == hipSuccess ? double(ms) : 0.0;
      clk_.dev[3] = std::max(0.0, clk_.dev[3] - clk_.dev_marg_wait);
    }
    for (int k = 0; k < 3; ++k) { clk_.kernel_ms[k] = 0; clk_.kernel_launches[k] = 0; }
    for (int q = 0; q + 3 < ev_k_used_; q += 4)
      for (int k = 0; k < 3; ++k) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev_k_[size_t(q + k)], ev_k_[size_t(q + k + 1)]) == hipSuccess) { clk_.kernel_ms[k] += double(ms); ++clk_.kernel_launches[k]; }
      }
    ev_k_used_ = 0;
    ev_valid_ = false; ev_wait_valid_ = false;
  }
  return clk_;
}

void EstimatorBatch::Sync() {
  LIO_HIP(hipStreamSynchronize(stream_));
  LIO_HIP(hipStreamSynchronize(stream_marg_));
}

// the matrices of the prior held in device buffer `buf` of window w -> pr (the fetch of a MargPrior shell)
void EstimatorBatch::FetchPrior(int w, int buf, MargPrior &pr) {
  const size_t n = size_t(pr.n);
  std::vector<double> h(ds_prior_mats_size(pr.n));
  Sync();
  LIO_HIP(hipMemcpy(h.data(), slab_.p + size_t(w) * lay_.total + lay_.prior[buf], h.size() * sizeof(double), hipMemcpyDeviceToHost));
  pr.JtJ = DMat(pr.n, pr.n); pr.lin_jac = DMat(pr.n, pr.n); pr.lin_res.assign(n, 0.0); pr.Jtr0.assign(n, 0.0);
  std::memcpy(pr.JtJ.a.data(), h.data(), sizeof(double) * n * n);
  std::memcpy(pr.lin_jac.a.data(), h.data() + n * n, sizeof(double) * n * n);
  std::memcpy(pr.lin_res.data(), h.data() + 2 * n * n, sizeof(double) * n);
  std::memcpy(pr.Jtr0.data(), h.data() + 2 * n * n + n, sizeof(double) * n);
}
// buffer `buf` of window w is about to be overwritten: whoever else still holds its prior as a shell gets the matrices first
void EstimatorBatch::Materialize(int w, int buf) {
  std::shared_ptr<MargPrior> &p = win_[w].dev_prior[buf];
  if (p && p->on_device && p.use_count() > 1) p->materialize();
  p.reset();
}

// ---- test hook: per-window digests of a stage's device arrays (est_batch.h)
static unsigned long long fnv1a(const void *p, size_t n, unsigned long long h = 1469598103934665603ull) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
static unsigned long long mix64(unsigned long long x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
template <typename T> static std::vector<T> fetch(const T *d, size_t n) {
  std::vector<T> h(std::max<size_t>(n, 1));
  if (n) LIO_HIP(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}
void EstimatorBatch::StageDigest(int stage, unsigned long long *out) {
  Sync();
  for (hipStream_t g : stream_grp_) LIO_HIP(hipStreamSynchronize(g));
  const int B = size();
  for (int w = 0; w < B; ++w) {
    const BatchWin &bw = h_win_.p[w];
    const BatchGrid &G = h_grid_.p[w];
    unsigned long long h = 0;
    switch (stage) {
      case 0: {
        const std::vector<float4> p = fetch(filtered_all_.p + bw.vox.off, size_t(G.n_filtered));
        h = fnv1a(p.data(), size_t(G.n_filtered) * sizeof(float4), mix64(G.n_filtered));
        break;
      }
      case 1: {
        size_t ncells = size_t(G.g.dims[0]) * G.g.dims[1] * G.g.dims[2];
        const std::vector<int> c = fetch(cells_all_.p + G.cell_off, ncells + 1);
        const std::vector<float4> p = fetch(sorted_all_.p + c[0], size_t(G.n_filtered));
        h = mix64(ncells);
        for (size_t k = 0; k < ncells; ++k) {
          unsigned long long run = 0;   // a cell's points as a multiset
          for (int j = c[k] - c[0]; j < c[k + 1] - c[0]; ++j) run += mix64(fnv1a(&p[size_t(j)], sizeof(float4)));
          const int rel[2] = {c[k] - c[0], c[k + 1] - c[0]};
          if (rel[1] != rel[0]) h = mix64(h ^ fnv1a(rel, sizeof(rel)) ^ run ^ mix64(k));
        }
        break;
      }
      case 2: {
        const std::vector<uint8_t> v = fetch(valid_all_.p + bw.slot_base, size_t(bw.n_slots));
        h = fnv1a(v.data(), size_t(bw.n_slots), mix64(bw.n_slots));
        break;
      }
      case 3: {
        const std::vector<uint8_t> v = fetch(valid_all_.p + bw.slot_base, size_t(bw.n_slots));
        const std::vector<float4> c = fetch(coef_all_.p + bw.slot_base, size_t(bw.n_slots));
        h = mix64(bw.n_slots);
        for (int k = 0; k < bw.n_slots; ++k) if (v[size_t(k)]) h = fnv1a(&c[size_t(k)], sizeof(float4), h ^ mix64(k));
        break;
      }
      case 4: { const std::vector<OdomState> o = fetch(d_odom_.p + w, 1); h = fnv1a(o.data(), sizeof(OdomState)); break; }
      case 5: { const std::vector<DevState> o = fetch(d_st_.p + w, 1); h = fnv1a(o.data(), sizeof(DevState)); break; }
      case 8: {   // scaled H at the accepted point (upper triangle), + on stderr whether it is positive definite
        const DevProblem &pb = h_pb_.p[w];
        const int n = pb.n, ld = pb.ld;
        const std::vector<double> Hc = fetch(slab_.p + size_t(w) * lay_.total + lay_.Hcur, size_t(pb.n_pad) * ld);
        h = mix64(n);
        std::vector<double> M(size_t(n) * n);
        for (int r = 0; r < n; ++r) { h = fnv1a(&Hc[size_t(r) * ld + r], sizeof(double) * (n - r), h); for (int c = r; c < n; ++c) M[size_t(r) * n + c] = M[size_t(c) * n + r] = Hc[size_t(r) * ld + c]; }
        if (std::getenv("LIO_DEBUG_DIGEST")) {
          int bad = -1; double dmin = 1e300, dmax = 0; bool finite = true;
          for (double v : M) if (!std::isfinite(v)) finite = false;
          for (int j = 0; j < n && bad < 0; ++j) {   // plain Cholesky of H + 1e-8 diag(H)
            double d = M[size_t(j) * n + j] * (1.0 + 1e-8);
            for (int k = 0; k < j; ++k) d -= M[size_t(j) * n + k] * M[size_t(j) * n + k];
            if (!(d > 0)) { bad = j; break; }
            dmin = std::min(dmin, d); dmax = std::max(dmax, d);
            const double l = std::sqrt(d);
            M[size_t(j) * n + j] = l;
            for (int r = j + 1; r < n; ++r) { double v = M[size_t(r) * n + j]; for (int k = 0; k < j; ++k) v -= M[size_t(r) * n + k] * M[size_t(j) * n + k]; M[size_t(r) * n + j] = v / l; }
          }
          std::fprintf(stderr, "[digest] window %d: H_cur %016llx finite %d cholesky %s (pivot %d) pivots in [%.3e, %.3e]\n", w, h, int(finite), bad < 0 ? "ok" : "FAILS", bad, dmin, dmax);
        }
        break;
      }
      case 9: {   // marginalization: sweeps and phase stamps of the last launch (stderr under LIO_DEBUG_DIGEST); digest of the new prior
        const std::vector<double> mi = fetch(slab_.p + size_t(w) * lay_.total + lay_.marg_info, MARG_MAX_N + 24);
        const std::vector<double> pm = fetch(slab_.p + size_t(w) * lay_.total + lay_.prior[1 - win_[w].cur], ds_prior_mats_size(h_mg_.p[w].n));
        h = fnv1a(pm.data(), pm.size() * sizeof(double), mix64(h_mg_.p[w].n));
        if (std::getenv("LIO_DEBUG_DIGEST") && (w == 0 || w == B - 1))
          std::fprintf(stderr, "[digest] window %d marginalization: m %d n %d QL sweeps %g / %g; shader clocks: assembly %.0f, Amm eig %.0f, pinv + T + S %.0f, S eig %.0f, factors out %.0f, J^T J %.0f\n",
                       w, h_mg_.p[w].m, h_mg_.p[w].n, mi[0], mi[1], mi[MARG_MAX_N + 9] - mi[MARG_MAX_N + 8], mi[MARG_MAX_N + 10] - mi[MARG_MAX_N + 9], mi[MARG_MAX_N + 11] - mi[MARG_MAX_N + 10], mi[MARG_MAX_N + 12] - mi[MARG_MAX_N + 11],
                       mi[MARG_MAX_N + 13] - mi[MARG_MAX_N + 12], mi[MARG_MAX_N + 14] - mi[MARG_MAX_N + 13]);
        if (std::getenv("LIO_DEBUG_DIGEST") && w == 0 && mi[MARG_MAX_N + 16] != 0.0)
          std::fprintf(stderr, "[digest] S eig, thread 0: reduction %.0f, QL %.0f of which wave 0's recurrence %.0f, its waits at the sweeps' barriers %.0f\n", mi[MARG_MAX_N + 16], mi[MARG_MAX_N + 19], mi[MARG_MAX_N + 17], mi[MARG_MAX_N + 18]);
        break;
      }
      case 7: { const std::vector<DevState> o = fetch(d_st_.p + w, 1); h = fnv1a(o[0].scale, sizeof(o[0].scale)); break; }
      case 6: {
        const Win &Wn = win_[w];
        const size_t n = Wn.device ? size_t(Wn.e->Wo_) * Wn.bpf * LIO_MOMENT_OUT : 0;
        const std::vector<double> o = fetch(partials_.p + Wn.part_off, n);
        h = mix64(n);
        for (size_t r = 0; r + LIO_MOMENT_OUT <= n; r += LIO_MOMENT_OUT) h = fnv1a(o.data() + r, 258 * sizeof(double), h);   // (the last two words of a row are never written)
        break;
      }
      default: throw std::runtime_error("EstimatorBatch::StageDigest: unknown stage");
    }
    out[w] = h;
  }
}

bool EstimatorBatch::GetMoments(int w, double *out, double *Rt) {
  if (w < 0 || w >= size() || !win_[size_t(w)].device) return false;
  Sync();
  for (hipStream_t g : stream_grp_) LIO_HIP(hipStreamSynchronize(g));
  const Estimator *e = win_[size_t(w)].e;
  const int Wo = e->Wo_;
  const std::vector<DevState> st = fetch(d_st_.p + w, 1);
  const std::vector<double> S = fetch(slab_.p + size_t(w) * lay_.total + lay_.Sbuf + size_t(st[0].s_cur) * Wo * LIO_MOMENT_OUT, size_t(Wo) * LIO_MOMENT_OUT);
  for (int f = 0; f < Wo; ++f) {
    std::memcpy(out + size_t(f) * 258, S.data() + size_t(f) * LIO_MOMENT_OUT, 258 * sizeof(double));
    relative_lidar_pose(st[0].x.pose[0], st[0].x.pose[f + 1], st[0].x.ex, Rt + size_t(f) * 12, Rt + size_t(f) * 12 + 9);
  }
  return true;
}

bool EstimatorBatch::GetLinearization(int w, int32_t *ints, double *problem, double *state, double *aux) {
  if (w < 0 || w >= size() || !win_[size_t(w)].device) return false;
  Sync();
  for (hipStream_t g : stream_grp_) LIO_HIP(hipStreamSynchronize(g));
  std::fill(ints, ints + LIO_DSL_INTS, 0);
  std::fill(problem, problem + LIO_DSL_PROBLEM, 0.0);
  std::fill(state, state + LIO_DSL_STATE, 0.0);
  std::fill(aux, aux + LIO_DSL_AUX, 0.0);
  const std::vector<DevProblem> pbv = fetch(d_pb_.p + w, 1);
  const std::vector<DevState> stv = fetch(d_st_.p + w, 1);
  const DevProblem &pb = pbv[0];
  const DevState &st = stv[0];
  const double *slab = slab_.p + size_t(w) * lay_.total;
  const int Wo = pb.Wo, n = pb.n, np = pb.n_prior;
  const int iv[16] = {Wo, n, pb.ex_col, np, pb.have_prior, pb.use_ex_prior, pb.n_keep, st.it, st.successful, st.termination, st.need_host, st.ntrace,
                      pb.n_pad, st.started, st.done, pb.max_iterations};
  std::copy(iv, iv + 16, ints);
  for (int i = 0; i < DS_MAX_NPAD; ++i) ints[16 + i] = pb.prior_col[i];
  for (int b = 0; b < DS_MAX_KEEP; ++b) {
    int32_t *k = ints + 144 + 5 * b;
    k[0] = pb.keep_kind[b]; k[1] = pb.keep_index[b]; k[2] = pb.keep_size[b]; k[3] = pb.keep_idx[b]; k[4] = pb.keep_x0[b];
  }
  std::copy(pb.prior_x0, pb.prior_x0 + DS_MAX_KEEP * 9, problem);
  std::copy(pb.ex_prior_pos, pb.ex_prior_pos + 3, problem + 90);
  std::copy(pb.ex_prior_rot, pb.ex_prior_rot + 4, problem + 93);
  for (int i = 0; i < DS_MAX_WO; ++i) {
    const DevPim &pm = pb.pim[i];
    ints[194 + i] = pm.present;
    double *o = problem + 97 + 470 * i;
    std::copy(pm.dp, pm.dp + 3, o); std::copy(pm.dq, pm.dq + 4, o + 3); std::copy(pm.dv, pm.dv + 3, o + 7); std::copy(pm.ba, pm.ba + 3, o + 10);
    std::copy(pm.bg, pm.bg + 3, o + 13); std::copy(pm.g, pm.g + 3, o + 16); o[19] = pm.sum_dt;
    std::copy(pm.jac, pm.jac + 225, o + 20); std::copy(pm.sqrt_info, pm.sqrt_info + 225, o + 245);
  }
  if (pb.have_prior && np > 0 && np <= MARG_MAX_N) {
    const std::vector<double> pm = fetch(slab + lay_.prior[win_[size_t(w)].cur], ds_prior_mats_size(np));
    std::copy(pm.begin(), pm.end(), problem + 3387);
  }
  auto params = [](const DevParams &P, double *o) {
    std::copy(&P.pose[0][0], &P.pose[0][0] + (DS_MAX_WO + 1) * 7, o);
    std::copy(&P.sb[0][0], &P.sb[0][0] + (DS_MAX_WO + 1) * 9, o + 56);
    std::copy(P.ex, P.ex + 7, o + 128);
  };
  params(st.x, state); params(st.cand, state + 135);
  std::copy(&st.cand_Rt[0][0], &st.cand_Rt[0][0] + DS_MAX_WO * 12, state + 270);
  std::copy(st.scale, st.scale + DS_MAX_NPAD, state + 354);
  std::copy(st.g, st.g + DS_MAX_NPAD, state + 482);
  std::copy(st.costs0, st.costs0 + 4, state + 610);
  std::copy(st.trace, st.trace + 40, state + 614);
  const double sc[10] = {st.radius, st.mu, st.alpha, st.dogleg_norm, st.model_change, st.step_norm, st.x_cost, st.x_norm, st.gmax, st.n_lidar};
  std::copy(sc, sc + 10, state + 654);
  {
    const int ld = pb.ld;
    const std::vector<double> Hc = fetch(slab + lay_.Hcur, size_t(pb.n_pad) * ld);
    for (int r = 0; r < n; ++r)
      for (int c = r; c < n; ++c) state[664 + size_t(r) * n + c] = state[664 + size_t(c) * n + r] = Hc[size_t(r) * ld + c];
  }
  {
    const std::vector<double> a = fetch(slab + lay_.imu, size_t(Wo) * DS_IMU_OUT);
    std::copy(a.begin(), a.begin() + size_t(Wo) * DS_IMU_OUT, aux);
    const std::vector<double> l = fetch(slab + lay_.lmap, size_t(Wo) * DS_LMAP_OUT);
    std::copy(l.begin(), l.begin() + size_t(Wo) * DS_LMAP_OUT, aux + 6524);
    if (pb.have_prior && np > 0 && np <= MARG_MAX_N) {
      const std::vector<double> p = fetch(slab + lay_.prior_out, size_t(np) + 1);
      std::copy(p.begin(), p.begin() + np + 1, aux + 8260);
    }
    if (pb.use_ex_prior) {
      const std::vector<double> x = fetch(slab + lay_.exprior, DS_EXP_OUT);
      std::copy(x.begin(), x.begin() + DS_EXP_OUT, aux + 8341);
    }
    // launch B folds into the slot that is NOT s_cur and then flips s_cur when the folded point becomes the accepted one (x == cand)
    const bool at_x = std::memcmp(&st.x, &st.cand, sizeof(DevParams)) == 0;
    const int slot = at_x ? st.s_cur : 1 - st.s_cur;
    const std::vector<double> S = fetch(slab + lay_.Sbuf + size_t(slot) * Wo * LIO_MOMENT_OUT, size_t(Wo) * LIO_MOMENT_OUT);
    for (int f = 0; f < Wo; ++f) std::copy(S.begin() + size_t(f) * LIO_MOMENT_OUT, S.begin() + size_t(f) * LIO_MOMENT_OUT + 258, aux + 8385 + size_t(f) * 258);
  }
  return true;
}

void EstimatorBatch::FeatureSlots(int w, const uint8_t **valid, const float4 **coef, const float **score) {
  Sync();
  const size_t off = size_t(h_win_.p[w].slot_base);
  *valid = valid_all_.p + off; *coef = coef_all_.p + off; *score = score_all_.p + off;
}

int EstimatorBatch::Solve(lio_solve_report *reps) {
  const double t0 = now_ms();
  const int B = size();
  hipStream_t s = stream_;
  std::vector<lio_solve_report> local;
  if (!reps) { local.resize(B); reps = local.data(); }
  std::memset(static_cast<void *>(reps), 0, sizeof(lio_solve_report) * B);
  clk_ = BatchClock();
  ev_valid_ = false;
  ev_k_used_ = 0;
  // ------------------------------------------------------------------------------------------------ describe
  int off = 0, slot = 0, part_rows = 0, max_cap = 0, max_slots = 0, max_M = 0, max_static = 0, max_nb = 0;
  long long q_static = 0, q_newest = 0;
  for (int w = 0; w < B; ++w) {
    Win &Wn = win_[w];
    Estimator *e = Wn.e;
    BatchWin &bw = h_win_.p[w];
    Wn.device = e->BatchEligible();
    Wn.prior_used.reset();
    if (Wn.device) {
      e->JoinMarg(false);
      Wn.max_slots = e->BatchDescribe(bw);
    } else {
      std::memset(&bw, 0, sizeof(bw));
      bw.vox.inv_leaf = 1.f;
    }
    bw.vox.off = off; bw.vox.cap = round_up(std::max(bw.vox.n, 1), 256); off += bw.vox.cap;
    bw.slot_base = slot; slot += round_up(bw.n_slots, 16);
    for (int k = 0; k < bw.nstatic; ++k) { bw.fr[k].slot_off += bw.slot_base; max_M = std::max(max_M, bw.fr[k].M); q_static += bw.fr[k].M; }
    bw.newest.slot_off += bw.slot_base; q_newest += bw.newest.M;
    bw.part_off = part_rows; part_rows += bw.nb_round;
    max_cap = std::max(max_cap, bw.vox.cap); max_slots = std::max(max_slots, bw.n_slots); max_static = std::max(max_static, bw.nstatic);
    max_nb = std::max(max_nb, bw.nb_round);
  }
  const size_t N = size_t(off);
  if (N > size_t(INT_MAX) / 2) throw std::runtime_error("EstimatorBatch: the batch's local maps exceed 2^30 points");
  local_all_.reserve(N, s); filtered_all_.reserve(N, s); sorted_all_.reserve(N, s);
  vox_.reserve(N, B, s);
  valid_all_.reserve(std::max(slot, 16), s); coef_all_.reserve(std::max(slot, 16), s); score_all_.reserve(std::max(slot, 16), s);
  odom_partials_.reserve(size_t(std::max(part_rows, 1)) * 28, s);
  const double t1 = now_ms();
  clk_.describe = t1 - t0;
  // ------------------------------------------------------------------------------------------------ BuildLocalMap
  LIO_HIP(hipEventRecord(ev_[0], s));
  LIO_HIP(hipMemcpyAsync(d_win_.p, h_win_.p, sizeof(BatchWin) * B, hipMemcpyHostToDevice, s));
  LIO_HIP(hipMemsetAsync(nconv_.p, 0, sizeof(int), s));
  launch_bw_setup(d_win_.p, B, max_slots, valid_all_.p, d_odom_.p, nconv_.p, s);
  // The filter's order: 9-bit passes over the keys relative to each window's bounds (pass 0 converts the stored absolute keys on the fly
  // and numbers the values); every window sorts its own range.  The host goes by what each window's keys took in its previous solve
  // (seg_vox.h: the pass rule); a window that outgrows the guess is flagged by the layout kernel and re-done by the single-window path.
  int vox_passes = 3;
  for (int w = 0; w < B; ++w) if (win_[w].device) vox_passes = std::max(vox_passes, SegVoxFilter::passes_for(win_[w].key_bits));
  launch_bw_concat_keys(d_win_.p, B, max_cap, local_all_.p, vox_.keys(), vox_.partial(), vox_.flag(), s);
  vox_.finish(&d_win_.p->vox, &h_win_.p->vox, sizeof(BatchWin), B, vox_passes, local_all_.p, filtered_all_.p, s);
  LIO_HIP(hipEventRecord(ev_[1], s));
  LIO_HIP(hipStreamSynchronize(s));
  const double t2 = now_ms();
  clk_.map = t2 - t1;
  // ------------------------------------------------------------------------------------------------ K-NN grids, features, rounds
  size_t cell_total = 0;
  int max_filtered = 0;
  for (int w = 0; w < B; ++w) {
    Win &Wn = win_[w];
    BatchGrid &G = h_grid_.p[w];
    std::memset(&G, 0, sizeof(G));
    const VoxSegOut &vo = vox_.out(w);
    size_t ncells = 1;
    G.g.dims[0] = G.g.dims[1] = G.g.dims[2] = 1;
    G.g.inv_cell = 1.f;
    if (const int kb = SegVoxFilter::bits_taken(vo.params)) Wn.key_bits = kb;   // the next solve's guess for the number of sort passes
    if (Wn.device && (vo.params.overflow || vo.flagged)) Wn.device = false;   // PCL's own index / "leaf too small" / keys beyond the passes: the single-window path has those forms
    if (Wn.device && vo.count > 0) {
      ncells = grid_extent(G.g, vo.params.mn, vo.params.mx, knn_cell_edge(Wn.e->cfg_.min_match_sq_dis));
      if (ncells > (size_t(1) << 28)) { Wn.device = false; ncells = 1; G.g.dims[0] = G.g.dims[1] = G.g.dims[2] = 1; }
      else { G.n_filtered = vo.count; G.g.n_points = vo.count; }
    }
    G.cell_off = int(cell_total);
    cell_total += ncells + 1;
    max_filtered = std::max(max_filtered, G.n_filtered);
    reps[w].n_local_map = G.n_filtered;
  }
  if (cell_total > size_t(INT_MAX)) throw std::runtime_error("EstimatorBatch: the batch's cell tables exceed 2^31 entries");
  cells_all_.reserve(cell_total, s);
  LIO_HIP(hipMemcpyAsync(d_grid_.p, h_grid_.p, sizeof(BatchGrid) * B, hipMemcpyHostToDevice, s));
  launch_bw_cell_keys(d_win_.p, d_grid_.p, B, max_filtered, filtered_all_.p, vox_.keys(), s);
  {
    // a window's filtered points ordered by cell: as many 9-bit passes as the largest table's index needs, on the filter's sort scratch
    // (the filter is done: the host has waited for it)
    SegDesc *seg = h_seg_.p;
    int bits = 1;
    for (int w = 0; w < B; ++w) {
      seg[w] = SegDesc{h_win_.p[w].vox.off, h_grid_.p[w].n_filtered, 0};
      bits = std::max(bits, bits_for(h_grid_.p[w].g.dims[0] * h_grid_.p[w].g.dims[1] * h_grid_.p[w].g.dims[2]));   // (at most 2^28 cells: checked above)
    }
    const int passes = std::max(1, (bits + SS_MAX_BITS - 1) / SS_MAX_BITS);
    const SegSortPlan plan = seg_sort_plan(seg, B, SS_MAX_BITS);
    uint32_t *hist = vox_.hist(plan.hist_entries, s);
    LIO_HIP(hipMemcpyAsync(d_seg_.p, seg, sizeof(SegDesc) * B, hipMemcpyHostToDevice, s));
    const SegSortPair sorted = seg_sort_passes(d_seg_.p, B, plan, vox_.keys(), nullptr, vox_.ping(), vox_.pong(), hist, SS_MAX_BITS, passes, nullptr, s);
    launch_bw_cell_table(d_win_.p, d_grid_.p, B, max_filtered, filtered_all_.p, sorted.keys, sorted.vals, cells_all_.p, sorted_all_.p, s);
  }
  LIO_HIP(hipEventRecord(ev_[2], s));
  launch_bw_features(d_win_.p, d_grid_.p, B, max_M, max_static, q_static, knobs_, sorted_all_.p, cells_all_.p, valid_all_.p, coef_all_.p, score_all_.p, s);
  LIO_HIP(hipEventRecord(ev_[3], s));
  int round = 0;
  for (; round < 3; ++round)
    launch_bw_odom_round(d_win_.p, d_grid_.p, B, max_nb, q_newest, knobs_, round, d_odom_.p, sorted_all_.p, cells_all_.p, valid_all_.p, coef_all_.p, score_all_.p, odom_partials_.p,
                         nconv_.p, s);
  // ---- while the device searches: the problems of Estimator.cc:1660-1921, packed for the device loop.  Their uploads overwrite
  // what the previous solve's marginalization (on its own stream) still reads: everything enqueued from here on waits for it —
  // it has had this solve's filter, grids, features and first rounds to finish.
  const double t3a = now_ms();
  ev_wait_valid_ = false;
  if (marg_in_flight_) {
    LIO_HIP(hipEventRecord(ev_wait_[0], s));
    LIO_HIP(hipStreamWaitEvent(s, ev_marg_, 0));
    LIO_HIP(hipEventRecord(ev_wait_[1], s));   // (reached when the first three rounds are done AND the marginalization is: the difference is rounds + wait;
    ev_wait_valid_ = true;                     //  the rounds in front of it end at ev_wait_[0], so [0] -> [1] is the wait alone)
    marg_in_flight_ = false;
  }
  int max_bpf = 1, max_wo = 1, max_npad = DS_NB;
  size_t part_total = 0;
  for (int w = 0; w < B; ++w) {
    Win &Wn = win_[w];
    if (!Wn.device) continue;
    Estimator *e = Wn.e;
    Wn.bpf = batch_blocks_per_frame(Wn.max_slots);
    if (h_win_.p[w].n_slots == 0 || !e->BatchPackProblem(Wn.bpf, h_pb_.p[w], h_st_.p[w], &Wn.prior_used)) { Wn.device = false; continue; }
    Wn.part_off = part_total;
    part_total += size_t(e->Wo_) * Wn.bpf * LIO_MOMENT_OUT;
    max_bpf = std::max(max_bpf, Wn.bpf); max_wo = std::max(max_wo, e->Wo_); max_npad = std::max(max_npad, h_pb_.p[w].n_pad);
    // the prior's matrices on the device: already there (the previous solve's marginalization left them, or an earlier upload), or sent now
    if (Wn.prior_used) {
      int k = -1;
      for (int q = 0; q < 2; ++q) if (Wn.dev_prior[q] == Wn.prior_used) k = q;
      if (k < 0) {
        k = 0;
        Materialize(w, k);
        MargPrior &pr = *Wn.prior_used;
        pr.materialize();
        const size_t n = size_t(pr.n);
        double *h = h_prior_.p + size_t(w) * ds_prior_mats_size(MARG_MAX_N);
        std::memcpy(h, pr.JtJ.a.data(), sizeof(double) * n * n);
        std::memcpy(h + n * n, pr.lin_jac.a.data(), sizeof(double) * n * n);
        std::memcpy(h + 2 * n * n, pr.lin_res.data(), sizeof(double) * n);
        std::memcpy(h + 2 * n * n + n, pr.Jtr0.data(), sizeof(double) * n);
        LIO_HIP(hipMemcpyAsync(slab_.p + size_t(w) * lay_.total + lay_.prior[k], h, sizeof(double) * ds_prior_mats_size(pr.n), hipMemcpyHostToDevice, s));
        Wn.dev_prior[k] = Wn.prior_used;
      }
      Wn.cur = k;
    } else {
      Wn.cur = 0;
    }
  }
  LIO_HIP(hipMemcpyAsync(d_pb_.p, h_pb_.p, sizeof(DevProblem) * B, hipMemcpyHostToDevice, s));
  LIO_HIP(hipMemcpyAsync(d_st_.p, h_st_.p, sizeof(DevState) * B, hipMemcpyHostToDevice, s));
  clk_.pack = now_ms() - t3a;
  // ---- the remaining rounds, with a look at the number of converged windows every second round
  for (; round < 10; ++round) {
    if (round >= 3 && round % 2 == 1) {
      LIO_HIP(hipMemcpyAsync(h_nconv_.p, nconv_.p, sizeof(int), hipMemcpyDeviceToHost, s));
      LIO_HIP(hipStreamSynchronize(s));
      if (*h_nconv_.p >= B) break;
    }
    launch_bw_odom_round(d_win_.p, d_grid_.p, B, max_nb, q_newest, knobs_, round, d_odom_.p, sorted_all_.p, cells_all_.p, valid_all_.p, coef_all_.p, score_all_.p, odom_partials_.p,
                         nconv_.p, s);
  }
  clk_.rounds = round;
  LIO_HIP(hipEventRecord(ev_[4], s));
  LIO_HIP(hipMemcpyAsync(h_odom_.p, d_odom_.p, sizeof(OdomState) * B, hipMemcpyDeviceToHost, s));
  LIO_HIP(hipStreamSynchronize(s));
  const double t3 = now_ms();
  clk_.grid_features = t3 - t2;
  // ------------------------------------------------------------------------------------------------ the trust-region loop
  partials_.reserve(std::max<size_t>(part_total, 1), s);
  int max_it = 0, n_dev = 0;
  for (int w = 0; w < B; ++w) {
    Win &Wn = win_[w];
    BatchSolve &S = h_bs_.p[w];
    std::memset(static_cast<void *>(&S), 0, sizeof(S));
    S.marg = d_mg_.p + w;
    if (!Wn.device) continue;
    Estimator *e = Wn.e;
    e->ApplyOdomState(h_odom_.p[w]);
    double *slab = slab_.p + size_t(w) * lay_.total;
    S.active = 1; S.nframes = e->Wo_; S.bpf = Wn.bpf;
    e->FillMomentFrames(S.fr, h_win_.p[w].slot_base);   // (BatchEligible: not sharded)
    S.pb = d_pb_.p + w; S.st = d_st_.p + w;
    S.prior_mats = slab + lay_.prior[Wn.cur]; S.next_prior_mats = slab + lay_.prior[1 - Wn.cur];
    S.partials = partials_.p + Wn.part_off;
    S.imu_out = slab + lay_.imu; S.lmap = slab + lay_.lmap; S.prior_out = slab + lay_.prior_out; S.exprior_out = slab + lay_.exprior;
    static const bool dbg_prof = std::getenv("LIO_DEBUG_TIMING") != nullptr;
    S.Hcur = slab + lay_.Hcur; S.S_buf = slab + lay_.Sbuf; S.prof = (dbg_prof && w == 0) ? reinterpret_cast<long long *>(slab + lay_.prof) : nullptr;
    S.marg_imu = slab + lay_.marg_imu; S.marg_lmap = slab + lay_.marg_lmap; S.marg_prior_out = slab + lay_.marg_prior_out;
    S.marg_A = slab + lay_.marg_A; S.marg_info = slab + lay_.marg_info;
    max_it = std::max(max_it, e->cfg_.max_num_iterations);
    ++n_dev;
  }
  LIO_HIP(hipMemcpyAsync(d_bs_.p, h_bs_.p, sizeof(BatchSolve) * B, hipMemcpyHostToDevice, s));
  if (n_dev > 0) {
    // iteration k evaluates candidate k (k = 0: the initial point); a window that is done costs its blocks one load each.
    // Groups of windows run their chains side by side (see est_batch.h); one group below 32 windows.
    // Groups by size, measured with the interleaved enqueue below (profiles/r6_m_loop_groups.txt; loop ms at 1 / 2 / 4 / 8 groups): 32 windows
    // 1.86 / 1.84 / 1.78 / 1.79, 64: 2.51 / 2.10 / 2.08 / 2.15, 128: 3.46 / 3.23 / 2.77 / 3.21 (four chains = four hardware queues), 256: 5.60 /
    // 5.05 / 5.28 / 5.04, 512: 10.3 / 9.6 / 9.6 / 9.6.
    const int G = knobs_.loop_groups ? std::min(knobs_.loop_groups, B) : (B >= 32 ? (B < 256 ? 4 : 2) : 1);
    const BatchBases bases{slab_.p, partials_.p, d_st_.p, d_pb_.p, d_mg_.p};
    static const int prof_it = [] { const char *e = std::getenv("LIO_DEBUG_TIMING_IT"); return e ? std::atoi(e) : 3; }();
    if (G > 1) LIO_HIP(hipEventRecord(ev_fork_, s));
    // The groups' chains are enqueued INTERLEAVED, iteration by iteration: a group's chain is 3 x (max_iterations + 1) launches, ~130 us of
    // host enqueue time — enqueued one whole chain after the other, group g started that much behind group g - 1 and the loop ended that
    // much later (at 64 windows the loop is one chain's latency, not throughput).
    struct Grp { int w0, w1, bpf, wo, npad, it, n; hipStream_t sg; };
    Grp grp[kGroups];
    int it_max = 0;
    for (int g = 0; g < G; ++g) {
      Grp &q = grp[g];
      q.w0 = int((long long)B * g / G); q.w1 = int((long long)B * (g + 1) / G);
      q.sg = G > 1 ? stream_grp_[g] : s;
      if (G > 1) LIO_HIP(hipStreamWaitEvent(q.sg, ev_fork_, 0));
      q.bpf = 1; q.wo = 1; q.npad = DS_NB; q.it = 0; q.n = 0;
      for (int w = q.w0; w < q.w1; ++w) {
        if (!win_[w].device) continue;
        const Estimator *e = win_[w].e;
        q.bpf = std::max(q.bpf, win_[w].bpf); q.wo = std::max(q.wo, e->Wo_); q.npad = std::max(q.npad, h_pb_.p[w].n_pad);
        q.it = std::max(q.it, e->cfg_.max_num_iterations); ++q.n;
      }
      if (q.n > 0) it_max = std::max(it_max, q.it);
    }
    for (int k = 0; k <= it_max; ++k)
      for (int g = 0; g < G; ++g) {
        const Grp &q = grp[g];
        if (q.n == 0 || k > q.it) continue;
        const int w0 = q.w0, w1 = q.w1, g_bpf = q.bpf, g_wo = q.wo, g_npad = q.npad;
        hipStream_t sg = q.sg;
        const BatchSolve *gb = d_bs_.p + w0;
        if (knobs_.time_kernels) {   // measurement run: the three launches bracketed by events on their stream
          while (ev_k_.size() < size_t(ev_k_used_ + 4)) { hipEvent_t e = nullptr; LIO_HIP(hipEventCreate(&e)); ev_k_.push_back(e); }
          hipEvent_t *ek = ev_k_.data() + ev_k_used_;
          ev_k_used_ += 4;
          LIO_HIP(hipEventRecord(ek[0], sg));
          launch_bw_aux(gb, bases, w1 - w0, g_wo, knobs_.aux_threads, sg);
          LIO_HIP(hipEventRecord(ek[1], sg));
          launch_bw_moments(gb, bases, w1 - w0, g_bpf, g_wo, valid_all_.p, coef_all_.p, sg);
          LIO_HIP(hipEventRecord(ek[2], sg));
          launch_bw_step(gb, bases, w1 - w0, g_wo, g_npad, sg);
          LIO_HIP(hipEventRecord(ek[3], sg));
        } else {
          launch_bw_solve_iteration(gb, bases, w1 - w0, g_bpf, g_wo, g_npad, knobs_.aux_threads, valid_all_.p, coef_all_.p, sg);
        }
        if (h_bs_.p[0].prof && w0 == 0 && k == prof_it)   // LIO_DEBUG_TIMING: keep the stamps of this iteration's launch B beside the last one's
          LIO_HIP(hipMemcpyAsync(h_bs_.p[0].prof + 32, h_bs_.p[0].prof, 32 * sizeof(long long), hipMemcpyDeviceToDevice, sg));
      }
    if (G > 1)
      for (int g = 0; g < G; ++g) { LIO_HIP(hipEventRecord(ev_grp_[g], grp[g].sg)); LIO_HIP(hipStreamWaitEvent(s, ev_grp_[g], 0)); }
    LIO_HIP(hipEventRecord(ev_[5], s));
    LIO_HIP(hipMemcpyAsync(h_st_.p, d_st_.p, sizeof(DevState) * B, hipMemcpyDeviceToHost, s));
    LIO_HIP(hipStreamSynchronize(s));
  } else {
    LIO_HIP(hipEventRecord(ev_[5], s));
  }
  if (h_bs_.p[0].prof) {   // LIO_DEBUG_TIMING: the phase stamps of window 0's last launch B (shader clock, 100 MHz wall clock is not used here)
    long long pr[96];
    LIO_HIP(hipMemcpy(pr, h_bs_.p[0].prof, sizeof(pr), hipMemcpyDeviceToHost));
    for (int half = 1; half >= 0; --half) {
      std::fprintf(stderr, "[lio_hip timing] launch B of window 0, %s, clock64 ticks from its start:", half ? "iteration LIO_DEBUG_TIMING_IT (default 3)" : "last launch");
      for (int k = 0; k < 32; ++k) std::fprintf(stderr, " P%d %lld", k, pr[32 * half + k] ? pr[32 * half + k] - pr[32 * half] : -1);
      std::fprintf(stderr, "\n");
    }
    std::fprintf(stderr, "[lio_hip timing] aux row of window 0, block 0 (ImuFactor 0 + lidar map 1), last launch, clock64 ticks: raw Jacobians + residual %lld, whitening %lld, J^T J %lld, lidar map %lld\n",
                 pr[65] - pr[64], pr[66] - pr[65], pr[67] - pr[66], pr[68] - pr[67]);
  }
  clk_.iterations = max_it + 1;
  const double t4 = now_ms();
  clk_.solve = t4 - t3;
  // ------------------------------------------------------------------------------------------------ write-back, marginalization
  int max_n = 1, n_marg = 0;
  std::vector<int> host_path;
  // per window: the state back into the estimator (DoubleToVector), the report, the marginalization's layout.  Window-local host
  // work with the device idle behind it (1.3 ms at 512 windows on one thread): from 128 windows on, four threads share it.
  std::vector<std::shared_ptr<MargPrior>> shells(B);
  std::vector<char> margs(B, 0);
  auto finish_range = [&](int w0, int w1) {
    for (int w = w0; w < w1; ++w) {
      Win &Wn = win_[w];
      DevMarg &mg = h_mg_.p[w];
      std::memset(&mg, 0, sizeof(mg));
      if (!Wn.device) continue;
      const DevState &st = h_st_.p[w];
      if (st.need_host || !st.started) continue;
      margs[w] = Wn.e->BatchFinish(st, Wn.prior_used, reps[w], mg, &shells[w]) ? 1 : 0;
    }
  };
  {
    const int T = knobs_.finish_threads ? std::min(knobs_.finish_threads, B) : (B >= 256 ? 8 : (B >= 128 ? 4 : 1));   // (512 windows: 1.31 -> 1.03 ms with eight, profiles/r6_h_*)
    if (T == 1) {
      finish_range(0, B);
    } else {
      std::vector<std::thread> pool;
      std::vector<std::exception_ptr> errs(T);
      for (int t = 0; t < T; ++t)
        pool.emplace_back([&, t] {
          try { finish_range(int((long long)B * t / T), int((long long)B * (t + 1) / T)); } catch (...) { errs[t] = std::current_exception(); }
        });
      for (std::thread &th : pool) th.join();
      for (const std::exception_ptr &e : errs) if (e) std::rethrow_exception(e);
    }
  }
  for (int w = 0; w < B; ++w) {
    Win &Wn = win_[w];
    if (!Wn.device) { host_path.push_back(w); continue; }
    const DevState &st = h_st_.p[w];
    if (st.need_host || !st.started) { Wn.device = false; host_path.push_back(w); continue; }
    if (margs[w]) {
      const int nb = 1 - Wn.cur;
      Materialize(w, nb);
      std::shared_ptr<MargPrior> &shell = shells[w];
      shell->on_device = true;
      shell->fetch = [this, w, nb](MargPrior &pr) { FetchPrior(w, nb, pr); };
      Wn.dev_prior[nb] = shell;
      Wn.e->last_marg_ = shell;
      max_n = std::max(max_n, h_mg_.p[w].n);
      ++n_marg;
    }
    Wn.prior_used.reset();
  }
  clk_.n_device = B - int(host_path.size()); clk_.n_host = int(host_path.size());
  if (n_marg > 0) {
    // (the host has waited for the loop; the marginalization's inputs — final moments, states, problems — are complete)
    LIO_HIP(hipMemcpyAsync(d_mg_.p, h_mg_.p, sizeof(DevMarg) * B, hipMemcpyHostToDevice, stream_marg_));
    launch_bw_marginalize(d_bs_.p, BatchBases{slab_.p, partials_.p, d_st_.p, d_pb_.p, d_mg_.p}, B, max_wo, max_n, stream_marg_);
    LIO_HIP(hipEventRecord(ev_marg_, stream_marg_));
    marg_in_flight_ = true;
  }
  LIO_HIP(hipEventRecord(ev_[6], stream_marg_));
  ev_valid_ = true;
  const double t5 = now_ms();
  clk_.finish = t5 - t4;
  // ------------------------------------------------------------------------------------------------ windows the device loop did not take
  for (int w = 0; w < B; ++w) ok_[size_t(w)] = 1;
  for (int w : host_path) ok_[size_t(w)] = win_[w].e->SolveOptimizationHost(&reps[w]) ? 1 : 0;
  for (int w = 0; w < B; ++w)   // the end of SolveOptimization for a window the device loop solved (the host path does it itself)
    if (win_[w].device && win_[w].e->full_cloud()) win_[w].e->CorrectNewestFull();
  const double t6 = now_ms();
  clk_.fallback = t6 - t5;
  clk_.total = t6 - t0;
  for (int w = 0; w < B; ++w) {
    if (!win_[w].device) continue;
    win_[w].e->feat_batch_ = this; win_[w].e->feat_batch_w_ = w;   // its feature slots are in valid_all_ / coef_all_ / score_all_
    lio_solve_report &R = reps[w];
    R.ms_build_map = clk_.map; R.ms_features = clk_.grid_features; R.ms_prepare = clk_.describe + clk_.pack; R.ms_opt = clk_.solve; R.ms_marg = clk_.finish;
    R.ms_total = t5 - t0;
  }
  return B;
}

// ---------------------------------------------------------------- the members' per-sweep work (include/lio_est_push_batch.h)
// Estimator::PushFrame of every member with the device work of all of them in one chain (est_push.h): PushFrameBegin per window, the clouds
// that are filtered through the chain (one wait), a flagged cloud through its handle's own filter, PushFrameEnd per window.
void EstimatorBatch::PushFrames(const lio_est_frame *fr) {
  std::vector<PushInput> in(static_cast<size_t>(size()));
  for (int w = 0; w < size(); ++w) {
    const lio_est_frame &f = fr[w];
    in[size_t(w)] = PushInput{Rigidf(Quat<float>(f.transform_in.q[3], f.transform_in.q[0], f.transform_in.q[1], f.transform_in.q[2]),
                                     Vec3<float>(f.transform_in.p[0], f.transform_in.p[1], f.transform_in.p[2])),
                              CloudSrc::host(f.surf_xyzi, f.n_surf), CloudSrc::host(f.corner_xyzi, f.n_corner), f.stamp, MapFullSource{}};
  }
  PushAll(in.data());
}

// The device-fed pushes (include/lio_est_from_odom.h).  composite: the message's third block of ProcessCompactData — a window with its full cloud
// on takes the given one or, given none, has it cleared; in the push form such a window keeps what it has.
void EstimatorBatch::PushFrom(const OdomSweep *src, const Rigidf *T_in, const double *stamps, bool composite) {
  const int B = size();
  std::vector<PushInput> in(static_cast<size_t>(B));
  for (int w = 0; w < B; ++w) {
    const OdomSweep &S = src[w];
    PushInput &f = in[size_t(w)] = PushInput{T_in[w], S.surf, S.corner, stamps[w], MapFullSource{}};
    if (m_[size_t(w)]->full_cloud()) {
      if (S.full.set) f.full = S.full;
      else if (composite) f.full.set = true;   // an empty third block: n = 0 clears it
    }
  }
  PushAll(in.data());
}
void EstimatorBatch::PushFramesFrom(const OdomSweep *src, const lio_transform_f *T_in, const double *stamps) {
  std::vector<Rigidf> T(static_cast<size_t>(size()));
  for (int w = 0; w < size(); ++w)
    T[size_t(w)] = Rigidf(Quat<float>(T_in[w].q[3], T_in[w].q[0], T_in[w].q[1], T_in[w].q[2]), Vec3<float>(T_in[w].p[0], T_in[w].p[1], T_in[w].p[2]));
  PushFrom(src, T.data(), stamps, false);
}

// Estimator::PushFrame of every member, the sweeps where `in` says (the device's: no cloud goes up, and the launch that takes the sweeps writes
// the maps' full clouds too, in front of PushFrameEnd's PushFull)
void EstimatorBatch::PushAll(const PushInput *in) {
  const int B = size();
  const bool on_device = clouds_on_device(size_t(2) * size_t(B), [&](size_t i) { return i & 1 ? in[i / 2].corner : in[i / 2].surf; });
  hipStream_t s = stream_;
  for (int &v : push_stats_) v = 0;
  if (on_device) for (int &v : from_stats_) v = 0;
  plans_.clear();
  plans_.resize(size_t(B));
  push_.begin(2 * B, on_device ? B : 0, on_device);
  std::vector<int> cloud(size_t(2 * B), -1);   // the chain's cloud of window w's surf [2 w] and corner [2 w + 1] sweep
  // by what every window's clouds took in its previous push (seg_vox.h: the pass rule, as for Solve's local maps)
  int passes = 3;
  for (int w = 0; w < B; ++w) {
    Estimator *e = m_[size_t(w)];
    PushPlan &pl = plans_[size_t(w)];
    const PushInput &f = in[w];
    if (on_device && f.full.set) {   // lio_map_set_full_cloud, the points written by the chain's launch (Estimator::ProcessCompact: SetFullCloud first)
      const MapFullSource &F = f.full;
      if (float4 *dst = e->map_->FullTake(F.n, s)) push_.add_full(FullTake{F.pts, dst, int(F.n), F.to_end});
      ++from_stats_[2];
    }
    e->PushFrameBegin(f.transform_in, f.surf.n, f.corner.n, f.stamp, pl);
    if (pl.filter) {
      if (pl.corner_cloud)
        cloud[size_t(2 * w + 1)] = push_.add(f.corner, e->cfg_.corner_filter_size, pl.deskew, pl.q, pl.p, 10.f, pl.corner_cloud->buf.p);
      cloud[size_t(2 * w)] = push_.add(f.surf, e->cfg_.surf_filter_size, pl.deskew, pl.q, pl.p, 10.f, pl.fresh.buf.p);
      passes = std::max(passes, SegVoxFilter::passes_for(win_[size_t(w)].push_bits));
    } else {   // both de-skew switches off (Estimator.cc:474-480): the clouds go into the handle's buffers as they are
      if (pl.corner_cloud) {
        if (f.corner.n) LIO_HIP(hipMemcpyAsync(pl.corner_cloud->buf.p, f.corner.p, f.corner.n * sizeof(float4), f.corner.to_device(), s));
        pl.corner_cloud->n = f.corner.n;
        ++push_stats_[2];
      }
      if (f.surf.n) LIO_HIP(hipMemcpyAsync(pl.fresh.buf.p, f.surf.p, f.surf.n * sizeof(float4), f.surf.to_device(), s));
      pl.fresh.n = f.surf.n;
      ++push_stats_[2];
    }
  }
  bool waited = push_.run(vox_, passes, s);
  if (!waited && push_stats_[2]) { LIO_HIP(hipStreamSynchronize(s)); waited = true; }   // the caller may reuse its buffers on return
  push_stats_[3] = waited ? 1 : 0;
  push_stats_[4] = push_.clouds() ? passes : 0;
  if (on_device) { from_stats_[0] = push_.clouds(); from_stats_[1] = push_stats_[2]; from_stats_[3] = push_.uploads(); }
  for (int w = 0; w < B; ++w) {
    Estimator *e = m_[size_t(w)];
    PushPlan &pl = plans_[size_t(w)];
    int bits = 0;
    for (int k = 1; k >= 0; --k) {   // (corner, then surf: PushFrame's order)
      const int i = cloud[size_t(2 * w + k)];
      if (i < 0) continue;
      const VoxSegOut &o = vox_.out(i);
      const size_t n = k ? pl.n_corner : pl.n_surf;
      size_t count = size_t(o.count);
      if (o.flagged || o.params.overflow) {
        // keys beyond the absolute range or the passes, or PCL's "leaf size too small": the handle's own filter has the exact and the
        // output-equals-input forms; it reads the cloud as the chain staged it (de-skewed already)
        count = k ? e->vox_corner_.run(push_.input(i), n, e->cfg_.corner_filter_size, pl.corner_cloud->buf, s)
                  : e->vox_.run(push_.input(i), n, e->cfg_.surf_filter_size, pl.fresh.buf, s);
        ++push_stats_[1];
      } else {
        ++push_stats_[0];
      }
      bits = std::max(bits, SegVoxFilter::bits_taken(o.params));
      if (k) pl.corner_cloud->n = count;
      else pl.fresh.n = count;
    }
    if (bits) win_[size_t(w)].push_bits = bits;
    e->PushFrameEnd(pl);
  }
  plans_.clear();
}

// Estimator::SlideWindow of every member: SlideBegin per window, the concats of all of them in one launch, SlideEnd per window
void EstimatorBatch::SlideWindows() {
  const int B = size();
  hipStream_t s = stream_;
  if (!ev_slide_) LIO_HIP(hipEventCreateWithFlags(&ev_slide_, hipEventDisableTiming));
  else LIO_HIP(hipEventSynchronize(ev_slide_));   // the previous call's table has left the pinned staging (long done: no stream is waited for)
  if (h_slide_.n < size_t(B)) h_slide_.alloc(size_t(B), hipHostMallocDefault, true);
  d_slide_.reserve(size_t(B), s);
  std::vector<ConcatArgs> ca(static_cast<size_t>(B));
  std::vector<char> concat(size_t(B), 0);
  int max_total = 0;
  for (int w = 0; w < B; ++w) {
    Estimator *e = m_[size_t(w)];
    concat[size_t(w)] = e->SlideBegin(ca[size_t(w)]) ? 1 : 0;
    BpSlide &S = h_slide_.p[w];
    std::memset(static_cast<void *>(&S), 0, sizeof(S));
    if (!concat[size_t(w)]) continue;
    S.seg[0] = ca[size_t(w)].seg[0]; S.seg[1] = ca[size_t(w)].seg[1];
    S.total = ca[size_t(w)].total;
    S.dst = e->slide_dst();
    max_total = std::max(max_total, S.total);
  }
  if (max_total > 0) {
    LIO_HIP(hipMemcpyAsync(d_slide_.p, h_slide_.p, sizeof(BpSlide) * size_t(B), hipMemcpyHostToDevice, s));
    LIO_HIP(hipEventRecord(ev_slide_, s));
    launch_bp_slide(d_slide_.p, B, max_total, s);
  }
  for (int w = 0; w < B; ++w) m_[size_t(w)]->SlideEnd(concat[size_t(w)] != 0, ca[size_t(w)]);
}

// Estimator::ProcessLaserOdom (Estimator.cc:430-774) of initialised members: push, solve, the map refresh (:703-708), slide
bool EstimatorBatch::ProcessLaserOdom(const lio_est_frame *fr, lio_solve_report *reps) {
  for (Estimator *e : m_) ++e->laser_odom_recv_count_;
  PushFrames(fr);
  return SolveRefreshSlide(reps);
}
// Estimator::ProcessCompact (Estimator.cc:776-856) of initialised members, the message never built: the prediction and transform_sum_
// (CompactPredict), then ProcessLaserOdom with the sweeps and the third block taken on the device
bool EstimatorBatch::ProcessCompactFrom(const OdomSweep *src, const double *stamps, lio_transform_f *T_out, lio_solve_report *reps) {
  const int B = size();
  std::vector<Rigidf> T(static_cast<size_t>(B));
  for (int w = 0; w < B; ++w) {
    T[size_t(w)] = m_[size_t(w)]->CompactPredict(src[w].transform_sum);
    if (T_out) {
      const Rigidf &t = T[size_t(w)];
      T_out[w] = lio_transform_f{{t.rot.x, t.rot.y, t.rot.z, t.rot.w}, {t.pos.x, t.pos.y, t.pos.z}};
    }
  }
  for (Estimator *e : m_) ++e->laser_odom_recv_count_;
  PushFrom(src, T.data(), stamps, true);
  return SolveRefreshSlide(reps);
}
bool EstimatorBatch::SolveRefreshSlide(lio_solve_report *reps) {
  const int B = size();
  Solve(reps);
  bool ok = true;
  for (int w = 0; w < B; ++w) {
    if (m_[size_t(w)]->map_refresh()) m_[size_t(w)]->RefreshMap();
    ok = ok && window_ok(w);
  }
  SlideWindows();
  for (Estimator *e : m_) e->last_event_ = Estimator::EV_SOLVED;
  return ok;
}

// ---------------------------------------------------------------- the partition
void BatchParts::Build() {
  b_[0].reset(); b_[1].reset();   // (a part's destructor brings its device-resident priors back to the host objects)
  const int n = size();
  const int want = parts_opt_ ? parts_opt_ : (n >= kBatchSplitFrom ? 2 : 1);
  n1_ = (want == 2 && n >= 2) ? (n + 1) / 2 : n;
  std::unique_ptr<EstimatorBatch> first(new EstimatorBatch(std::vector<Estimator *>(e_.begin(), e_.begin() + n1_)));
  if (n1_ < n) b_[1].reset(new EstimatorBatch(std::vector<Estimator *>(e_.begin() + n1_, e_.end())));
  b_[0] = std::move(first);   // (built() only once every part stands)
  ApplyOptions();
}
void BatchParts::ApplyOptions() {
  bool groups_set = false;
  for (const auto &o : options_) {
    if (o.first == "loop_groups" && o.second != 0) groups_set = true;
    for (auto &b : b_) if (b) b->SetOption(o.first.c_str(), o.second);
  }
  // two parts side by side are two launch chains already: one loop group each unless the caller asked for a number
  if (b_[1] && !groups_set) for (auto &b : b_) b->SetOption("loop_groups", 1);
}
bool BatchParts::SetOption(const char *name, int value) {
  if (!name) return false;
  if (std::string(name) == "parts") {
    if (value < 0 || value > 2) return false;
    if (value != parts_opt_) { parts_opt_ = value; Build(); }
    return true;
  }
  if (!b_[0]->SetOption(name, value)) return false;
  bool found = false;
  for (auto &o : options_) if (o.first == name) { o.second = value; found = true; }
  if (!found) options_.emplace_back(name, value);
  ApplyOptions();
  return true;
}
template <typename F> void BatchParts::ForParts(F &&f) {
  if (!b_[1]) { f(*b_[0], 0); return; }
  std::exception_ptr err1, err2;   // the first part's is rethrown in preference to the second's
  std::thread t2([&] {   // (the current device is per thread)
    try { LIO_HIP(hipSetDevice(b_[1]->device())); f(*b_[1], n1_); } catch (...) { err2 = std::current_exception(); }
  });
  try { f(*b_[0], 0); } catch (...) { err1 = std::current_exception(); }
  t2.join();
  if (err1 || err2) std::rethrow_exception(err1 ? err1 : err2);
}
void BatchParts::Solve(lio_solve_report *reps) { ForParts([&](EstimatorBatch &b, int w0) { b.Solve(reps ? reps + w0 : nullptr); }); }
bool BatchParts::SolveRestored(int steps, lio_solve_report *reps) {
  std::atomic<int> bad{0};
  ForParts([&](EstimatorBatch &b, int w0) {
    const int w1 = w0 + b.size();
    for (int k = 0; k < steps && !bad.load(); ++k) {
      for (int w = w0; w < w1; ++w) if (!e_[size_t(w)]->Restore()) { bad.store(1); return; }
      for (int w = w0; w < w1; ++w) if (!e_[size_t(w)]->inited_) { bad.store(1); return; }
      b.Solve(reps ? reps + w0 : nullptr);
    }
    b.Sync();
  });
  return !bad.load();
}
bool BatchParts::PushReady() const {
  for (const Estimator *e : e_) if (!e->inited_ || e->PushRefused()) return false;
  return true;
}
void BatchParts::PushFrames(const lio_est_frame *frames) { ForParts([&](EstimatorBatch &b, int w0) { b.PushFrames(frames + w0); }); }
void BatchParts::SlideWindows() { ForParts([&](EstimatorBatch &b, int) { b.SlideWindows(); }); }
bool BatchParts::ProcessLaserOdom(const lio_est_frame *frames, lio_solve_report *reps) {
  std::atomic<int> bad{0};
  ForParts([&](EstimatorBatch &b, int w0) { if (!b.ProcessLaserOdom(frames + w0, reps ? reps + w0 : nullptr)) bad.store(1); });
  return !bad.load();
}
void BatchParts::PushFramesFrom(const OdomSweep *src, const lio_transform_f *T_in, const double *stamps) {
  ForParts([&](EstimatorBatch &b, int w0) { b.PushFramesFrom(src + w0, T_in + w0, stamps + w0); });
}
bool BatchParts::ProcessCompactFrom(const OdomSweep *src, const double *stamps, lio_transform_f *T_out, lio_solve_report *reps) {
  std::atomic<int> bad{0};
  ForParts([&](EstimatorBatch &b, int w0) {
    if (!b.ProcessCompactFrom(src + w0, stamps + w0, T_out ? T_out + w0 : nullptr, reps ? reps + w0 : nullptr)) bad.store(1);
  });
  return !bad.load();
}
void BatchParts::FromOdomStats(int out[8]) const {
  for (int k = 0; k < 8; ++k) out[k] = 0;
  for (const auto &b : b_) if (b) for (int k = 0; k < 8; ++k) out[k] += b->from_odom_stats()[k];
}
void BatchParts::PushStats(int out[8]) const {
  for (int k = 0; k < 8; ++k) out[k] = 0;
  for (const auto &b : b_) if (b) for (int k = 0; k < 8; ++k) out[k] += b->push_stats()[k];
}
void BatchParts::Sync() { for (auto &b : b_) if (b) b->Sync(); }
void BatchParts::StageDigest(int stage, unsigned long long *out) {
  b_[0]->StageDigest(stage, out);
  if (b_[1]) b_[1]->StageDigest(stage, out + n1_);
}
BatchClock BatchParts::clock() {
  BatchClock c = b_[0]->clock();
  if (!b_[1]) return c;
  const BatchClock d = b_[1]->clock();
  c.describe = std::max(c.describe, d.describe); c.map = std::max(c.map, d.map); c.grid_features = std::max(c.grid_features, d.grid_features);
  c.pack = std::max(c.pack, d.pack); c.solve = std::max(c.solve, d.solve); c.finish = std::max(c.finish, d.finish);
  c.fallback = std::max(c.fallback, d.fallback); c.total = std::max(c.total, d.total);
  c.n_device += d.n_device; c.n_host += d.n_host; c.rounds = std::max(c.rounds, d.rounds);
  for (int k = 0; k < 6; ++k) c.dev[k] += d.dev[k];
  c.dev_marg_wait += d.dev_marg_wait;
  for (int k = 0; k < 3; ++k) { c.kernel_ms[k] += d.kernel_ms[k]; c.kernel_launches[k] += d.kernel_launches[k]; }
  return c;
}

}  // namespace lio
