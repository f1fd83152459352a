// capi.hip — include/lio_c.h implemented by the product (liblio_hip.so).  Every entry point that touches
// point data runs on the GPU; a missing device or a HIP failure is reported as LIO_ERR_DEVICE — there is
// no CPU fallback.  Pure-host entry points (pre-integration, single-factor evaluation) are the host
// half of the estimator and also back the `-m "not gpu"` ABI tests.
#include <cstring>
#include <new>

#include "../../include/lio_c.h"
#include "../../include/lio_test_hooks.h"
#include "../../include/lio_ext.h"
#include "../../include/lio_est_wide.h"
#include "../../include/lio_full_cloud.h"
#include "../../include/lio_est_from_odom.h"
#include "../../include/lio_odom_batch.h"
#include "../../include/lio_frontend_batch.h"
#include "../../include/lio_map_batch.h"
#include "../../include/lio_map_from_odom.h"
#include "../../include/lio_vox_sort.h"
#include "../../include/lio_seg_bounds.h"
#include "est_batch.h"
#include "seg_sort.h"
#include "estimator.h"
#include "rccl_comm.h"
#include "host_init.h"
#include "kf_batch.h"
#include <mutex>
#include <algorithm>

#include "mapping.h"
#include "odometry.h"
#include "pointproc.h"

using namespace lio;

struct lio_pim { std::shared_ptr<Preintegration> p; };
// (members are destroyed in reverse order: the batch of one that serves lio_est_config.device_solve goes before the estimator it adopted)
struct lio_map { std::unique_ptr<MappingDev> m; bool borrowed = false; };   // borrowed: the member of a lio_est (lio_est_map), not for lio_map_destroy
struct lio_est { std::unique_ptr<Estimator> e; EstConfig cfg; lio_map map; lio_map_config map_cfg; std::unique_ptr<EstimatorBatch> solo; bool adopted = false; struct lio_est_batch *owner = nullptr; };
// `parts`: the batch's one or two EstimatorBatch objects (est_batch.h); null once the batch is dissolved.  `members`: adoption and ownership.
struct lio_est_batch { std::unique_ptr<BatchParts> parts; std::vector<lio_est *> members; };
// lio_pp_process_batch runs its sweeps through ONE multi-sweep processor shared by the handles of the call (`pool`); a handle whose last
// sweep went that way reads its results from sweep `pool_sweep` of it.  The pool is shared state: its users take `mu`.
// `gen` counts the pool's batches, from 1.  A handle reads the pool only while its `pool_gen` is the pool's: a handle whose results a LATER
// batch of other handles overwrote (same pool, its own sweep not among them) is told so instead of being handed somebody else's sweep, and
// pool_gen = 0 is a lease on nothing (the handle of a batch that failed).
struct lio_pp_pool { PointProcessorDev pp; std::mutex mu; unsigned long gen = 0; lio_pp_pool(float lo, float up, int r, const lio_pp_config &c) : pp(lo, up, r, c) {} };
struct lio_pp { std::unique_ptr<PointProcessorDev> pp; std::shared_ptr<lio_pp_pool> pool; int pool_sweep = -1; unsigned long pool_gen = 0; };
struct lio_odom { std::unique_ptr<OdometryDev> o; };

static V3d v3(const double *p) { return V3d(p[0], p[1], p[2]); }
static Rigidf toT(const lio_transform_f &t) { return Rigidf(Quat<float>(t.q[3], t.q[0], t.q[1], t.q[2]), Vec3<float>(t.p[0], t.p[1], t.p[2])); }
static void fromT(const Rigidf &T, lio_transform_f *o) {
  o->q[0] = T.rot.x; o->q[1] = T.rot.y; o->q[2] = T.rot.z; o->q[3] = T.rot.w; o->p[0] = T.pos.x; o->p[1] = T.pos.y; o->p[2] = T.pos.z;
}

static thread_local char g_last_error[512];
template <typename F> static int guarded(F &&f) {
  try {
    return f();
  } catch (const DeviceError &e) {
    std::snprintf(g_last_error, sizeof(g_last_error), "%s", e.what());
    std::fprintf(stderr, "[lio_hip] %s\n", e.what());
    return LIO_ERR_DEVICE;
  } catch (const CapacityError &e) {
    std::snprintf(g_last_error, sizeof(g_last_error), "%s", e.what());
    std::fprintf(stderr, "[lio_hip] %s\n", e.what());
    return LIO_ERR_CAPACITY;
  } catch (const std::exception &e) {
    std::snprintf(g_last_error, sizeof(g_last_error), "%s", e.what());
    std::fprintf(stderr, "[lio_hip] %s\n", e.what());
    return LIO_ERR_STATE;
  }
}

// what a size_t accessor answers: f(), or 0 when it throws
template <typename F> static size_t guarded_count(F &&f) {
  size_t n = 0;
  guarded([&] { n = f(); return LIO_OK; });
  return n;
}
// a new handle that `build` has filled, or null (no memory, or build threw: reported as guarded reports it)
template <typename H, typename F> static H *make_handle(F &&build) {
  H *h = new (std::nothrow) H;
  if (h && guarded([&] { build(*h); return LIO_OK; }) != LIO_OK) { delete h; h = nullptr; }
  return h;
}
// no pointer twice (null entries are the caller's to refuse)
template <typename T> static bool distinct(T *const *ptrs, size_t n) {
  std::vector<const void *> sorted(ptrs, ptrs + n);
  std::sort(sorted.begin(), sorted.end(), std::less<const void *>());
  return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
}

// The processors that hold the handles' last sweeps, ready to be read for as long as the lease lives: the handle's own one, or sweep
// pool_sweep of the one it shares.  The distinct shared ones are locked in address order (one order for every caller) until the lease
// goes; a handle whose pool has run another batch since is refused; a sweep still in flight (lio_pp_process_async) is waited for.
// A null handle (or a null array) gives an empty slot.  What differs between the readers is theirs to say: `capacity_is_state` reports a
// processor that ended over capacity as the reader's state error instead of passing its own capacity error on, `need_results` refuses a
// processor without a completed sweep, and selecting the sweep (SelectSweep) is the reader's call.
class PpLease {
 public:
  PpLease(const lio_pp *const *handles, size_t n, const char *who, bool capacity_is_state, bool need_results) : slot_(handles ? n : 0) {
    std::vector<lio_pp_pool *> pools;
    for (size_t k = 0; k < slot_.size(); ++k)
      if (handles[k] && shared(handles[k])) pools.push_back(handles[k]->pool.get());
    std::sort(pools.begin(), pools.end(), std::less<lio_pp_pool *>());
    pools.erase(std::unique(pools.begin(), pools.end()), pools.end());
    for (lio_pp_pool *p : pools) locks_.emplace_back(p->mu);
    for (size_t k = 0; k < slot_.size(); ++k) {
      const lio_pp *h = handles[k];
      if (!h) continue;   // an empty slot
      if (shared(h) && h->pool_gen != h->pool->gen)
        throw std::runtime_error(std::string(who) + ": a processor's batch results were overwritten by a later lio_pp_process_batch on the storage it shared");
      PointProcessorDev &p = shared(h) ? h->pool->pp : *h->pp;
      try { p.ProcessFinish(); }
      catch (const CapacityError &e) { if (!capacity_is_state) throw; throw std::runtime_error(e.what()); }
      if (need_results && !p.has_results()) throw std::runtime_error(std::string(who) + ": a processor has no completed sweep");
      slot_[k] = {&p, shared(h) ? h->pool_sweep : 0};
    }
  }
  static bool shared(const lio_pp *h) { return h->pool && h->pool_sweep >= 0; }
  PointProcessorDev *pp(size_t k) const { return k < slot_.size() ? slot_[k].pp : nullptr; }   // null: an empty slot
  int sweep(size_t k) const { return slot_[k].sweep; }

 private:
  struct Slot { PointProcessorDev *pp = nullptr; int sweep = 0; };
  std::vector<Slot> slot_;
  std::vector<std::unique_lock<std::mutex>> locks_;
};
// The hand-over from the odometry to the next stage (mapping.h: OdomSweep): the handle's last clouds and transform_sum_ where they lie on the
// device, and the ring cloud of slot k's processor through the handle's TransformToEnd as the full cloud (an empty slot: full.set false).
// The sources are valid only while `lease` lives: the caller holds it until the chain that reads them has returned synchronised.
static OdomSweep odom_sweep(const lio_odom *odom, const PpLease &lease, size_t k) {
  const OdometryDev::DeviceView v = odom->o->View();
  OdomSweep S{v.last[0], v.last[1], odom->o->transform_sum_, MapFullSource{}};
  if (lease.pp(k)) {
    S.full.set = true;
    lease.pp(k)->DeviceRings(lease.sweep(k), S.full.pts, S.full.n);
    S.full.to_end = v.to_end;
  }
  return S;
}
// f(the processor that holds the handle's last sweep, that sweep selected)
template <typename F> static int pp_read(const lio_pp *h, F &&f) {
  return guarded([&] {
    PpLease lease(&h, 1, "lio_pp", false, false);
    PointProcessorDev &p = *lease.pp(0);
    if (PpLease::shared(h)) p.SelectSweep(lease.sweep(0));   // (a handle's own processor has one sweep, selected since it finished)
    f(p);
    return LIO_OK;
  });
}

// The front the two batch calls share, behind the caller's own null checks: the refusals in the order the headers state them (the sensor
// count; a null handle or what `arg_ok(k)` refuses of sensor k's other arguments; the same handle twice; an estimator's map), then the
// handles' devices in the caller's order.  Nothing here touches the device or a handle.
template <typename ArgOk> static int map_batch_devices(lio_map *const *handles, int n, ArgOk &&arg_ok, std::vector<MappingDev *> &m) {
  if (n > LIO_MAP_BATCH_MAX_SENSORS) return LIO_ERR_CAPACITY;
  for (int k = 0; k < n; ++k)
    if (!handles[k] || !arg_ok(k)) return LIO_ERR_ARG;
  if (!distinct(handles, size_t(n))) return LIO_ERR_ARG;
  for (int k = 0; k < n; ++k)
    if (handles[k]->borrowed || !handles[k]->m) return LIO_ERR_STATE;   // an estimator's map (lio_est_map) is stepped by its estimator
  for (int k = 0; k < n; ++k) m.push_back(handles[k]->m.get());
  return LIO_OK;
}
// the stateless blocks' device scratch, one per host thread
struct Scratch {
  hipStream_t s = nullptr;
  DBuf<float4> a, b, coef, abs_coef;
  VoxelGridDev vox;
  KnnGrid grid;
  DBuf<uint8_t> valid;
  DBuf<float> score, tf, sqd, nbr;
  DBuf<int32_t> idx;
  DBuf<double> gn_partials, gn_sums;   // the Gauss-Newton hooks
  DBuf<OdomState> gn_state;
  DBuf<KfDesc> gn_kd;
  DBuf<float> gn_rows;
  float tf_host[8];
  // The round trip of a stateless block, all on `s`: up(), the launches, down(), one sync() at the end (host memory handed to up() lives until then).
  // host -> device.  The buffer holds at least one element (the kernels take its pointer when n == 0 too); an empty upload is skipped
  template <typename T> void up(DBuf<T> &d, const void *src, size_t n) {
    room(d, n);
    if (n) LIO_HIP(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
  }
  template <typename T> void room(DBuf<T> &d, size_t n) { d.reserve(std::max<size_t>(n, 1)); }   // for n results
  template <typename T> void down(void *dst, const T *src, size_t n) {   // device -> host; an empty download is skipped
    if (n) LIO_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, s));
  }
  void sync() { LIO_HIP(hipStreamSynchronize(s)); }
  void up_tf(const lio_transform_f &T) {   // into `tf`, as the feature kernels read a transform: q (x y z w), p, pad
    const float v[8] = {T.q[0], T.q[1], T.q[2], T.q[3], T.p[0], T.p[1], T.p[2], 0.f};
    std::memcpy(tf_host, v, sizeof(v));
    up(tf, tf_host, 8);
  }
  // the K-NN grid of cell edge `cell` over the host map that up() has put into `a`
  void grid_over_a(const float *map, size_t n_map, float cell) {
    float mn[3], mx[3];
    host_cloud_bounds(map, n_map, mn, mx);
    grid.build(a.p, n_map, mn, mx, cell, s);
  }
};
// one frame of M points at tf_index 0, slots from 0
static FeatArgs one_frame(const float4 *stack, int M, float mm, float mp) {
  FeatArgs fa{};
  fa.nframes = 1; fa.max_M = M; fa.min_match_sq_dis = mm; fa.min_plane_dis = mp;
  fa.fr[0].stack = stack; fa.fr[0].M = M; fa.fr[0].slot_off = 0; fa.fr[0].tf_index = 0;
  return fa;
}
static Scratch &scratch() {
  static thread_local Scratch sc;
  if (!sc.s) {
    int nd = 0;
    LIO_HIP(hipGetDeviceCount(&nd));
    if (nd <= 0) throw DeviceError("no HIP device: the product has no CPU path");
    LIO_HIP(hipStreamCreate(&sc.s));
  }
  return sc;
}

// the prior's linearization point, block after block: read into `out` (null: only counted) or, with `in`, written from it; the length
static int prior_x0(MargPrior &pr, double *out, const double *in = nullptr) {
  int len = 0;
  for (auto &b : pr.x0)
    for (double &v : b) { if (in) v = in[len]; else if (out) out[len] = v; ++len; }
  return len;
}
// the last marginalization's prior as one n x n matrix and one n-vector of it (picked by `mat` / `vec`) and x0; returns n, 0 without a prior
template <typename Mat, typename Vec> static int est_get_prior(const lio_est *h, Mat &&mat, Vec &&vec, double *M, double *v, double *x0, int *x0_len) {
  if (!h) return LIO_ERR_ARG;
  // JoinMarg rethrows a failed worker task: nothing may unwind through the C boundary
  return guarded([&] {
    h->e->JoinMarg();
    const auto &pr = h->e->last_marg_;
    if (!pr) return 0;
    const int n = pr->n;
    if (M) std::memcpy(M, mat(*pr), sizeof(double) * size_t(n) * n);
    if (v) std::memcpy(v, vec(*pr), sizeof(double) * n);
    const int len = prior_x0(*pr, x0);
    if (x0_len) *x0_len = len;
    return n;
  });
}

extern "C" {

const char *lio_backend(void) { return "hip-gfx950"; }

// ---------------------------------------------------------------- PointProcessor
void lio_pp_default_config(lio_pp_config *c) {
  if (!c) return;
  c->scan_period = 0.1; c->num_scan_subregions = 8; c->num_curvature_regions = 5; c->surf_curv_th = 0.1f;
  c->max_corner_sharp = 2; c->max_corner_less_sharp = 20; c->max_surf_flat = 4; c->less_flat_filter_size = 0.2f;
  c->infer_start_ori = 0; c->rad_diff = 0.2;
}
static lio_pp_config pp_config_or_default(const lio_pp_config *c) {
  lio_pp_config cfg;
  if (c) cfg = *c; else lio_pp_default_config(&cfg);
  return cfg;
}
static int pp_check_config(float lo, float up, int rings, const lio_pp_config &cfg) {
  if (rings <= 0 || rings > LIO_PP_MAX_RINGS || !(up > lo)) return LIO_ERR_ARG;
  if (cfg.num_scan_subregions < 1 || cfg.num_scan_subregions > 16 || cfg.num_curvature_regions < 1 || cfg.num_curvature_regions > 8) return LIO_ERR_ARG;
  // pick caps size LDS tables and device reserves; the leaf is inverted: keep them in sane ranges
  const int caps[3] = {cfg.max_corner_sharp, cfg.max_corner_less_sharp, cfg.max_surf_flat};
  for (int v : caps)
    if (v < 0 || v > 4096) return LIO_ERR_ARG;
  if (cfg.max_corner_sharp > cfg.max_corner_less_sharp) return LIO_ERR_ARG;
  if (!(cfg.less_flat_filter_size > 1e-4f && cfg.less_flat_filter_size < 1e4f)) return LIO_ERR_ARG;
  if (!(cfg.scan_period > 0.0f) || !std::isfinite(cfg.scan_period)) return LIO_ERR_ARG;
  if (cfg.infer_start_ori && !(cfg.rad_diff >= 0.0)) return LIO_ERR_ARG;
  // k_ring_pick keeps the picks of a subregion one per lane of a wave (corner picks + flat picks in 64 slots): a fixed capacity of
  // the device path, reported as such (the reference accepts any quota; its defaults are 20 + 4)
  if (cfg.max_corner_less_sharp + cfg.max_surf_flat > 64) return LIO_ERR_CAPACITY;
  return LIO_OK;
}
int lio_pp_check_config(float lo, float up, int rings, const lio_pp_config *c) { return pp_check_config(lo, up, rings, pp_config_or_default(c)); }
lio_pp *lio_pp_create(float lo, float up, int rings, const lio_pp_config *c) {
  const lio_pp_config cfg = pp_config_or_default(c);
  const int chk = pp_check_config(lo, up, rings, cfg);
  if (chk != LIO_OK) {
    if (chk == LIO_ERR_CAPACITY)
      std::fprintf(stderr, "lio_pp_create: LIO_ERR_CAPACITY — max_corner_less_sharp + max_surf_flat > 64 picks per subregion is beyond k_ring_pick's per-wave pick table "
                           "(lio_pp_check_config reports the code)\n");
    return nullptr;
  }
  return make_handle<lio_pp>([&](lio_pp &h) { h.pp.reset(new PointProcessorDev(lo, up, rings, cfg)); });
}
void lio_pp_destroy(lio_pp *h) { delete h; }
float lio_pp_start_ori(const lio_pp *h) {
  if (!h) return std::nanf("");
  float v = std::nanf("");
  pp_read(h, [&](PointProcessorDev &p) { v = p.StartOri(); });
  return v;
}
int lio_pp_process(lio_pp *h, const float *xyzi, size_t n) {
  if (!h || (!xyzi && n)) return LIO_ERR_ARG;
  h->pool_sweep = -1;
  return guarded([&] { h->pp->Process(xyzi, n); return LIO_OK; });
}
int lio_pp_process_async(lio_pp *h, const float *xyzi, size_t n) {
  if (!h || (!xyzi && n)) return LIO_ERR_ARG;
  h->pool_sweep = -1;
  return guarded([&] { h->pp->ProcessLaunch(xyzi, n); return LIO_OK; });
}
int lio_pp_wait(lio_pp *h) {
  if (!h) return LIO_ERR_ARG;
  return guarded([&] { h->pp->ProcessFinish(); return LIO_OK; });
}
static int pp_process_batch(lio_pp *const *handles, const float *const *xyzi, const size_t *n, int n_sweeps, bool on_device,
                            const uint16_t *const *ring = nullptr) {
  if (n_sweeps < 0 || (n_sweeps > 0 && (!handles || !xyzi || !n))) return LIO_ERR_ARG;
  bool same = true;
  for (int k = 0; k < n_sweeps; ++k) {
    if (!handles[k] || (!xyzi[k] && n[k]) || (ring && !ring[k] && n[k])) return LIO_ERR_ARG;
    same = same && handles[k]->pp->SameSensor(*handles[0]->pp);
  }
  if (n_sweeps == 0) return LIO_OK;
  if (!distinct(handles, size_t(n_sweeps))) return LIO_ERR_ARG;
  if (n_sweeps >= 2 && same) {
    // ONE launch chain over all sweeps: the handles share a multi-sweep processor (kept for the next call), every handle reads its own
    // sweep of it; a sweep's start azimuth still goes through ITS handle's ten-sweep history (infer_start_ori)
    return guarded([&] {
      std::shared_ptr<lio_pp_pool> pool = handles[0]->pool;
      if (!pool || !pool->pp.SameSensor(*handles[0]->pp)) {
        const PointProcessorDev &a = *handles[0]->pp;
        pool = std::make_shared<lio_pp_pool>(a.lower(), a.upper(), a.rings(), a.config());
      }
      std::vector<StartOriFilter *> filters(static_cast<size_t>(n_sweeps));
      std::vector<CloudSrc> sweeps(static_cast<size_t>(n_sweeps));
      for (int k = 0; k < n_sweeps; ++k) sweeps[size_t(k)] = CloudSrc::at(xyzi[k], n[k], on_device);
      std::lock_guard<std::mutex> lk(pool->mu);
      ++pool->gen;   // the chain overwrites the pool's storage: every lease on it ends here
      // Everything below can throw (a handle's own sweep still in flight may have ended over capacity), and nothing is served of a failed
      // call: until the chain has finished, the handles of the call hold a lease on nothing
      for (int k = 0; k < n_sweeps; ++k) { handles[k]->pool = pool; handles[k]->pool_sweep = k; handles[k]->pool_gen = 0; }
      const auto lease = [&] { for (int k = 0; k < n_sweeps; ++k) handles[k]->pool_gen = pool->gen; };
      for (int k = 0; k < n_sweeps; ++k) {
        handles[k]->pp->ProcessFinish();
        filters[size_t(k)] = &handles[k]->pp->start_ori_filter();
      }
      pool->pp.ProcessLaunchBatch(sweeps.data(), ring, n_sweeps, filters.data());
      try { pool->pp.ProcessFinish(); }
      catch (const CapacityError &) { lease(); throw; }   // finished, over capacity: the pool's processor reads zero for every sweep
      lease();
      return LIO_OK;
    });
  }
  // different sensors (or one sweep): every handle's own chain, all enqueued before the first is waited for
  int rc = LIO_OK, launched = 0;
  for (; launched < n_sweeps && rc == LIO_OK; ++launched) {
    lio_pp *h = handles[launched];
    h->pool_sweep = -1;
    rc = guarded([&] {
      StartOriFilter *f = &h->pp->start_ori_filter();
      const CloudSrc sweep = CloudSrc::at(xyzi[launched], n[launched], on_device);
      h->pp->ProcessLaunchBatch(&sweep, ring ? &ring[launched] : nullptr, 1, &f);
      return LIO_OK;
    });
  }
  if (rc != LIO_OK) --launched;   // (the failing handle has nothing in flight)
  for (int k = 0; k < launched; ++k) { const int r = lio_pp_wait(handles[k]); if (rc == LIO_OK) rc = r; }
  return rc;
}
int lio_pp_process_batch(lio_pp *const *handles, const float *const *xyzi, const size_t *n, int n_sweeps) {
  return pp_process_batch(handles, xyzi, n, n_sweeps, false);
}
int lio_pp_process_batch_device(lio_pp *const *handles, const float *const *d_xyzi, const size_t *n, int n_sweeps) {
  return pp_process_batch(handles, d_xyzi, n, n_sweeps, true);
}
int lio_pp_process_rings_batch(lio_pp *const *handles, const float *const *xyzi, const uint16_t *const *ring, const size_t *n, int n_sweeps) {
  if (n_sweeps > 0 && !ring) return LIO_ERR_ARG;
  return pp_process_batch(handles, xyzi, n, n_sweeps, false, ring);
}
int lio_pp_process_rings(lio_pp *h, const float *xyzi, const uint16_t *ring, size_t n) {
  if (!h || ((!xyzi || !ring) && n)) return LIO_ERR_ARG;
  h->pool_sweep = -1;
  return guarded([&] { h->pp->Process(xyzi, n, n ? ring : nullptr); return LIO_OK; });
}
size_t lio_pp_count(const lio_pp *h, int which) {
  if (!h || which < 0 || which > 4) return 0;
  size_t n = 0;
  pp_read(h, [&](PointProcessorDev &p) { n = p.Count(which); });
  return n;
}
int lio_pp_get_cloud(const lio_pp *h, int which, float *out) {
  if (!h || which < 0 || which > 4 || !out) return LIO_ERR_ARG;
  return pp_read(h, [&](PointProcessorDev &p) { p.GetCloud(which, out); });
}
int lio_pp_get_indices(const lio_pp *h, int which, int32_t *ring, int32_t *idx) {
  if (!h || which < 1 || which > 3 || !ring || !idx) return LIO_ERR_ARG;
  return pp_read(h, [&](PointProcessorDev &p) { p.GetIndices(which, ring, idx); });
}
int lio_pp_get_ring_offsets(const lio_pp *h, int32_t *out) {
  if (!h || !out) return LIO_ERR_ARG;
  return pp_read(h, [&](PointProcessorDev &p) { p.GetRingOffsets(out); });
}
int lio_pp_get_curvature(const lio_pp *h, float *curv, int32_t *mask) {
  if (!h) return LIO_ERR_ARG;
  return pp_read(h, [&](PointProcessorDev &p) { p.GetCurvature(curv, mask); });
}

int lio_pp_get_ring_intensity(const lio_pp *h, float *out) {
  if (!h || !out) return LIO_ERR_ARG;
  return pp_read(h, [&](PointProcessorDev &p) { p.GetRingIntensity(out); });
}

// ---------------------------------------------------------------- PointOdometry
lio_odom *lio_odom_create(float scan_period, int io_ratio, int max_iter, int no_deskew) {
  if (!(scan_period > 0) || max_iter < 1) return nullptr;
  return make_handle<lio_odom>([&](lio_odom &h) { h.o.reset(new OdometryDev(scan_period, io_ratio, max_iter, no_deskew != 0)); });
}
void lio_odom_destroy(lio_odom *h) { delete h; }
// the handles' devices in the caller's order; false: the same handle twice
static bool odom_devices(lio_odom *const *handles, int n, std::vector<OdometryDev *> &o) {
  for (int k = 0; k < n; ++k) o.push_back(handles[k]->o.get());
  return distinct(handles, size_t(n));
}
// what a step hands back per sensor; every array is optional
static void odom_results(OdometryDev *const *o, int n, lio_transform_f *Tsum, lio_transform_f *Tes, int32_t *iters, int32_t *nsel) {
  for (int k = 0; k < n; ++k) {
    const OdometryDev &d = *o[k];
    if (Tsum) fromT(d.transform_sum_, &Tsum[k]);
    if (Tes) fromT(d.transform_es_, &Tes[k]);
    if (iters) iters[k] = d.iterations_done_;
    if (nsel) nsel[k] = d.last_num_sel_;
  }
}
int lio_odom_process(lio_odom *h, const float *sharp, size_t n_sharp, const float *less_sharp, size_t n_ls, const float *flat, size_t n_flat,
                     const float *less_flat, size_t n_lf, lio_transform_f *Tsum, lio_transform_f *Tes, int *iters, int *nsel) {
  if (!h || (!sharp && n_sharp) || (!less_sharp && n_ls) || (!flat && n_flat) || (!less_flat && n_lf)) return LIO_ERR_ARG;
  return guarded([&] {
    OdometryDev *o = h->o.get();
    o->Process(sharp, n_sharp, less_sharp, n_ls, flat, n_flat, less_flat, n_lf);
    odom_results(&o, 1, Tsum, Tes, iters, nsel);
    return LIO_OK;
  });
}
// include/lio_odom_batch.h.  Every check comes before any device work and before any handle changes.
int lio_odom_process_batch(lio_odom *const *handles, int n_sensors, const float *const *sharp, const size_t *n_sharp, const float *const *less_sharp,
                           const size_t *n_ls, const float *const *flat, const size_t *n_flat, const float *const *less_flat, const size_t *n_lf,
                           lio_transform_f *Tsum, lio_transform_f *Tes, int32_t *iters, int32_t *nsel) {
  if (!handles || n_sensors < 1 || !sharp || !n_sharp || !less_sharp || !n_ls || !flat || !n_flat || !less_flat || !n_lf) return LIO_ERR_ARG;
  if (n_sensors > LIO_ODOM_BATCH_MAX_SENSORS) return LIO_ERR_CAPACITY;
  for (int k = 0; k < n_sensors; ++k)
    if (!handles[k] || (!sharp[k] && n_sharp[k]) || (!less_sharp[k] && n_ls[k]) || (!flat[k] && n_flat[k]) || (!less_flat[k] && n_lf[k])) return LIO_ERR_ARG;
  return guarded([&] {
    std::vector<OdometryDev *> o;
    if (!odom_devices(handles, n_sensors, o)) return int(LIO_ERR_ARG);
    std::vector<OdometryDev::Clouds> in(static_cast<size_t>(n_sensors));
    for (int k = 0; k < n_sensors; ++k)
      in[size_t(k)] = OdometryDev::Clouds{{CloudSrc::host(sharp[k], n_sharp[k]), CloudSrc::host(less_sharp[k], n_ls[k]), CloudSrc::host(flat[k], n_flat[k]), CloudSrc::host(less_flat[k], n_lf[k])}};
    OdometryDev::ProcessBatch(o.data(), n_sensors, in.data());
    odom_results(o.data(), n_sensors, Tsum, Tes, iters, nsel);
    return int(LIO_OK);
  });
}
// include/lio_frontend_batch.h.  The lease on the processors is held until the chain, which reads their clouds, has returned synchronised.
int lio_odom_process_batch_from_pp(lio_odom *const *handles, lio_pp *const *pp, int n_sensors, lio_transform_f *Tsum, lio_transform_f *Tes,
                                   int32_t *iters, int32_t *nsel) {
  if (!handles || !pp || n_sensors < 1) return LIO_ERR_ARG;
  if (n_sensors > LIO_ODOM_BATCH_MAX_SENSORS) return LIO_ERR_CAPACITY;
  for (int k = 0; k < n_sensors; ++k)
    if (!handles[k] || !pp[k]) return LIO_ERR_ARG;
  return guarded([&] {
    const size_t n = size_t(n_sensors);
    std::vector<OdometryDev *> o;
    if (!odom_devices(handles, n_sensors, o)) return int(LIO_ERR_ARG);
    const PpLease lease(pp, n, "lio_odom_process_batch_from_pp", true, true);
    std::vector<OdometryDev::Clouds> in(n);
    for (size_t k = 0; k < n; ++k) {
      const float4 *s4[4]; size_t n4[4];
      lease.pp(k)->DeviceClouds(lease.sweep(k), s4, n4);
      for (int c = 0; c < 4; ++c) in[k].c[c] = CloudSrc::device(s4[c], n4[c]);
    }
    OdometryDev::ProcessBatch(o.data(), n_sensors, in.data());
    odom_results(o.data(), n_sensors, Tsum, Tes, iters, nsel);
    return int(LIO_OK);
  });
}
int lio_odom_get_iteration_trace(const lio_odom *h, lio_transform_f *trace, int capacity, int *kz) {
  if (!h || capacity < 0 || (!trace && capacity)) return LIO_ERR_ARG;
  const int n = h->o->iterations_done_;
  for (int k = 0; k < n && k < capacity && k < int(h->o->es_trace_.size()); ++k) fromT(h->o->es_trace_[size_t(k)], &trace[k]);
  if (kz) *kz = h->o->last_kz_;
  return n;
}
int lio_odom_enable(lio_odom *h, int on) {
  if (!h) return LIO_ERR_ARG;
  h->o->enable_odom_ = on != 0;
  return LIO_OK;
}
size_t lio_odom_get_last_cloud(const lio_odom *h, int which, float *out) {
  if (!h || which < 0 || which > 1) return 0;
  return guarded_count([&] { return h->o->GetLastCloud(which, out); });
}

// ---------------------------------------------------------------- ImuInitializer (host)
static bool gatherLaserFrames(size_t n, const lio_transform_f *T, lio_pim *const *pims, std::vector<LaserFrame> &all) {
  all.resize(n);
  for (size_t i = 0; i < n; ++i) {
    all[i].transform = toT(T[i]);
    if (pims[i]) all[i].pim = pims[i]->p;
    else if (i != 0) return false;
  }
  return true;
}
int lio_imu_estimate_extrinsic_rotation(size_t n, const lio_transform_f *T, lio_pim *const *pims, lio_transform_f *lb) {
  if (n < 2 || !T || !pims || !lb) return LIO_ERR_ARG;
  std::vector<LaserFrame> all;
  if (!gatherLaserFrames(n, T, pims, all)) return LIO_ERR_ARG;
  return guarded([&] {
    Rigidf tlb = toT(*lb);
    const bool ok = estimate_extrinsic_rotation(all, tlb);
    fromT(tlb, lb);
    return ok ? 1 : 0;
  });
}
int lio_imu_initialization(size_t n, const lio_transform_f *T, lio_pim *const *pims, const lio_transform_f *lb, double *Vs, double *Bgs, double g[3],
                           double R_WI[9]) {
  if (n < 2 || !T || !pims || !lb || !Vs || !Bgs || !g || !R_WI) return LIO_ERR_ARG;
  std::vector<LaserFrame> all;
  if (!gatherLaserFrames(n, T, pims, all)) return LIO_ERR_ARG;
  return guarded([&] {
    std::vector<V3d> vs(n), bgs(n);
    for (size_t i = 0; i < n; ++i) bgs[i] = v3(Bgs + 3 * i);
    V3d gv;
    M3d R;
    R(0, 0) = R(1, 1) = R(2, 2) = 1.0;
    const bool ok = imu_initialization(all, vs, bgs, gv, toT(*lb), R);
    for (size_t i = 0; i < n; ++i) {
      Vs[3 * i] = vs[i].x; Vs[3 * i + 1] = vs[i].y; Vs[3 * i + 2] = vs[i].z;
      Bgs[3 * i] = bgs[i].x; Bgs[3 * i + 1] = bgs[i].y; Bgs[3 * i + 2] = bgs[i].z;
    }
    g[0] = gv.x; g[1] = gv.y; g[2] = gv.z;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R_WI[r * 3 + c] = R(r, c);
    return ok ? 1 : 0;
  });
}

// ---------------------------------------------------------------- PointMapping
void lio_map_default_config(lio_map_config *c) {
  if (!c) return;
  c->corner_filter_size = 0.2f; c->surf_filter_size = 0.4f; c->min_match_sq_dis = 1.0f; c->min_plane_dis = 0.2f; c->num_max_iterations = 10;
  c->map_builder = 0; c->enable_4d = 1; c->skip_count = 2;
}
lio_map *lio_map_create(const lio_map_config *c) {
  lio_map_config cfg;
  if (c) cfg = *c; else lio_map_default_config(&cfg);
  if (!(cfg.corner_filter_size > 0) || !(cfg.surf_filter_size > 0) || cfg.num_max_iterations < 1) return nullptr;
  if (cfg.map_builder && cfg.skip_count < 1) return nullptr;
  return make_handle<lio_map>([&](lio_map &h) { h.m.reset(new MappingDev(cfg)); });
}
void lio_map_destroy(lio_map *h) {
  if (h && h->borrowed) { std::fprintf(stderr, "[lio_hip] lio_map_destroy: the handle belongs to a lio_est (lio_est_map); ignored\n"); return; }
  delete h;
}
// what a step hands back per handle; every array is optional
static void map_results(MappingDev *const *m, int n, lio_transform_f *Taft, int32_t *iters, int32_t *nsel) {
  for (int k = 0; k < n; ++k) {
    if (Taft) fromT(m[k]->transform_aft_mapped_, &Taft[k]);
    if (iters) iters[k] = m[k]->iterations_;
    if (nsel) nsel[k] = m[k]->num_selected_;
  }
}
int lio_map_process(lio_map *h, const float *corner, size_t nc, const float *surf, size_t ns, const lio_transform_f *Tsum, lio_transform_f *Taft,
                    int *iters, int *nsel) {
  if (!h || !Tsum || (!corner && nc) || (!surf && ns)) return LIO_ERR_ARG;
  return guarded([&] {
    MappingDev *m = h->m.get();
    m->Process(corner, nc, surf, ns, toT(*Tsum));
    map_results(&m, 1, Taft, iters, nsel);
    return LIO_OK;
  });
}
// include/lio_map_batch.h.  Every check comes before any device work and before any handle changes.
int lio_map_process_batch(lio_map *const *handles, int n_sensors, const float *const *corner, const size_t *nc, const float *const *surf, const size_t *ns,
                          const lio_transform_f *Tsum, lio_transform_f *Taft, int32_t *iters, int32_t *nsel) {
  if (!handles || n_sensors < 1 || !corner || !nc || !surf || !ns || !Tsum) return LIO_ERR_ARG;
  std::vector<MappingDev *> m;
  const int rc = map_batch_devices(handles, n_sensors, [&](int k) { return (corner[k] || !nc[k]) && (surf[k] || !ns[k]); }, m);
  if (rc != LIO_OK) return rc;
  return guarded([&] {
    std::vector<OdomSweep> sweeps(static_cast<size_t>(n_sensors));
    for (int k = 0; k < n_sensors; ++k) sweeps[size_t(k)] = OdomSweep{CloudSrc::host(corner[k], nc[k]), CloudSrc::host(surf[k], ns[k]), toT(Tsum[k]), MapFullSource{}};
    MappingDev::ProcessBatch(m.data(), n_sensors, sweeps.data());
    map_results(m.data(), n_sensors, Taft, iters, nsel);
    return int(LIO_OK);
  });
}
// include/lio_map_from_odom.h.  Every check comes before any device work and before any handle changes; the lease on the processors is
// held until the chain, which reads their clouds, has returned synchronised.  A null `pp`, or a null entry: this handle's full cloud stays.
int lio_map_process_batch_from_odom(lio_map *const *handles, lio_odom *const *odom, lio_pp *const *pp, int n_sensors, lio_transform_f *Taft,
                                    int32_t *iters, int32_t *nsel) {
  if (!handles || !odom || n_sensors < 1) return LIO_ERR_ARG;
  std::vector<MappingDev *> m;
  const int rc = map_batch_devices(handles, n_sensors, [&](int k) { return odom[k] != nullptr; }, m);
  if (rc != LIO_OK) return rc;
  for (int k = 0; k < n_sensors; ++k)
    if (!odom[k]->o->processed()) return LIO_ERR_STATE;   // no sweep to hand over
  return guarded([&] {
    const size_t n = size_t(n_sensors);
    const PpLease lease(pp, n, "lio_map_process_batch_from_odom", true, true);
    std::vector<OdomSweep> sweeps(n);
    for (size_t k = 0; k < n; ++k) sweeps[k] = odom_sweep(odom[k], lease, k);
    MappingDev::ProcessBatch(m.data(), n_sensors, sweeps.data());
    map_results(m.data(), n_sensors, Taft, iters, nsel);
    return int(LIO_OK);
  });
}
int lio_map_get_degeneracy(const lio_map *h, int *kz) {
  if (!h) return LIO_ERR_ARG;
  if (kz) *kz = h->m->kz_;
  return h->m->degenerate_ ? 1 : 0;
}
int lio_map_set_init_flag(lio_map *h, int on) {
  if (!h) return LIO_ERR_ARG;
  h->m->imu_inited_ = on != 0;
  return LIO_OK;
}
int lio_map_set_transform_tobe_mapped(lio_map *h, const lio_transform_f *T) {
  if (!h || !T) return LIO_ERR_ARG;
  h->m->transform_tobe_mapped_ = toT(*T);
  return LIO_OK;
}
int lio_map_get_transform_tobe_mapped(const lio_map *h, lio_transform_f *T) {
  if (!h || !T) return LIO_ERR_ARG;
  fromT(h->m->transform_tobe_mapped_, T);
  return LIO_OK;
}
int lio_map_update_map_database(lio_map *h, const float *corner, size_t nc, const float *surf, size_t ns, const uint32_t *valid, size_t nv,
                                const lio_transform_f *T, const int cen[3]) {
  if (!h || !T || !cen || (!corner && nc) || (!surf && ns) || (!valid && nv)) return LIO_ERR_ARG;
  for (size_t i = 0; i < nv; ++i)
    if (valid[i] >= uint32_t(MappingDev::L * MappingDev::Wd * MappingDev::H)) return LIO_ERR_ARG;
  return guarded([&] { h->m->UpdateMapDatabase(corner, nc, surf, ns, valid, nv, toT(*T), cen); return LIO_OK; });
}
size_t lio_map_get_cloud(const lio_map *h, int which, float *out) {
  if (!h || which < 0 || which > 3) return 0;
  return guarded_count([&] { return h->m->GetCloud(which, out); });
}
size_t lio_map_get_cube(const lio_map *h, int cls, uint32_t idx, float *out) {
  if (!h || cls < 0 || cls > 1 || idx >= uint32_t(MappingDev::L * MappingDev::Wd * MappingDev::H)) return 0;
  return guarded_count([&] { return h->m->GetCube(cls, idx, out); });
}
size_t lio_map_get_cube_state(const lio_map *h, int cen[3], uint32_t *valid) {
  if (!h) return 0;
  if (cen) for (int d = 0; d < 3; ++d) cen[d] = h->m->cen_[d];
  if (valid) for (size_t i = 0; i < h->m->valid_idx_.size(); ++i) valid[i] = h->m->valid_idx_[i];
  return h->m->valid_idx_.size();
}
size_t lio_map_get_score_point_coeff(const lio_map *h, float *score, float *point, float *coeff) {
  if (!h) return 0;
  return guarded_count([&] { return h->m->GetScorePointCoeff(score, point, coeff); });
}

// ---------------------------------------------------------------- batched keyframe refinement
struct lio_kf_batch { std::unique_ptr<KfBatchDev> b; };
lio_kf_batch *lio_kf_batch_create(const lio_map_config *c) {
  lio_map_config cfg;
  if (c) cfg = *c; else lio_map_default_config(&cfg);
  if (cfg.num_max_iterations < 1) return nullptr;
  return make_handle<lio_kf_batch>([&](lio_kf_batch &h) { h.b.reset(new KfBatchDev(cfg)); });
}
void lio_kf_batch_destroy(lio_kf_batch *h) { delete h; }
int lio_kf_batch_add_map(lio_kf_batch *h, const float *corner, size_t nc, const float *surf, size_t ns) {
  if (!h || (!corner && nc) || (!surf && ns)) return LIO_ERR_ARG;
  int idx = -1;
  int rc = guarded([&] { idx = h->b->AddMap(corner, nc, surf, ns); return LIO_OK; });
  return rc == LIO_OK ? idx : rc;
}
int lio_kf_batch_add_keyframe(lio_kf_batch *h, int map, const float *corner, size_t nc, const float *surf, size_t ns, const lio_transform_f *T) {
  if (!h || !T || (!corner && nc) || (!surf && ns) || map < 0 || size_t(map) >= h->b->n_maps()) return LIO_ERR_ARG;
  int idx = -1;
  int rc = guarded([&] { idx = h->b->AddKeyframe(map, corner, nc, surf, ns, toT(*T)); return LIO_OK; });
  return rc == LIO_OK ? idx : rc;
}
int lio_kf_batch_clear_keyframes(lio_kf_batch *h) {
  if (!h) return LIO_ERR_ARG;
  h->b->ClearKeyframes();
  return LIO_OK;
}
size_t lio_kf_batch_size(const lio_kf_batch *h) { return h ? h->b->n_keyframes() : 0; }
int lio_kf_batch_refine(lio_kf_batch *h, lio_transform_f *T_out, int32_t *iters, int32_t *rows, double *device_ms) {
  if (!h) return LIO_ERR_ARG;
  return guarded([&] {
    h->b->Refine();
    const auto &st = h->b->states();
    for (size_t k = 0; k < st.size(); ++k) {
      if (T_out) fromT(Rigidf(Quat<float>(st[k].T[3], st[k].T[0], st[k].T[1], st[k].T[2]), Vec3<float>(st[k].T[4], st[k].T[5], st[k].T[6])), &T_out[k]);
      if (iters) iters[k] = st[k].iters;
      if (rows) rows[k] = st[k].nsel;
    }
    if (device_ms) *device_ms = h->b->device_ms_;
    return LIO_OK;
  });
}
int lio_kf_batch_get_degeneracy(const lio_kf_batch *h, int32_t *kz_out) {
  if (!h || !kz_out) return LIO_ERR_ARG;
  const auto &st = h->b->states();
  if (st.size() != h->b->n_keyframes()) return LIO_ERR_STATE;   // no refine since the keyframe list changed
  for (size_t k = 0; k < st.size(); ++k) kz_out[k] = st[k].kz;
  return LIO_OK;
}
int lio_kf_batch_refine_gather(lio_kf_batch *h, lio_rccl *comm, int slots_per_rank, float *packed_all, double *device_ms) {
  if (!h || !comm || !packed_all || slots_per_rank < 1) return LIO_ERR_ARG;
  // collective precondition, checked before any device work: slots_per_rank is the SAME on every rank and >= every rank's
  // keyframe count (a rank that returned here would leave its peers waiting in ncclAllGather — the caller sizes it from the
  // global maximum, dist_util.refine_keyframes_sharded)
  if (size_t(slots_per_rank) < h->b->n_keyframes()) return LIO_ERR_CAPACITY;
  return guarded([&] {
    h->b->RefineGather(rccl_raw_comm(comm), lio_rccl_world(comm), slots_per_rank, packed_all);
    if (device_ms) *device_ms = h->b->device_ms_;
    return LIO_OK;
  });
}

// ---------------------------------------------------------------- /compact_data codec (host: a memcpy-class wire format)
size_t lio_compact_encode(const lio_transform_f *T, const float *corner, size_t nc, const float *surf, size_t ns, const float *full, size_t nf,
                          float *out) {
  if (!T || !out || (!corner && nc) || (!surf && ns) || (!full && nf)) return 0;
  float *o = out;
  *o++ = T->p[0]; *o++ = T->p[1]; *o++ = T->p[2]; *o++ = 0.f;
  *o++ = T->q[0]; *o++ = T->q[1]; *o++ = T->q[2]; *o++ = T->q[3];
  *o++ = float(nc); *o++ = float(ns); *o++ = float(nf); *o++ = T->q[3];  // the reused PointT keeps intensity = qw
  const float *src[3] = {corner, surf, full};
  const size_t cnt[3] = {nc, ns, nf};
  for (int k = 0; k < 3; ++k) { if (cnt[k]) std::memcpy(o, src[k], cnt[k] * 4 * sizeof(float)); o += 4 * cnt[k]; }
  return size_t(o - out) / 4;
}
int lio_compact_decode(const float *d, size_t n, lio_transform_f *T, size_t *nc, size_t *ns, size_t *nf) {
  if (!d || !nc || !ns || !nf || n < 4) return LIO_ERR_ARG;
  // the three sizes are untrusted wire floats: reject NaN / Inf / negative / larger-than-the-message values BEFORE any
  // float -> integer cast (undefined behaviour otherwise) and before they are summed
  const float lim = float(n);
  for (int k = 8; k <= 10; ++k)
    if (!(d[k] >= 0.0f && d[k] <= lim)) return LIO_ERR_ARG;
  const unsigned long long c = (unsigned long long)d[8], s = (unsigned long long)d[9], f = (unsigned long long)d[10];
  if (3ull + c + s + f != (unsigned long long)n) return LIO_ERR_ARG;
  if (T) { for (int k = 0; k < 3; ++k) T->p[k] = d[k]; for (int k = 0; k < 4; ++k) T->q[k] = d[4 + k]; }
  *nc = size_t(c); *ns = size_t(s); *nf = size_t(f);
  return LIO_OK;
}

// ---------------------------------------------------------------- stateless blocks
int lio_voxel_grid(const float *xyzi, size_t n, float leaf, float *out, size_t *n_out) {
  if ((!xyzi && n) || !out || !n_out || !(leaf > 0)) return LIO_ERR_ARG;
  return guarded([&] {
    Scratch &sc = scratch();
    sc.up(sc.a, xyzi, n);
    size_t m = sc.vox.run(sc.a.p, n, leaf, sc.b, sc.s);
    sc.down(out, sc.b.p, m);
    sc.sync();
    *n_out = m;
    return LIO_OK;
  });
}

// include/lio_vox_sort.h
static_assert(LIO_VOX_SORT_SAMPLE == VSORT_PATH_SAMPLE && LIO_VOX_SORT_SINGLE == VSORT_PATH_SINGLE && LIO_VOX_SORT_LIBRARY == VSORT_PATH_LIBRARY &&
              LIO_VOX_SORT_SINGLE_MAX == VSORT_CAP && LIO_VOX_SORT_BUCKET_CAP == VSORT_CAP && LIO_VOX_SORT_MEAN_BUCKET == VSORT_MEAN &&
              LIO_VOX_SORT_OVERSAMPLE == VSORT_OVERSAMPLE && LIO_VOX_SORT_SAMPLE_MAX == VSORT_MAX_N, "the header states the sizing rule of cloud_kernels.h");
int lio_vox_sort_pairs(const uint32_t *keys, size_t n, uint32_t *keys_out, uint32_t *vals_out, int *path_out) {
  if (!keys || n == 0 || !keys_out || !vals_out) return LIO_ERR_ARG;
  if (n >= size_t(INT_MAX)) return LIO_ERR_CAPACITY;
  return guarded([&] {
    Scratch &sc = scratch();
    const int path = sc.vox.sort_pairs_hook(keys, n, keys_out, vals_out, sc.s);
    if (path_out) *path_out = path;
    return LIO_OK;
  });
}
int lio_vox_sort_stats(uint64_t out[3]) {
  if (!out) return LIO_ERR_ARG;
  return guarded([&] {
    unsigned long long c[3];
    scratch().vox.sort_stats(c);
    for (int k = 0; k < 3; ++k) out[k] = c[k];
    return LIO_OK;
  });
}

// include/lio_seg_bounds.h
static_assert(sizeof(lio_seg_bounds_out) == sizeof(VoxParams) && offsetof(lio_seg_bounds_out, minb) == offsetof(VoxParams, minb) &&
              offsetof(lio_seg_bounds_out, n_valid) == offsetof(VoxParams, n_valid), "the header states VoxParams");
int lio_seg_bounds(const float *const *xyzi, const size_t *n, int nseg, float inv_leaf, lio_seg_bounds_out *out) {
  if (!xyzi || !n || nseg < 1 || !(inv_leaf > 0) || !out) return LIO_ERR_ARG;
  for (int k = 0; k < nseg; ++k) {
    if (!xyzi[k] && n[k]) return LIO_ERR_ARG;
    if (n[k] >= size_t(INT_MAX)) return LIO_ERR_CAPACITY;
  }
  return guarded([&] {
    Scratch &sc = scratch();
    hipStream_t s = sc.s;
    std::vector<DBuf<float4>> clouds(static_cast<size_t>(nseg));
    GridBatch gb;
    gb.begin(0, nseg);
    for (int k = 0; k < nseg; ++k) {
      DBuf<float4> &c = clouds[size_t(k)];
      sc.up(c, xyzi[k], n[k]);
      gb.add(c.p, int(n[k]));
    }
    std::memcpy(out, gb.bounds(s, inv_leaf), size_t(nseg) * sizeof(VoxParams));
    return LIO_OK;
  });
}

int lio_knn(const float *map, size_t n_map, const float *query, size_t m, int k, float radius_sq, int32_t *idx, float *sqd) {
  if ((!map && n_map) || (!query && m) || !(k == 1 || k == 5) || !idx || !sqd) return LIO_ERR_ARG;
  if (!(radius_sq > 0)) return LIO_ERR_ARG;  // the GPU search is radius-bounded by construction
  if (m > size_t(INT_MAX) / 8 || n_map > size_t(INT_MAX)) return LIO_ERR_CAPACITY;   // eight lanes per query, int thread ids
  return guarded([&] {
    Scratch &sc = scratch();
    sc.up(sc.a, map, n_map); sc.up(sc.b, query, m);
    sc.room(sc.idx, m * k); sc.room(sc.sqd, m * k);
    sc.grid_over_a(map, n_map, knn_cell_edge(radius_sq));
    launch_knn(sc.b.p, int(m), k, radius_sq, sc.grid.sorted(), sc.grid.cells(), sc.grid.desc(), sc.idx.p, sc.sqd.p, sc.s);
    sc.down(idx, sc.idx.p, m * k); sc.down(sqd, sc.sqd.p, m * k);
    sc.sync();
    return LIO_OK;
  });
}

int lio_knn_walk(const float *map, size_t n_map, const float *query, size_t m, float cell, int lanes_per_query, int32_t *idx, float *sqd,
                 float *nbr_xyz) {
  if ((!map && n_map) || (!query && m) || !idx || !sqd || !nbr_xyz || !(cell > 0) || !std::isfinite(cell)) return LIO_ERR_ARG;
  if (!(lanes_per_query == 1 || lanes_per_query == 4 || lanes_per_query == 8)) return LIO_ERR_ARG;   // the forms the product launches
  if (m > size_t(INT_MAX) / 8 || n_map > size_t(INT_MAX)) return LIO_ERR_CAPACITY;
  return guarded([&] {
    Scratch &sc = scratch();
    sc.up(sc.a, map, n_map); sc.up(sc.b, query, m);
    sc.room(sc.idx, m * 5); sc.room(sc.sqd, m * 5); sc.room(sc.nbr, m * 15);
    sc.grid_over_a(map, n_map, cell);
    launch_knn_walk(sc.b.p, int(m), lanes_per_query, sc.grid.sorted(), sc.grid.cells(), sc.grid.desc(), sc.idx.p, sc.sqd.p, sc.nbr.p, sc.s);
    sc.down(idx, sc.idx.p, m * 5); sc.down(sqd, sc.sqd.p, m * 5); sc.down(nbr_xyz, sc.nbr.p, m * 15);
    sc.sync();
    return LIO_OK;
  });
}

int lio_fit_five(int form, const float *nbr_xyz, const float *fifth_sqd, const float *stack, size_t m, const lio_transform_f *T,
                 const float *fixed_pz, float mm, float mp, uint8_t *valid, float *coeff, float *score, float *abs_coeff) {
  if (form < 0 || form > 3 || ((!nbr_xyz || !fifth_sqd || !stack) && m) || !T || !fixed_pz || !valid || !coeff || !score || !abs_coeff) return LIO_ERR_ARG;
  if (m > size_t(INT_MAX) / 5) return LIO_ERR_CAPACITY;   // positions 5 i .. 5 i + 4 are ints
  return guarded([&] {
    Scratch &sc = scratch();
    std::vector<float4> nb(m * 5);   // the fits load float4 map points; .w (the original index) is not read by them
    for (size_t k = 0; k < m * 5; ++k) nb[k] = make_float4(nbr_xyz[3 * k], nbr_xyz[3 * k + 1], nbr_xyz[3 * k + 2], 0.f);
    sc.up_tf(*T);
    sc.up(sc.a, nb.data(), m * 5); sc.up(sc.b, stack, m); sc.up(sc.sqd, fifth_sqd, m);
    sc.room(sc.valid, m); sc.room(sc.coef, m); sc.room(sc.score, m); sc.room(sc.abs_coef, m);
    launch_fit_five(form, mm, mp, fixed_pz, sc.tf.p, sc.b.p, int(m), sc.a.p, sc.sqd.p, sc.valid.p, sc.coef.p, sc.score.p, sc.abs_coef.p, sc.s);
    sc.down(valid, sc.valid.p, m); sc.down(coeff, sc.coef.p, m); sc.down(score, sc.score.p, m); sc.down(abs_coeff, sc.abs_coef.p, m);
    sc.sync();   // also keeps nb alive until its upload has read it
    return LIO_OK;
  });
}

int lio_odom_correspondences(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_lc,
                             const float *last_surf, size_t n_lsf, const lio_transform_f *T, float scan_period, int no_deskew,
                             int32_t *corner_idx, int32_t *surf_idx, float *sel_out) {
  if ((!sharp && n_sharp) || (!flat && n_flat) || (!last_corner && n_lc) || (!last_surf && n_lsf) || !T || !corner_idx || !surf_idx || !sel_out)
    return LIO_ERR_ARG;
  if (!(scan_period > 0) || !std::isfinite(scan_period)) return LIO_ERR_ARG;
  if (n_sharp + n_flat > size_t(INT_MAX) / 4 || n_lc > size_t(1) << 24 || n_lsf > size_t(1) << 24) return LIO_ERR_CAPACITY;   // odo_corr_body's scan-order keys
  return guarded([&] {
    OdometryDev od(scan_period, 1, 1, no_deskew != 0);   // stateless: a device object of its own, gone on return
    od.Correspondences(sharp, n_sharp, flat, n_flat, last_corner, n_lc, last_surf, n_lsf, toT(*T), corner_idx, surf_idx, sel_out);
    return LIO_OK;
  });
}

// ---- the Gauss-Newton hooks (include/lio_test_hooks.h)
static_assert(sizeof(lio_gn_state) == sizeof(OdomState) && offsetof(lio_gn_state, nsel) == offsetof(OdomState, nsel), "lio_gn_state is OdomState");
static bool finite_T(const lio_transform_f *T) {
  for (int k = 0; k < 4; ++k) if (!std::isfinite(T->q[k])) return false;
  for (int k = 0; k < 3; ++k) if (!std::isfinite(T->p[k])) return false;
  return true;
}

int lio_gn_rows_map(int form, const float *stack, size_t m, const uint8_t *valid, const float *coeff, const lio_transform_f *T, uint8_t *ok_out,
                    float *rows_out, int32_t *nb_out, double *partials_out) {
  if (form < 0 || form > 2 || ((!stack || !valid || !coeff || !ok_out || !rows_out) && m) || !T || !nb_out || !partials_out) return LIO_ERR_ARG;
  if (!finite_T(T)) return LIO_ERR_ARG;
  if (m > size_t(INT_MAX) / 8) return LIO_ERR_CAPACITY;
  return guarded([&] {
    Scratch &sc = scratch();
    const int M = int(m), nb = odom_rows_blocks(M);
    sc.room(sc.idx, (m + 3) / 4);   // ok_out, as bytes
    sc.room(sc.gn_rows, m * 7); sc.gn_partials.reserve(size_t(nb) * 28);
    const OdomState st = odom_state_at(toT(*T));
    sc.up(sc.gn_state, &st, 1);
    LIO_HIP(hipMemsetAsync(sc.gn_partials.p, 0, size_t(nb) * 28 * sizeof(double), sc.s));
    sc.up(sc.b, stack, m); sc.up(sc.valid, valid, m); sc.up(sc.coef, coeff, m);
    if (m) {
      // what production launches (csrc/mapping.hip, csrc/kf_batch.hip): the rows kernel over a keyframe table, here one record of M slots
      // in odom_rows_blocks(M) blocks
      const KfDesc kd{0, 0, M, 0, nb, 0, {0.f, 0.f, 0.f}};
      sc.up(sc.gn_kd, &kd, 1);
      launch_kf_rows(sc.gn_kd.p, sc.gn_state.p, 1, nb, sc.b.p, sc.valid.p, sc.coef.p, sc.gn_partials.p, form, sc.s);
      uint8_t *ok_dev = reinterpret_cast<uint8_t *>(sc.idx.p);
      launch_gn_rows_map(sc.b.p, M, sc.valid.p, sc.coef.p, sc.gn_state.p, form, ok_dev, sc.gn_rows.p, sc.s);
      sc.down(ok_out, ok_dev, m); sc.down(rows_out, sc.gn_rows.p, m * 7);
    }
    sc.down(partials_out, sc.gn_partials.p, size_t(nb) * 28);
    sc.sync();
    *nb_out = nb;
    return LIO_OK;
  });
}

// every stated correspondence lies in its cloud, and a second / third entry comes with a closest one (the search gives all -1 without it; the
// rows read the closest point whenever the others exist)
static bool gn_indices_ok(const int32_t *idx, size_t n, int per, size_t n_last) {
  for (size_t i = 0; i < n; ++i) {
    bool others = false;
    for (int k = 0; k < per; ++k) {
      const int32_t v = idx[i * per + k];
      if (v < -1 || (v >= 0 && size_t(v) >= n_last)) return false;
      if (k > 0 && v >= 0) others = true;
    }
    if (others && idx[i * per] < 0) return false;
  }
  return true;
}
int lio_gn_rows_odom(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_lc, const float *last_surf,
                     size_t n_lsf, const int32_t *corner_idx, const int32_t *surf_idx, const lio_transform_f *T, float scan_period, int no_deskew, int iter,
                     uint8_t *ok_out, float *rows_out, int32_t *nb_out, double *partials_out) {
  if ((!sharp && n_sharp) || (!flat && n_flat) || (!last_corner && n_lc) || (!last_surf && n_lsf) || (!corner_idx && n_sharp) || (!surf_idx && n_flat) ||
      ((!ok_out || !rows_out) && (n_sharp + n_flat)) || !T || !nb_out || !partials_out || iter < 0)
    return LIO_ERR_ARG;
  if (!(scan_period > 0) || !std::isfinite(scan_period) || !finite_T(T)) return LIO_ERR_ARG;
  if (n_sharp + n_flat > size_t(INT_MAX) / 8 || n_lc > size_t(INT_MAX) || n_lsf > size_t(INT_MAX)) return LIO_ERR_CAPACITY;
  if (!gn_indices_ok(corner_idx, n_sharp, 2, n_lc) || !gn_indices_ok(surf_idx, n_flat, 3, n_lsf)) return LIO_ERR_ARG;
  return guarded([&] {
    OdometryDev od(scan_period, 1, 1, no_deskew != 0);   // stateless: a device object of its own, gone on return
    od.Rows(sharp, n_sharp, flat, n_flat, last_corner, n_lc, last_surf, n_lsf, corner_idx, surf_idx, toT(*T), iter, ok_out, rows_out, nb_out, partials_out);
    return LIO_OK;
  });
}

int lio_gn_fold(const double *partials, int nblocks, int wide, double *sums_out) {
  if (nblocks < 0 || (!partials && nblocks) || !(wide == 0 || wide == 1) || !sums_out) return LIO_ERR_ARG;
  if (nblocks > INT_MAX / 32) return LIO_ERR_CAPACITY;   // reduce_partials28 indexes b * 28 + c in int
  return guarded([&] {
    Scratch &sc = scratch();
    sc.up(sc.gn_partials, partials, size_t(nblocks) * 28); sc.room(sc.gn_sums, 28);
    launch_gn_fold(sc.gn_partials.p, nblocks, wide, sc.gn_sums.p, sc.s);
    sc.down(sums_out, sc.gn_sums.p, 28);
    sc.sync();
    return LIO_OK;
  });
}

int lio_gn_step(int family, const double *sums, const lio_gn_state *state_in, int iter, int min_rows, int left_update, lio_gn_state *state_out) {
  if (!(family == 0 || family == 1) || !sums || !state_in || !state_out || iter < 0 || min_rows < 0) return LIO_ERR_ARG;
  if (family == 1 && (min_rows != 0 || left_update != 0)) return LIO_ERR_ARG;
  for (int k = 0; k < 7; ++k) if (!std::isfinite(state_in->T[k])) return LIO_ERR_ARG;
  return guarded([&] {
    Scratch &sc = scratch();
    sc.up(sc.gn_sums, sums, 28); sc.up(sc.gn_state, state_in, 1);
    if (family == 0) launch_gn_step(sc.gn_sums.p, sc.gn_state.p, iter, min_rows, left_update ? 1 : 0, sc.s);
    else launch_gn_odo_step(sc.gn_sums.p, sc.gn_state.p, iter, sc.s);
    sc.down(state_out, sc.gn_state.p, 1);
    sc.sync();
    return LIO_OK;
  });
}

int lio_gn_round(const float *map, size_t n_map, const float *stack, size_t m, const lio_transform_f *T, float mm, float mp, int lpq, int32_t *nb_out,
                 double *partials_out, lio_gn_state *state_out) {
  if ((!map && n_map) || (!stack && m) || !T || !nb_out || !partials_out || !state_out || !(lpq == 4 || lpq == 8)) return LIO_ERR_ARG;
  if (!finite_T(T) || !(mm > 0) || !std::isfinite(mm) || !(mp > 0) || !std::isfinite(mp)) return LIO_ERR_ARG;
  if (m > size_t(INT_MAX) / 8 || n_map > size_t(INT_MAX)) return LIO_ERR_CAPACITY;
  return guarded([&] {
    Scratch &sc = scratch();
    const int M = int(m), nb = M > 0 ? odom_round_blocks(M, lpq) : 0;
    sc.up(sc.a, map, n_map); sc.up(sc.b, stack, m);
    sc.room(sc.valid, m); sc.room(sc.coef, m); sc.room(sc.score, m); sc.room(sc.gn_partials, size_t(nb) * 28);
    const OdomState st = odom_state_at(toT(*T));
    sc.up(sc.gn_state, &st, 1);
    sc.grid_over_a(map, n_map, knn_cell_edge(mm));   // the grid of lio_calculate_features
    launch_odom_round(one_frame(sc.b.p, M, mm, mp), 0, 0, 0, sc.gn_state.p, sc.grid.sorted(), sc.grid.cells(), sc.grid.desc(), sc.valid.p, sc.coef.p, sc.score.p,
                      sc.gn_partials.p, sc.s, nullptr, HostSignal(), lpq);
    sc.down(partials_out, sc.gn_partials.p, size_t(nb) * 28); sc.down(state_out, sc.gn_state.p, 1);
    sc.sync();
    *nb_out = nb;
    return LIO_OK;
  });
}

int lio_calculate_features(const float *map, size_t n_map, const float *stack, size_t m, const lio_transform_f *T, float mm, float mp,
                           uint8_t *valid, float *coeff, float *score) {
  if ((!map && n_map) || (!stack && m) || !T || !valid || !coeff || !score || !(mm > 0)) return LIO_ERR_ARG;
  return guarded([&] {
    Scratch &sc = scratch();
    sc.up(sc.a, map, n_map); sc.up(sc.b, stack, m);
    sc.room(sc.valid, m); sc.room(sc.coef, m); sc.room(sc.score, m);
    sc.up_tf(*T);
    sc.grid_over_a(map, n_map, knn_cell_edge(mm));
    launch_features(one_frame(sc.b.p, int(m), mm, mp), sc.tf.p, sc.grid.sorted(), sc.grid.cells(), sc.grid.desc(), sc.valid.p, sc.coef.p, sc.score.p, nullptr, sc.s);
    sc.down(valid, sc.valid.p, m); sc.down(coeff, sc.coef.p, m); sc.down(score, sc.score.p, m);
    sc.sync();
    return LIO_OK;
  });
}

// ---------------------------------------------------------------- pre-integration (host)
lio_pim *lio_pim_create(const double acc0[3], const double gyr0[3], const double ba[3], const double bg[3], double acc_n, double gyr_n,
                        double acc_w, double gyr_w, double g_norm) {
  if (!acc0 || !gyr0 || !ba || !bg) return nullptr;
  PimNoise n; n.acc_n = acc_n; n.gyr_n = gyr_n; n.acc_w = acc_w; n.gyr_w = gyr_w; n.g_norm = g_norm;
  lio_pim *h = new (std::nothrow) lio_pim;
  if (h) h->p = std::make_shared<Preintegration>(v3(acc0), v3(gyr0), v3(ba), v3(bg), n);
  return h;
}
void lio_pim_destroy(lio_pim *h) { delete h; }
int lio_pim_push_back(lio_pim *h, double dt, const double acc[3], const double gyr[3]) {
  if (!h || !acc || !gyr) return LIO_ERR_ARG;
  h->p->push_back(dt, v3(acc), v3(gyr));
  return LIO_OK;
}
int lio_pim_repropagate(lio_pim *h, const double ba[3], const double bg[3]) {
  if (!h || !ba || !bg) return LIO_ERR_ARG;
  h->p->repropagate(v3(ba), v3(bg));
  return LIO_OK;
}
int lio_pim_get(const lio_pim *h, double *sum_dt, double *dp, double *dq, double *dv, double *jac, double *cov) {
  if (!h) return LIO_ERR_ARG;
  const Preintegration &p = *h->p;
  if (sum_dt) *sum_dt = p.sum_dt;
  if (dp) { dp[0] = p.dp.x; dp[1] = p.dp.y; dp[2] = p.dp.z; }
  if (dq) { dq[0] = p.dq.x; dq[1] = p.dq.y; dq[2] = p.dq.z; dq[3] = p.dq.w; }
  if (dv) { dv[0] = p.dv.x; dv[1] = p.dv.y; dv[2] = p.dv.z; }
  if (jac) std::memcpy(jac, p.jac, sizeof(p.jac));
  if (cov) std::memcpy(cov, p.cov, sizeof(p.cov));
  return LIO_OK;
}
int lio_pim_evaluate(const lio_pim *h, const double *pi, const double *sbi, const double *pj, const double *sbj, double *res) {
  if (!h || !pi || !sbi || !pj || !sbj || !res) return LIO_ERR_ARG;
  V3d Pi, Pj; Qd Qi, Qj;
  unpack_pose(pi, Pi, Qi); unpack_pose(pj, Pj, Qj);
  h->p->evaluate(Pi, Qi, v3(sbi), v3(sbi + 3), v3(sbi + 6), Pj, Qj, v3(sbj), v3(sbj + 3), v3(sbj + 6), res);
  return LIO_OK;
}

// ---------------------------------------------------------------- factors (host)
int lio_factor_imu(const lio_pim *h, const double *pi, const double *sbi, const double *pj, const double *sbj, double *res, double *j0,
                   double *j1, double *j2, double *j3) {
  if (!h || !pi || !sbi || !pj || !sbj || !res) return LIO_ERR_ARG;
  return imu_factor(*h->p, pi, sbi, pj, sbj, res, j0, j1, j2, j3) ? LIO_OK : LIO_ERR_STATE;
}
int lio_factor_pivot_point_plane(const double point[3], const double coeff[4], const double *pp, const double *pi, const double *pex,
                                 double *res, double *j0, double *j1, double *j2) {
  if (!point || !coeff || !pp || !pi || !pex || !res) return LIO_ERR_ARG;
  ppp_factor(v3(point), coeff, pp, pi, pex, res, j0, j1, j2);
  return LIO_OK;
}
int lio_factor_prior(const double pos0[3], const double rot0[4], const double *pose, double *res, double *j) {
  if (!pos0 || !rot0 || !pose || !res) return LIO_ERR_ARG;
  prior_factor(v3(pos0), Qd(rot0[3], rot0[0], rot0[1], rot0[2]), pose, res, j);
  return LIO_OK;
}
int lio_pose_plus(const double *pose, const double *d, double *out) {
  if (!pose || !d || !out) return LIO_ERR_ARG;
  pose_plus(pose, d, out);
  return LIO_OK;
}

// ---------------------------------------------------------------- estimator
void lio_est_default_config(lio_est_config *c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->window_size = 15; c->opt_window_size = 5; c->corner_filter_size = 0.2f; c->surf_filter_size = 0.4f;
  c->min_match_sq_dis = 1.0f; c->min_plane_dis = 0.2f;
  c->transform_lb.q[3] = 1.f; c->transform_lb.p[2] = -0.1f;
  c->opt_extrinsic = 0; c->imu_factor = 1; c->point_distance_factor = 0; c->prior_factor = 0; c->marginalization_factor = 1;
  c->enable_deskew = 1; c->cutoff_deskew = 0; c->keep_features = 0;
  c->acc_n = 0.1; c->gyr_n = 0.01; c->acc_w = 0.0002; c->gyr_w = 2.0e-5; c->g_norm = 9.805;
  c->max_num_iterations = 10; c->max_solver_time = 0.10; c->extrinsic_stage = 2; c->init_window_factor = 3;
}
static EstConfig to_est_config(const lio_est_config &c) {
  EstConfig e;
  e.W = c.window_size; e.Wo = c.opt_window_size;
  e.corner_filter_size = c.corner_filter_size; e.surf_filter_size = c.surf_filter_size;
  e.min_match_sq_dis = c.min_match_sq_dis; e.min_plane_dis = c.min_plane_dis;
  e.transform_lb = toT(c.transform_lb);
  e.opt_extrinsic = c.opt_extrinsic; e.imu_factor = c.imu_factor; e.point_distance_factor = c.point_distance_factor;
  e.prior_factor = c.prior_factor; e.marginalization_factor = c.marginalization_factor;
  e.enable_deskew = c.enable_deskew; e.cutoff_deskew = c.cutoff_deskew; e.keep_features = c.keep_features;
  e.pim.acc_n = c.acc_n; e.pim.gyr_n = c.gyr_n; e.pim.acc_w = c.acc_w; e.pim.gyr_w = c.gyr_w; e.pim.g_norm = c.g_norm;
  e.max_num_iterations = c.max_num_iterations; e.max_solver_time = c.max_solver_time; e.extrinsic_stage = c.extrinsic_stage;
  e.init_window_factor = c.init_window_factor > 0 ? c.init_window_factor : 1;
  e.device_solve = c.device_solve != 0; e.inline_marg = c.inline_marg != 0;
  e.stream_sync = c.stream_sync != 0;
  e.resident_moments = (c.resident_moments >= 1 && c.resident_moments <= 3) ? c.resident_moments : 0;
  return e;
}
lio_est *lio_est_create(const lio_est_config *c) {
  if (!c || c->window_size < 1 || c->opt_window_size < 1 || c->opt_window_size > c->window_size || c->window_size + 1 > LIO_MAX_FRAMES) return nullptr;
  return make_handle<lio_est>([&](lio_est &h) {
    h.cfg = to_est_config(*c);
    // Estimator.cc:189-194: the estimator's filter sizes and thresholds configure its PointMapping base (created on first use)
    lio_map_default_config(&h.map_cfg);
    h.map_cfg.corner_filter_size = c->corner_filter_size; h.map_cfg.surf_filter_size = c->surf_filter_size;
    h.map_cfg.min_match_sq_dis = c->min_match_sq_dis; h.map_cfg.min_plane_dis = c->min_plane_dis;
    h.e.reset(new Estimator(h.cfg));
    if (h.cfg.device_solve) {   // a batch of one window: the device loop and the device marginalization serve this handle's solves
      EstimatorBatch *b = new EstimatorBatch({h.e.get()});
      h.solo.reset(b);
      h.e->solve_hook_ = [b](lio_solve_report *rep) { b->Solve(rep); return b->window_ok(0); };
    }
  });
}
static void dissolve_batch(lio_est_batch *B);
void lio_est_destroy(lio_est *h) {
  if (!h) return;
  if (h->owner) {   // destroyed before its batch: the batch goes first (it holds pointers into every member)
    std::fprintf(stderr, "[lio_hip] lio_est_destroy: the handle is a member of a batch; the batch is dissolved\n");
    dissolve_batch(h->owner);
  }
  delete h;
}

int lio_est_process_imu(lio_est *h, double dt, const double acc[3], const double gyr[3], double stamp) {
  if (!h || !acc || !gyr) return LIO_ERR_ARG;
  h->e->ProcessImu(dt, v3(acc), v3(gyr), stamp);
  return LIO_OK;
}
int lio_est_process_imu_batch(lio_est *h, size_t n, const double *dt, const double *acc, const double *gyr, const double *stamp) {
  if (!h || (n && (!dt || !acc || !gyr || !stamp))) return LIO_ERR_ARG;
  for (size_t k = 0; k < n; ++k) h->e->ProcessImu(dt[k], v3(acc + 3 * k), v3(gyr + 3 * k), stamp[k]);
  return LIO_OK;
}
int lio_est_process_laser_odom(lio_est *h, const lio_transform_f *T, const float *surf, size_t ns, const float *corner, size_t nc, double stamp,
                               lio_solve_report *rep) {
  if (!h || !T || (!surf && ns) || (!corner && nc)) return LIO_ERR_ARG;
  return guarded([&] { return h->e->ProcessLaserOdom(toT(*T), CloudSrc::host(surf, ns), CloudSrc::host(corner, nc), stamp, rep) ? LIO_OK : LIO_ERR_STATE; });
}
// int thread ids, one point per lane in workgroups of 256: the last workgroup's tail lanes must not pass INT_MAX
static constexpr size_t kMaxCloudPoints = size_t(INT_MAX) - 255;
// the estimator's PointMapping base, created on first use (Estimator.cc:189-194: configured from the estimator's own sizes)
static MappingDev &est_map(lio_est *h) {
  if (!h->map.m) { h->map.m.reset(new MappingDev(h->map_cfg)); h->map.borrowed = true; }
  h->e->map_ = h->map.m.get();
  return *h->map.m;
}
// ProcessCompactData (Estimator.cc:776-856).  The post-initialisation map-database refresh (:703-708), which feeds the published
// surround map, runs inside ProcessLaserOdom under lio_est_set_map_refresh (include/lio_ext.h); it is off by default.
int lio_est_process_compact(lio_est *h, const float *data, size_t n, double stamp, lio_transform_f *T_out, lio_solve_report *rep) {
  if (!h || !data) return LIO_ERR_ARG;
  lio_transform_f Tsum;
  size_t nc = 0, ns = 0, nf = 0;
  int rc = lio_compact_decode(data, n, &Tsum, &nc, &ns, &nf);
  if (rc != LIO_OK) return rc;
  return guarded([&] {
    Estimator &e = *h->e;
    if (e.inited_ && !e.cfg_.imu_factor) return LIO_ERR_STATE;  // LOAM-only operation after init is not part of this path
    est_map(h);
    if (e.full_cloud() && nf > kMaxCloudPoints) return LIO_ERR_CAPACITY;
    Rigidf T_to_init;
    const bool ok = e.ProcessCompact(toT(Tsum), data + 4 * 3, nc, data + 4 * (3 + nc), ns, data + 4 * (3 + nc + ns), nf, stamp, &T_to_init, rep);
    if (T_out) fromT(T_to_init, T_out);
    return ok ? LIO_OK : LIO_ERR_STATE;
  });
}
// ---------------------------------------------------------------- include/lio_est_wide.h: seven optimised frames on the device loop
int lio_est_set_device_solve_limit(lio_est *h, int max_opt_window) {
  if (!h || max_opt_window < LIO_DEVICE_SOLVE_LIMIT_DEFAULT || max_opt_window > LIO_DEVICE_SOLVE_LIMIT_MAX) return LIO_ERR_ARG;
  h->e->device_solve_limit_ = max_opt_window;   // (read by BatchPackProblem at the next solve; a solve is one blocking call)
  return LIO_OK;
}
int lio_est_get_device_solve_limit(const lio_est *h) { return h ? h->e->device_solve_limit_ : LIO_ERR_ARG; }
// ---------------------------------------------------------------- include/lio_ext.h: the map refresh and the surround map
lio_map *lio_est_map(lio_est *h) {
  if (!h) return nullptr;
  const int rc = guarded([&] { est_map(h); return LIO_OK; });
  return rc == LIO_OK ? &h->map : nullptr;
}
int lio_est_set_map_refresh(lio_est *h, int on) {
  if (!h || (on != 0 && on != 1)) return LIO_ERR_ARG;
  return guarded([&] { h->e->SetMapRefresh(on != 0, &est_map(h)); return LIO_OK; });
}
int lio_est_refresh_map(lio_est *h) {
  if (!h) return LIO_ERR_ARG;
  if (!h->e->inited_) return LIO_ERR_STATE;
  return guarded([&] { est_map(h); return h->e->RefreshMap(); });
}
size_t lio_map_get_surround(lio_map *h, float leaf, float *xyzi_or_null) {
  if (!h || !h->m || !(leaf > 0)) return 0;
  return guarded_count([&] { return h->m->GetSurround(leaf, xyzi_or_null); });
}
int lio_est_get_last_map_refresh(const lio_est *h, int *applied, lio_transform_f *T, int cube_center[3], uint32_t *valid_idx, int *n_valid,
                                 size_t *n_corner, float *corner_xyzi_or_null, size_t *n_surf, float *surf_xyzi_or_null) {
  if (!h) return LIO_ERR_ARG;
  const MapRefreshRecord &r = h->e->last_refresh();
  if (!r.have) return LIO_ERR_STATE;
  return guarded([&] {
    Estimator &e = *h->e;
    const OptSlot &sl = r.slot;
    const DeviceCloud *surf = sl.surf_frame == OptSlot::kNoFrame ? nullptr : e.OptSurfCloud(sl.surf_frame);
    if (sl.surf_frame != OptSlot::kNoFrame && !surf) return int(LIO_ERR_STATE);   // the frame has left the window since
    if (applied) *applied = r.applied;
    if (T) fromT(sl.transform, T);
    if (cube_center) for (int d = 0; d < 3; ++d) cube_center[d] = sl.cen[d];
    if (valid_idx) for (size_t k = 0; k < sl.valid_idx.size(); ++k) valid_idx[k] = sl.valid_idx[k];
    if (n_valid) *n_valid = int(sl.valid_idx.size());
    const size_t nc = e.CopyCloudToHost(sl.corner.get(), corner_xyzi_or_null);
    const size_t ns = e.CopyCloudToHost(surf, surf_xyzi_or_null);
    if (n_corner) *n_corner = nc;
    if (n_surf) *n_surf = ns;
    return int(LIO_OK);
  });
}
// ---------------------------------------------------------------- include/lio_full_cloud.h: the full-resolution sweep
// PointOdometry.cc:261-292 at :725-730
int lio_odom_full_to_end(lio_odom *h, const float *xyzi, size_t n, float *xyzi_out) {
  if (!h || (n && (!xyzi || !xyzi_out))) return LIO_ERR_ARG;
  if (n > kMaxCloudPoints) return LIO_ERR_CAPACITY;
  return guarded([&] { h->o->FullToEnd(xyzi, n, xyzi_out); return LIO_OK; });
}
// PointMapping.cc:212-224
int lio_map_set_full_cloud(lio_map *h, const float *xyzi, size_t n) {
  if (!h || !h->m || (!xyzi && n)) return LIO_ERR_ARG;
  if (n > kMaxCloudPoints) return LIO_ERR_CAPACITY;
  return guarded([&] { h->m->SetFullCloud(xyzi, n); return LIO_OK; });
}
// PointMapping.cc:1244-1251
size_t lio_map_get_full_cloud(const lio_map *h, float *xyzi_or_null) {
  if (!h || !h->m) return 0;
  return guarded_count([&] { return h->m->GetFullCloud(xyzi_or_null); });
}
// Estimator.cc:482, :2355-2420
int lio_est_set_full_cloud(lio_est *h, int on) {
  if (!h || (on != 0 && on != 1)) return LIO_ERR_ARG;
  return guarded([&] { h->e->SetFullCloud(on != 0, &est_map(h)); return LIO_OK; });
}
// Estimator.cc:2372-2375
size_t lio_est_get_full_stack(const lio_est *h, int frame, float *xyzi_or_null, int *state_or_null) {
  if (!h) return 0;
  const FullEntry *e = h->e->FullEntryOf(frame);
  if (!e) return 0;
  size_t n = 0;
  if (guarded([&] { n = h->e->CopyCloudToHost(&e->cloud, xyzi_or_null); return LIO_OK; }) != LIO_OK) return 0;
  if (state_or_null) *state_or_null = e->state;
  return n;
}
// Estimator.cc:2284-2286, :2293-2295, :2311 and PointMapping.cc:303-314
int lio_est_get_registered_full(const lio_est *h, int frame, lio_transform_f *T_out_or_null, size_t *n_out, float *xyzi_or_null) {
  if (!h) return LIO_ERR_ARG;
  return guarded([&] {
    Rigidf T;
    size_t n = 0;
    if (!h->e->RegisteredFull(frame, &T, &n, xyzi_or_null)) return int(LIO_ERR_STATE);
    if (T_out_or_null) fromT(T, T_out_or_null);
    if (n_out) *n_out = n;
    return int(LIO_OK);
  });
}
int lio_est_get_full_transform_es(const lio_est *h, int frame, lio_transform_f *T_es) {
  if (!h || !T_es) return LIO_ERR_ARG;
  const FullEntry *e = h->e->FullEntryOf(frame);
  if (!e) return LIO_ERR_STATE;
  fromT(e->tes, T_es);
  return LIO_OK;
}
// Estimator.cc:62-103
int lio_deskew_to_end(const float *xyzi, size_t n, const lio_transform_f *T_es, float time_factor, int keep_intensity, float *xyzi_out) {
  if (!T_es || (keep_intensity != 0 && keep_intensity != 1) || (n && (!xyzi || !xyzi_out))) return LIO_ERR_ARG;
  if (n > kMaxCloudPoints) return LIO_ERR_CAPACITY;
  if (!n) return LIO_OK;
  return guarded([&] {
    Scratch &sc = scratch();
    sc.up(sc.a, xyzi, n);
    launch_deskew_to_end(sc.a.p, int(n), T_es->q, T_es->p, time_factor, sc.s, keep_intensity != 0);
    sc.down(xyzi_out, sc.a.p, n);
    sc.sync();
    return LIO_OK;
  });
}

int lio_est_get_stage(const lio_est *h, int *stage, int *cir_buf_count, int *extrinsic_stage, int *last_event, double *R_WI, double *g_vec) {
  if (!h) return LIO_ERR_ARG;
  const Estimator &e = *h->e;
  if (stage) *stage = e.inited_ ? 1 : 0;
  if (cir_buf_count) *cir_buf_count = e.cir_buf_count_;
  if (extrinsic_stage) *extrinsic_stage = e.extrinsic_stage_;
  if (last_event) *last_event = e.last_event_;
  if (R_WI) for (int k = 0; k < 9; ++k) R_WI[k] = e.R_WI_.m[k];
  if (g_vec) { g_vec[0] = e.g_vec_.x; g_vec[1] = e.g_vec_.y; g_vec[2] = e.g_vec_.z; }
  return LIO_OK;
}
int lio_est_push_frame(lio_est *h, const lio_transform_f *T, const float *surf, size_t ns, const float *corner, size_t nc, double stamp) {
  if (!h || !T || (!surf && ns) || (!corner && nc)) return LIO_ERR_ARG;
  if (!h->e->inited_) return LIO_ERR_STATE;
  return guarded([&] { return h->e->PushFrame(toT(*T), CloudSrc::host(surf, ns), CloudSrc::host(corner, nc), stamp) ? LIO_OK : LIO_ERR_STATE; });
}
int lio_est_solve_optimization(lio_est *h, lio_solve_report *rep) {
  if (!h) return LIO_ERR_ARG;
  if (!h->e->inited_) return LIO_ERR_STATE;
  return guarded([&] { return h->e->SolveOptimization(rep) ? LIO_OK : LIO_ERR_STATE; });
}
int lio_est_slide_window(lio_est *h) {
  if (!h) return LIO_ERR_ARG;
  if (!h->e->inited_) return LIO_ERR_STATE;
  return guarded([&] { h->e->SlideWindow(); return LIO_OK; });
}
int lio_est_sync(lio_est *h) {
  if (!h) return LIO_ERR_ARG;
  return guarded([&] { h->e->JoinMarg(); return LIO_OK; });
}
int lio_est_set_window(lio_est *h, int n, const double *Ps, const double *Rs, const double *Vs, const double *Bas, const double *Bgs,
                       const double g[3]) {
  if (!h || !Ps || !Rs || !Vs || !Bas || !Bgs || !g || n != h->e->W_ + 1) return LIO_ERR_ARG;
  h->e->SetWindow(Ps, Rs, Vs, Bas, Bgs, g);
  return LIO_OK;
}
int lio_est_get_window(const lio_est *h, int n, double *Ps, double *Rs, double *Vs, double *Bas, double *Bgs, lio_transform_f *Tlb) {
  if (!h || n != h->e->W_ + 1) return LIO_ERR_ARG;
  const Estimator &e = *h->e;
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) {
      if (Ps) Ps[3 * i + k] = e.Ps_[i][k];
      if (Vs) Vs[3 * i + k] = e.Vs_[i][k];
      if (Bas) Bas[3 * i + k] = e.Bas_[i][k];
      if (Bgs) Bgs[3 * i + k] = e.Bgs_[i][k];
    }
    if (Rs) for (int k = 0; k < 9; ++k) Rs[9 * i + k] = e.Rs_[i].m[k];
  }
  if (Tlb) fromT(e.transform_lb_, Tlb);
  return LIO_OK;
}
int lio_est_set_surf_stack(lio_est *h, int frame, const float *xyzi, size_t n) {
  if (!h || frame < 0 || frame > h->e->W_ || (!xyzi && n)) return LIO_ERR_ARG;
  return guarded([&] { h->e->SetSurfStack(frame, xyzi, n); return LIO_OK; });
}
size_t lio_est_get_surf_stack(const lio_est *h, int frame, float *out) {
  if (!h || frame < 0 || frame > h->e->W_) return 0;
  return guarded_count([&] { return h->e->GetSurfStack(frame, out); });
}
int lio_est_set_preintegration(lio_est *h, int frame, const double acc0[3], const double gyr0[3], const double ba[3], const double bg[3],
                               const double *dt, const double *acc, const double *gyr, size_t ns) {
  if (!h || frame < 0 || frame > h->e->W_ || !acc0 || !gyr0 || !ba || !bg || (ns && (!dt || !acc || !gyr))) return LIO_ERR_ARG;
  auto p = std::make_shared<Preintegration>(v3(acc0), v3(gyr0), v3(ba), v3(bg), h->cfg.pim);
  for (size_t k = 0; k < ns; ++k) p->push_back(dt[k], v3(acc + 3 * k), v3(gyr + 3 * k));
  h->e->SetPreintegration(frame, p);
  return LIO_OK;
}
int lio_est_begin_frame(lio_est *h, const double acc[3], const double gyr[3]) {
  if (!h || !acc || !gyr) return LIO_ERR_ARG;
  h->e->BeginFrame(v3(acc), v3(gyr));
  return LIO_OK;
}
int lio_est_build_local_map(lio_est *h) {
  if (!h) return LIO_ERR_ARG;
  if (!h->e->inited_) return LIO_ERR_STATE;
  return guarded([&] { h->e->BuildLocalMap(nullptr); return LIO_OK; });
}
size_t lio_est_get_local_map(const lio_est *h, float *out) {
  if (!h) return 0;
  return guarded_count([&] { return h->e->GetLocalMap(out); });
}
size_t lio_est_get_features(const lio_est *h, int frame, double *pt, double *co, double *sc) {
  if (!h) return 0;
  return guarded_count([&] { return h->e->GetFeatures(frame, pt, co, sc); });
}
int lio_est_eval_lidar_moments(lio_est *h, int n_passes, const double *Rt, double *out, int *path_out) {
  if (!h || n_passes < 1 || !Rt || !out) return LIO_ERR_ARG;
  if (!h->e->inited_) return LIO_ERR_STATE;
  return guarded([&] {
    const int path = h->e->EvalLidarMoments(n_passes, Rt, out);
    if (path < 0) return LIO_ERR_STATE;
    if (path_out) *path_out = path;
    return LIO_OK;
  });
}
int lio_est_force_moments_per_lane(lio_est *h, int per_lane) {
  if (!h || !(per_lane == 0 || per_lane == 1 || per_lane == 2 || per_lane == 4 || per_lane == 8)) return LIO_ERR_ARG;
  h->e->resident_.ForcePerLane(per_lane);
  return LIO_OK;
}
int lio_est_set_max_num_iterations(lio_est *h, int n) {
  if (!h || n < 0) return LIO_ERR_ARG;
  h->e->cfg_.max_num_iterations = n;
  return LIO_OK;
}
int lio_est_get_laser_odom_transform(const lio_est *h, lio_transform_f *out) {
  if (!h || !out) return LIO_ERR_ARG;
  fromT(h->e->laser_odom_transform_, out);
  return LIO_OK;
}
int lio_est_get_prior(const lio_est *h, double *JtJ, double *Jtr, double *x0, int *x0_len) {
  return est_get_prior(h, [](MargPrior &p) { return p.JtJ.a.data(); }, [](MargPrior &p) { return p.Jtr0.data(); }, JtJ, Jtr, x0, x0_len);
}
int lio_est_get_prior_factor(const lio_est *h, double *lin_jac, double *lin_res, double *x0, int *x0_len) {
  return est_get_prior(h, [](MargPrior &p) { return p.lin_jac.a.data(); }, [](MargPrior &p) { return p.lin_res.data(); }, lin_jac, lin_res, x0, x0_len);
}
int lio_est_set_prior_factor(lio_est *h, int n, const double *lin_jac, const double *lin_res, const double *x0, int x0_len) {
  if (!h || !lin_jac || !lin_res || !x0 || n <= 0) return LIO_ERR_ARG;
  return guarded([&] {
    h->e->JoinMarg();
    const auto &old = h->e->last_marg_;
    if (!old || old->n != n || prior_x0(*old, nullptr) != x0_len) return LIO_ERR_STATE;
    auto pr = std::make_shared<MargPrior>(*old);   // the old object may still be referenced by a snapshot
    std::memcpy(pr->lin_jac.a.data(), lin_jac, sizeof(double) * size_t(n) * n);
    std::memcpy(pr->lin_res.data(), lin_res, sizeof(double) * n);
    prior_x0(*pr, nullptr, x0);
    pr->finalize();
    h->e->last_marg_ = pr;
    return LIO_OK;
  });
}
int lio_est_set_extrinsic(lio_est *h, const lio_transform_f *T) {
  if (!h || !T) return LIO_ERR_ARG;
  return guarded([&] {
    h->e->JoinMarg();   // a marginalization in flight captured its own copy of the states; join so that nothing reads half a change
    h->e->transform_lb_ = toT(*T);
    return LIO_OK;
  });
}
int lio_dense_spd_solve(const double *A, const double *b, int n, double *x) {
  if (!A || !b || !x || n < 1 || n > 128) return LIO_ERR_ARG;
  return guarded([&] {
    const int ok = ldlt_solve_device(A, b, n, x, scratch().s);
    return ok == 1 ? LIO_OK : (ok == -2 ? LIO_ERR_ARG : LIO_ERR_STATE);
  });
}
int lio_marginalize_schur(const double *A, const double *b, int m, int n, double *lin_jac, double *lin_res, double *evals) {
  if (!A || !b || !lin_jac || !lin_res || m < 1 || m > MARG_MAX_M - 1 || n < 1 || n > MARG_MAX_N) return LIO_ERR_ARG;
  return guarded([&] {
    int dev = 0;
    LIO_HIP(hipGetDevice(&dev));
    MargSchurDev md(dev);
    return md.Run(A, b, m, n, 1e-8, lin_jac, lin_res, evals, nullptr) ? LIO_OK : LIO_ERR_ARG;
  });
}
int lio_est_snapshot(lio_est *h) {
  if (!h) return LIO_ERR_ARG;
  return guarded([&] { h->e->Snapshot(); return LIO_OK; });
}
int lio_est_restore(lio_est *h) {
  if (!h) return LIO_ERR_ARG;
  return guarded([&] { return h->e->Restore() ? LIO_OK : LIO_ERR_STATE; });
}

int lio_est_copy_snapshot(lio_est *dst, lio_est *src) {
  if (!dst || !src) return LIO_ERR_ARG;
  return guarded([&] { return dst->e->CopySnapshotOf(*src->e) ? LIO_OK : LIO_ERR_STATE; });
}

int lio_est_solve_restored(lio_est *h, int steps, lio_solve_report *rep) {
  if (!h || steps < 0) return LIO_ERR_ARG;
  for (int k = 0; k < steps; ++k) {
    int rc = lio_est_restore(h);
    if (rc != LIO_OK) return rc;
    rc = lio_est_solve_optimization(h, rep);
    if (rc != LIO_OK) return rc;
  }
  return LIO_OK;
}

// ---------------------------------------------------------------- batched windows
static bool batch_live(const lio_est_batch *h) { return h->parts && h->parts->built(); }
lio_est_batch *lio_est_batch_create(lio_est *const *windows, int n) {
  if (!windows || n < 1 || n > 65535) return nullptr;
  for (int i = 0; i < n; ++i)
    if (!windows[i] || windows[i]->adopted || windows[i]->solo) return nullptr;
  if (!distinct(windows, size_t(n))) return nullptr;
  lio_est_batch *h = make_handle<lio_est_batch>([&](lio_est_batch &b) {
    std::vector<Estimator *> es;
    for (int i = 0; i < n; ++i) { b.members.push_back(windows[i]); es.push_back(windows[i]->e.get()); }
    b.parts.reset(new BatchParts(es));
  });
  for (int i = 0; h && i < n; ++i) { windows[i]->adopted = true; windows[i]->owner = h; }
  return h;
}
static void dissolve_batch(lio_est_batch *B) {
  (void)guarded([&] { B->parts.reset(); return LIO_OK; });
  for (lio_est *m : B->members) { m->adopted = false; m->owner = nullptr; }
  B->members.clear();
}
void lio_est_batch_destroy(lio_est_batch *h) {
  if (!h) return;
  dissolve_batch(h);
  delete h;
}
int lio_est_batch_size(const lio_est_batch *h) { return (h && batch_live(h)) ? h->parts->size() : 0; }
int lio_est_batch_solve(lio_est_batch *h, lio_solve_report *reps) {
  if (!h) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  for (lio_est *m : h->members) if (!m->e->inited_) return LIO_ERR_STATE;
  return guarded([&] { h->parts->Solve(reps); return LIO_OK; });
}
int lio_est_batch_set_option(lio_est_batch *h, const char *name, int value) {
  if (!h || !name) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  return guarded([&] { return h->parts->SetOption(name, value) ? LIO_OK : LIO_ERR_ARG; });
}
int lio_est_batch_solve_restored(lio_est_batch *h, int steps, lio_solve_report *reps) {
  if (!h || steps < 0) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  return guarded([&] { return h->parts->SolveRestored(steps, reps) ? LIO_OK : LIO_ERR_STATE; });
}
// ---- include/lio_est_push_batch.h: every refusal comes before a window is touched
static int push_batch_check(const lio_est_batch *h, const lio_est_frame *frames) {
  if (!h || !frames) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  const int n = h->parts->size();
  for (int w = 0; w < n; ++w)
    if ((!frames[w].surf_xyzi && frames[w].n_surf) || (!frames[w].corner_xyzi && frames[w].n_corner)) return LIO_ERR_ARG;
  size_t total = 0;   // the chain indexes the clouds of a part, each rounded up to 256 points, by int
  for (int w = 0; w < n; ++w) {
    if (frames[w].n_surf > kMaxCloudPoints || frames[w].n_corner > kMaxCloudPoints) return LIO_ERR_CAPACITY;
    total += frames[w].n_surf + frames[w].n_corner + 512;
    if (total > (size_t(1) << 30)) return LIO_ERR_CAPACITY;
  }
  return h->parts->PushReady() ? LIO_OK : LIO_ERR_STATE;
}
int lio_est_batch_push_frames(lio_est_batch *h, const lio_est_frame *frames) {
  const int rc = push_batch_check(h, frames);
  if (rc != LIO_OK) return rc;
  return guarded([&] { h->parts->PushFrames(frames); return LIO_OK; });
}
int lio_est_batch_slide_windows(lio_est_batch *h) {
  if (!h) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  for (lio_est *m : h->members) if (!m->e->inited_) return LIO_ERR_STATE;
  return guarded([&] { h->parts->SlideWindows(); return LIO_OK; });
}
int lio_est_batch_process_laser_odom(lio_est_batch *h, const lio_est_frame *frames, lio_solve_report *reps) {
  const int rc = push_batch_check(h, frames);
  if (rc != LIO_OK) return rc;
  return guarded([&] { return h->parts->ProcessLaserOdom(frames, reps) ? LIO_OK : LIO_ERR_STATE; });
}
int lio_est_batch_push_stats(const lio_est_batch *h, int *out8) {
  if (!h || !out8) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  h->parts->PushStats(out8);
  return LIO_OK;
}
// ---- include/lio_est_from_odom.h: the windows' sweeps taken from the odometry handles on the device.  Every refusal comes before a window, a
// map or the device is touched, in the header's order; the lease on the processors is held until the parts, which read their clouds, have
// returned synchronised.  f(the sources, one per window) runs the call.
static int est_from_odom(lio_est_batch *h, lio_odom *const *odom, lio_pp *const *pp, const double *stamps, bool need_T, const void *T, bool composite,
                         const char *who, const std::function<int(const OdomSweep *)> &f) {
  if (!h || !odom || !stamps || (need_T && !T)) return LIO_ERR_ARG;
  const int n = batch_live(h) ? h->parts->size() : 0;
  for (int w = 0; w < n; ++w)
    if (!odom[w]) return LIO_ERR_ARG;
  if (!batch_live(h) || !h->parts->PushReady()) return LIO_ERR_STATE;
  for (int w = 0; w < n; ++w) {
    if (composite && !h->members[size_t(w)]->e->cfg_.imu_factor) return LIO_ERR_STATE;   // (as lio_est_process_compact)
    if (!odom[w]->o->processed()) return LIO_ERR_STATE;                                  // no sweep to hand over
  }
  return guarded([&] {
    const PpLease lease(pp, size_t(n), who, true, true);
    std::vector<OdomSweep> src(static_cast<size_t>(n));
    size_t total = 0;   // push_batch_check's limits, the full cloud included
    for (int w = 0; w < n; ++w) {
      const OdomSweep &S = src[size_t(w)] = odom_sweep(odom[w], lease, size_t(w));
      if (S.corner.n > kMaxCloudPoints || S.surf.n > kMaxCloudPoints || S.full.n > kMaxCloudPoints) return int(LIO_ERR_CAPACITY);
      total += S.corner.n + S.surf.n + S.full.n + 768;
      if (total > (size_t(1) << 30)) return int(LIO_ERR_CAPACITY);
    }
    if (composite) for (lio_est *m : h->members) est_map(m);   // (behind the last refusal, as lio_est_process_compact creates it)
    return int(f(src.data()));
  });
}
int lio_est_batch_push_frames_from_odom(lio_est_batch *h, lio_odom *const *odom, lio_pp *const *pp, const lio_transform_f *T_in, const double *stamps) {
  return est_from_odom(h, odom, pp, stamps, true, T_in, false, "lio_est_batch_push_frames_from_odom", [&](const OdomSweep *src) {
    h->parts->PushFramesFrom(src, T_in, stamps);
    return LIO_OK;
  });
}
int lio_est_batch_process_compact_from_odom(lio_est_batch *h, lio_odom *const *odom, lio_pp *const *pp, const double *stamps, lio_transform_f *T_out,
                                            lio_solve_report *reps) {
  return est_from_odom(h, odom, pp, stamps, false, nullptr, true, "lio_est_batch_process_compact_from_odom", [&](const OdomSweep *src) {
    return h->parts->ProcessCompactFrom(src, stamps, T_out, reps) ? LIO_OK : LIO_ERR_STATE;
  });
}
int lio_est_batch_from_odom_stats(const lio_est_batch *h, int *out8) {
  if (!h || !out8) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  h->parts->FromOdomStats(out8);
  return LIO_OK;
}
int lio_est_batch_sync(lio_est_batch *h) {
  if (!h) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  return guarded([&] { h->parts->Sync(); return LIO_OK; });
}
int lio_seg_sort_pairs(const unsigned *keys, const unsigned *vals, size_t n_total, const int *seg_off, const int *seg_n, int nseg, int bits, int passes, unsigned *keys_out,
                       unsigned *vals_out) {
  return guarded([&] { return seg_sort_host_test(keys, vals, n_total, seg_off, seg_n, nseg, bits, passes, keys_out, vals_out) ? LIO_OK : LIO_ERR_ARG; });
}
int lio_est_batch_stage_digest(lio_est_batch *h, int stage, unsigned long long *out) {
  if (!h || !out || stage < 0 || stage > 9) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  return guarded([&] { h->parts->StageDigest(stage, out); return LIO_OK; });
}
int lio_est_batch_get_moments(lio_est_batch *h, int window, double *out, double *Rt) {
  if (!h || !out || !Rt || window < 0) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  if (window >= h->parts->size()) return LIO_ERR_ARG;
  return guarded([&] { return h->parts->GetMoments(window, out, Rt) ? LIO_OK : LIO_ERR_STATE; });
}
int lio_est_batch_get_linearization(lio_est_batch *h, int window, int32_t *ints, double *problem, double *state, double *aux) {
  if (!h || !ints || !problem || !state || !aux || window < 0) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  if (window >= h->parts->size()) return LIO_ERR_ARG;
  return guarded([&] { return h->parts->GetLinearization(window, ints, problem, state, aux) ? LIO_OK : LIO_ERR_STATE; });
}
int lio_est_batch_get_clock(const lio_est_batch *h, double *out) {
  if (!h || !out) return LIO_ERR_ARG;
  if (!batch_live(h)) return LIO_ERR_STATE;
  BatchClock c;
  const int rc = guarded([&] { c = h->parts->clock(); return LIO_OK; });
  if (rc != LIO_OK) return rc;
  for (int k = 0; k < 6; ++k) out[10 + k] = c.dev[k];
  out[0] = c.describe; out[1] = c.map; out[2] = c.grid_features; out[3] = c.pack; out[4] = c.solve; out[5] = c.finish; out[6] = c.fallback; out[7] = c.total;
  out[8] = c.n_device; out[9] = c.rounds;
  out[16] = c.dev_marg_wait;
  for (int k = 0; k < 3; ++k) { out[17 + k] = c.kernel_ms[k]; out[20 + k] = double(c.kernel_launches[k]); }
  out[23] = 0.0;   // reserved
  return LIO_OK;
}

int lio_est_set_factor_sharding(lio_est *h, int rank, int world, lio_allreduce_fn fn, void *user) {
  if (!h || world < 1 || rank < 0 || rank >= world) return LIO_ERR_ARG;
  h->e->shard_rank_ = rank; h->e->shard_world_ = world; h->e->allreduce_ = fn; h->e->allreduce_user_ = user;
  h->e->rccl_comm_ = nullptr;   // the callback form replaces an RCCL communicator set earlier (which the caller may destroy now)
  return LIO_OK;
}
int lio_est_set_factor_sharding_rccl(lio_est *h, lio_rccl *comm) {
  if (!h) return LIO_ERR_ARG;
  if (!comm) { h->e->rccl_comm_ = nullptr; h->e->shard_rank_ = 0; h->e->shard_world_ = 1; return LIO_OK; }
  h->e->rccl_comm_ = rccl_raw_comm(comm);
  h->e->shard_rank_ = lio_rccl_rank(comm); h->e->shard_world_ = lio_rccl_world(comm);
  h->e->allreduce_ = nullptr; h->e->allreduce_user_ = nullptr;
  return LIO_OK;
}
int lio_bench_voxel_grid(const float *xyzi, size_t n, float leaf, int reps, double *avg_ms, size_t *n_out) {
  if (!xyzi || n == 0 || !(leaf > 0) || reps < 1 || !avg_ms) return LIO_ERR_ARG;
  return guarded([&] {
    hipStream_t s = nullptr;
    LIO_HIP(hipStreamCreate(&s));
    DBuf<float4> in, out;
    in.reserve(n);
    LIO_HIP(hipMemcpyAsync(in.p, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, s));
    VoxelGridDev vox;
    size_t m = 0;
    for (int w = 0; w < 2; ++w) m = vox.run(in.p, n, leaf, out, s);   // warm-up: buffers, sort scratch
    hipEvent_t e0, e1;
    LIO_HIP(hipEventCreate(&e0)); LIO_HIP(hipEventCreate(&e1));
    LIO_HIP(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) m = vox.run(in.p, n, leaf, out, s);
    LIO_HIP(hipEventRecord(e1, s));
    LIO_HIP(hipStreamSynchronize(s));
    float ms = 0;
    LIO_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = double(ms) / reps;
    if (n_out) *n_out = m;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    return LIO_OK;
  });
}
int lio_est_bench_batched_moments(lio_est *h, int n_windows, int reps, double *avg_ms, double *bytes) {
  if (!h || n_windows < 1 || reps < 1) return LIO_ERR_ARG;
  return guarded([&] { return h->e->BenchBatchedMoments(n_windows, reps, avg_ms, bytes) ? LIO_OK : LIO_ERR_STATE; });
}
int lio_est_enable_kernel_timing(lio_est *h, int on) {
  if (!h) return LIO_ERR_ARG;
  h->e->resident_.LaunchTiming(on == -1);   // -1: only the resident moments kernel's launches are bracketed (it stays in use)
  h->e->timers_.on = on > 0;
  h->e->timers_.sample = on > 1 ? on : 1;
  h->e->timers_.reset();
  return LIO_OK;
}
int lio_est_get_kernel_timing(lio_est *h, const char *name, double *total_ms, double *bytes) {
  if (total_ms) *total_ms = 0;
  if (bytes) *bytes = 0;
  if (!h || !name) return 0;
  static const char *names[KT_COUNT] = {"features", "odom_features", "odom_rows", "odom_update", "moments", "voxel", "knn_grid", "concat"};
  if (std::strcmp(name, "moments_resident") == 0) {
    // the resident moments kernel cannot be bracketed by HIP events per pass (one launch serves a whole solve): its passes are
    // timed on the device's wall clock, doorbell copy seen -> sums posted, slowest frame; counted since the handle was created
    int passes = 0;
    const double us = h->e->resident_.BusyUs(&passes, bytes);
    if (total_ms) *total_ms = us * 1e-3;
    return passes;
  }
  if (std::strcmp(name, "moments_resident_launch") == 0) {   // dispatch-to-exit spans recorded under lio_est_enable_kernel_timing(-1)
    int n = 0;
    guarded([&] { n = h->e->resident_.LaunchStats(total_ms, h->e->stream()); return LIO_OK; });
    return n;
  }
  for (int k = 0; k < KT_COUNT; ++k)
    if (std::strcmp(name, names[k]) == 0) {
      const KernelTimers::Acc &a = h->e->timers_.acc[k];
      if (total_ms) *total_ms = a.ms;
      if (bytes) *bytes = a.bytes;
      return a.n;
    }
  return 0;
}

}  // extern "C"
