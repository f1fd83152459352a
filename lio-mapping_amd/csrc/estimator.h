// estimator.h — the product's mirror of lio::Estimator's post-initialisation surface
// (include/imu_processor/Estimator.h:110-299): ProcessImu, ProcessLaserOdom (INITED branch),
// BuildLocalMap, SolveOptimization, SlideWindow.  Clouds live in HBM for the life of the window;
// the host keeps only the (W+1) x {P,R,V,Ba,Bg} states, the pre-integrations and the prior.
#pragma once
#include <climits>
#include <condition_variable>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/lio_c.h"
#include "cloud_kernels.h"
#include "cloud_src.h"
#include "host_init.h"
#include "host_solver.h"
#include "batch_kernels.h"
#include "resident_moments.h"
#include "solve_step.h"

namespace lio {

typedef Rigid<float> Rigidf;
typedef Rigid<double> Rigidd;

struct EstConfig {
  int W = 15, Wo = 5;
  float corner_filter_size = 0.2f, surf_filter_size = 0.4f, min_match_sq_dis = 1.0f, min_plane_dis = 0.2f;
  Rigidf transform_lb;
  bool opt_extrinsic = false, imu_factor = true, point_distance_factor = false, prior_factor = false, marginalization_factor = true,
       enable_deskew = true, cutoff_deskew = false, keep_features = false;
  PimNoise pim;
  int max_num_iterations = 10;
  double max_solver_time = 0.10;
  int extrinsic_stage = 2;
  int init_window_factor = 3;
  // execution switches (lio_est_config's trailing block)
  bool device_solve = false, inline_marg = false, stream_sync = false;
  int resident_moments = 0;
};

struct DeviceCloud {
  DBuf<float4> buf;
  size_t n = 0;
  uint64_t id = 0;  // content id: equal ids in the same slot => identical content (restore() skips the copy)
  DeviceCloud() = default;
  // a moved-from cloud is EMPTY (n = 0, id = 0), not a null buffer with a stale count
  DeviceCloud(DeviceCloud &&o) noexcept : buf(std::move(o.buf)), n(o.n), id(o.id) { o.n = 0; o.id = 0; }
  DeviceCloud &operator=(DeviceCloud &&o) noexcept {
    if (this != &o) { buf = std::move(o.buf); n = o.n; id = o.id; o.n = 0; o.id = 0; }
    return *this;
  }
};

struct StampedPose { double time; Rigidf T; };

class MappingDev;

// One slot of the optimisation-window buffers (Estimator.cc:177-183; pushed at :467-485): opt_point_coeff_mask_, opt_cube_centers_,
// opt_valid_idx_, opt_transforms_, opt_surf_stack_, opt_corner_stack_.  The reference's stacks are shared pointers: a slot's surf
// cloud IS a window frame's cloud, later in-place edits included (the pivot fusion :1434, SlideWindow :2615), so the slot names the
// frame (by its push number) and the cloud is looked up in the window when it is read.  Corner clouds are never edited: shared, immutable.
struct OptSlot {
  bool mask = false;
  int cen[3] = {0, 0, 0};
  std::vector<uint32_t> valid_idx;
  Rigidf transform;
  static constexpr long kNoFrame = LONG_MIN;
  long surf_frame = kNoFrame;             // push number of the frame whose surf stack the slot holds (negative: a frame SetWindow injected)
  std::shared_ptr<DeviceCloud> corner;    // null: no corner cloud (a frame from before the refresh was enabled)
};
// the arguments of the last RefreshMap (lio_est_get_last_map_refresh)
struct MapRefreshRecord {
  bool have = false;
  int applied = 0;
  OptSlot slot;
};

// One entry of full_stack_ (Estimator.cc:482; include/lio_full_cloud.h): the full-resolution sweep of a window frame, the transform_es_ its
// frame was pushed with (identity under cutoff_deskew and with both de-skew switches off) and where it stands.  The states are
// LIO_FULL_* of the header.
enum { FULL_NONE = 0, FULL_MAP_FRAME = 1, FULL_SENSOR_RAW = 2, FULL_SENSOR_END = 3 };
struct FullEntry {
  DeviceCloud cloud;
  int state = FULL_NONE;
  Rigidf tes;
};

// HIP-event kernel timing on the estimator's stream (lio_est_enable_kernel_timing)
enum { KT_FEATURES = 0, KT_ODOM_FEATURES, KT_ODOM_ROWS, KT_ODOM_UPDATE, KT_MOMENTS, KT_VOXEL, KT_KNN_GRID, KT_CONCAT, KT_COUNT };
struct KernelTimers {
  bool on = false;
  int sample = 1;            // record every sample-th launch of each kind (events between kernels cost ~10 % when all are timed)
  int seen[KT_COUNT] = {0};
  struct Rec { hipEvent_t a, b; int id; double bytes; };
  struct Acc { int n = 0; double ms = 0, bytes = 0; };
  std::vector<Rec> pending;
  std::vector<hipEvent_t> pool;
  Acc acc[KT_COUNT];
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e; LIO_HIP(hipEventCreate(&e)); return e;
  }
  int begin(int id, double bytes, hipStream_t s) {
    if (!on) return -1;
    if ((seen[id]++ % sample) != 0) return -1;
    Rec r{get(), get(), id, bytes};
    LIO_HIP(hipEventRecord(r.a, s));
    pending.push_back(r);
    return int(pending.size()) - 1;
  }
  void end(int h, hipStream_t s) { if (h >= 0) LIO_HIP(hipEventRecord(pending[h].b, s)); }
  void resolve() {  // call after the stream has been synchronised
    for (Rec &r : pending) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { acc[r.id].n++; acc[r.id].ms += ms; acc[r.id].bytes += r.bytes; }
      pool.push_back(r.a); pool.push_back(r.b);
    }
    pending.clear();
  }
  void reset() { for (Acc &a : acc) a = Acc(); for (int &v : seen) v = 0; }
  ~KernelTimers() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); for (Rec &r : pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); } }
};

// Marginalization is host-only work (one factor evaluation from the solve's final lidar moments, a Schur complement, two
// symmetric eigendecompositions: 0.12 ms) whose result — the prior — is first read by the NEXT solve, after that solve
// has built its local map and features (0.45 ms, mostly device time).  A persistent worker thread computes it meanwhile;
// every reader of the prior joins first, so the sequence of values is exactly the synchronous one.
class MargWorker {
 public:
  using Task = std::function<std::shared_ptr<MargPrior>()>;
  ~MargWorker() {
    { std::lock_guard<std::mutex> lk(mu_); quit_ = true; }
    cv_.notify_all();
    if (th_.joinable()) th_.join();
  }
  void submit(Task t) {
    std::unique_lock<std::mutex> lk(mu_);
    if (!th_.joinable()) th_ = std::thread([this] { run(); });
    cv_.wait(lk, [this] { return state_ == IDLE || state_ == DONE; });  // an unjoined (discarded) task finishes first
    task_ = std::move(t); state_ = PENDING; err_ = nullptr; result_.reset();
    lk.unlock();
    cv_.notify_all();
  }
  bool busy() { std::lock_guard<std::mutex> lk(mu_); return state_ != IDLE; }
  // blocks until the submitted task is done; returns false when nothing was submitted since the last join
  bool join(std::shared_ptr<MargPrior> &out) {
    std::unique_lock<std::mutex> lk(mu_);
    if (state_ == IDLE) return false;
    cv_.wait(lk, [this] { return state_ == DONE; });
    state_ = IDLE;
    if (err_) { std::exception_ptr e = err_; err_ = nullptr; std::rethrow_exception(e); }
    out = std::move(result_);
    return true;
  }

 private:
  enum { IDLE, PENDING, RUNNING, DONE };
  void run() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [this] { return quit_ || state_ == PENDING; });
      if (quit_) return;
      Task t = std::move(task_);
      state_ = RUNNING;
      lk.unlock();
      std::shared_ptr<MargPrior> r;
      std::exception_ptr e;
      try { r = t(); } catch (...) { e = std::current_exception(); }
      lk.lock();
      result_ = std::move(r); err_ = e; state_ = DONE;
      cv_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::thread th_;
  Task task_;
  std::shared_ptr<MargPrior> result_;
  std::exception_ptr err_;
  int state_ = IDLE;
  bool quit_ = false;
};

class EstimatorBatch;

// What PushFrameBegin leaves for the device work of a push and for PushFrameEnd.  The single call (PushFrame) and the batched one
// (EstimatorBatch::PushFrames) do the device work in between; the bookkeeping on both sides of it is one piece of code.
struct PushPlan {
  int n_before = 0;
  size_t n_surf = 0, n_corner = 0;
  bool filter = false;                         // de-skewed and filtered (Estimator.cc:678-693); else the clouds go in as they come (:474-480)
  bool deskew = false;                         // ... with TransformToEnd by (q, p) in front of the filter (enable_deskew without cutoff_deskew)
  float q[4] = {0.f, 0.f, 0.f, 1.f}, p[3] = {0.f, 0.f, 0.f};
  Rigidf full_tes;                             // transform_es_ as SolveOptimization meets it (:2355): identity unless this push computes it
  DeviceCloud fresh;                           // the recycled buffer of the slot being (re)written, room for n_surf points; n is the device work's to set
  std::shared_ptr<DeviceCloud> corner_cloud;   // map refresh only: this frame's corner cloud, room for n_corner points; n likewise
};

// One window as BOTH solve paths read it (Estimator::PlanWindow): the single-window path fills ConcatArgs / SolveSetup / FeatArgs from
// it, the batched path BatchWin.  The slot layout it goes with is the estimator's slot_off_ / nslots_ / total_slots_.
struct WindowPlan {
  int pivot, keep_mult;            // keep_mult: slots per point of the newest frame (10 rounds' features kept, else 1)
  ConcatSeg seg[LIO_MAX_FRAMES];   // local map (Estimator.cc:1480-1507): the pivot's cloud as it is, frames pivot+1 .. W-1 transformed, intensity = frame index
  int nseg, n_local;
  float tf[LIO_MAX_FRAMES][8];     // local transform of frame i >= first_frame (qx qy qz qw px py pz 0)
  int max_slots;                   // largest nslots_ of frames pivot+1 .. W (the newest frame's is an upper bound until the rounds are done)
};

class Estimator {
 public:
  explicit Estimator(const EstConfig &cfg);
  ~Estimator();

  void ProcessImu(double dt, const V3d &acc, const V3d &gyr, double stamp);
  // surf, corner: host or device (cloud_src.h; the scan-to-map stage's down-sampled stacks before initialisation are the device's).  corner
  // is read only while the map refresh is on (PushFrame)
  bool ProcessLaserOdom(const Rigidf &transform_in, CloudSrc surf, CloudSrc corner, double stamp, lio_solve_report *rep);
  // ProcessCompactData (Estimator.cc:776-856) on the decoded blocks of a /compact_data message, map_ being the PointMapping base: before
  // initialisation the scan-to-map step and its stacks, afterwards the pose predicted from the IMU-propagated body motion, go into
  // ProcessLaserOdom.  *T_to_init: the pose that went in.  false: ProcessLaserOdom refused.
  bool ProcessCompact(const Rigidf &transform_sum, const float *corner, size_t nc, const float *surf, size_t ns, const float *full, size_t nf, double stamp,
                      Rigidf *T_to_init, lio_solve_report *rep);
  // the initialised branch of ProcessCompact in front of ProcessLaserOdom (:780-805): the prediction of the map's transform_tobe_mapped_, its
  // transform_sum_; returns the pose that goes in.  ProcessCompact and the batch's device-fed composite (est_batch.h) both call it.
  Rigidf CompactPredict(const Rigidf &transform_sum);
  bool PushFrame(const Rigidf &transform_in, CloudSrc surf, CloudSrc corner, double stamp);
  // PushFrame in two parts with the device work in between (the single call's: PushFrame; a batch's: est_push.h).  PushRefused: the de-skew
  // precondition fails — checked before the window is touched.  PushFrameBegin: the LaserFrame and pre-integration pushes, the refresh ring's
  // slot, buffer recycling, transform_es, the destinations reserved.  PushFrameEnd: PushCloud, PushFull, the counts.
  bool PushRefused() const { return inited_ && (cfg_.enable_deskew || cfg_.cutoff_deskew) && !cfg_.cutoff_deskew && imu_stamped_.empty(); }
  void PushFrameBegin(const Rigidf &transform_in, size_t n_surf, size_t n_corner, double stamp, PushPlan &pl);
  void PushFrameEnd(PushPlan &pl);
  // SlideWindow likewise: SlideBegin fills the concat of Estimator.cc:2602-2615 and reserves the scratch cloud (false: no local map yet, no
  // device work), SlideEnd swaps the stacks and pushes the state
  bool SlideBegin(ConcatArgs &ca);
  void SlideEnd(bool concat, const ConcatArgs &ca);
  float4 *slide_dst() const { return scratch_cloud_.buf.p; }
  // ---- the map-database refresh (Estimator.cc:703-708), off unless SetMapRefresh(true, map): PushFrame then keeps the optimisation-window
  // buffers (and the corner clouds they need), ProcessLaserOdom refreshes between SolveOptimization and SlideWindow
  void SetMapRefresh(bool on, MappingDev *map);
  bool map_refresh() const { return map_refresh_; }
  // after a solve, before the slide.  1: the map was updated; 0: slot 0 is masked or the ring is not full (:626)
  int RefreshMap();
  const MapRefreshRecord &last_refresh() const { return last_refresh_; }
  // the surf cloud an optimisation-window slot holds, where it is now (nullptr: the frame has left the window)
  const DeviceCloud *OptSurfCloud(long surf_frame) const;
  size_t CopyCloudToHost(const DeviceCloud *c, float *out);
  MappingDev *map_ = nullptr;   // the PointMapping base (owned by the C handle); read by PushFrame and RefreshMap only while the refresh or the full cloud is on
  // ---- the full-resolution sweep (include/lio_full_cloud.h), off unless SetFullCloud(true, map): PushFrame then copies the map's full
  // cloud into a ring of W + 1 that moves with the window, every completed solve corrects the newest entry once
  void SetFullCloud(bool on, MappingDev *map);
  bool full_cloud() const { return full_cloud_; }
  void CorrectNewestFull();                       // Estimator.cc:2355-2420 (update_laser_imu): TransformToEnd(full_stack_.last(), transform_es_, 10, true)
  const FullEntry *FullEntryOf(int frame) const;  // nullptr: the frame has no entry
  Rigidf OptPose(int i) const;                    // the lidar pose of window frame i (Estimator.cc:2284-2286, :2293-2295): in double, cast to float
  // a FULL_SENSOR_END entry mapped by its frame's lidar pose, out of place; false for any other state
  bool RegisteredFull(int frame, Rigidf *T, size_t *n, float *out);
  bool RunInitialization();
  void SetStatesFromLaser();
  // Estimator.cc:1648-2438.  With a hook installed (lio_est_config.device_solve: a batch of one window, est_batch.h) the whole
  // solve runs there; SolveOptimizationHost is the default path (device kernels + the trust-region loop on the host).
  bool SolveOptimization(lio_solve_report *rep) { return solve_hook_ ? solve_hook_(rep) : SolveOptimizationHost(rep); }
  bool SolveOptimizationHost(lio_solve_report *rep);
  std::function<bool(lio_solve_report *)> solve_hook_;
  void SlideWindow();
  void BuildLocalMap(lio_solve_report *rep);

  // ---- the per-window host halves of a BATCHED solve (est_batch.h drives them; the device work between them is one launch per
  // stage over all windows of the batch)
  bool BatchEligible() const;
  // host half of BuildLocalMap (Estimator.cc:1361-1646): segments of the local map, frames, local transforms, slot layout.
  // Offsets are the window's own (from 0); the batch shifts them to its arrays.  Returns WindowPlan::max_slots.
  int BatchDescribe(BatchWin &bw);
  // the problem of Estimator.cc:1660-1921 as the device loop reads it; *prior = the marginalization prior the problem uses.
  // false: this window's problem does not fit the device loop.
  bool BatchPackProblem(int bpf, DevProblem &pb, DevState &st, std::shared_ptr<MargPrior> *prior);
  // the largest optimisation window BatchPackProblem hands to the device loop (include/lio_est_wide.h: 6, or 7 = n_pad 128).  A choice of
  // the handle, not part of its state: Snapshot / Restore / CopySnapshotOf leave it alone.
  int device_solve_limit_ = 6;
  // after the device loop: DoubleToVector, the report, convergence_flag_.  true: the window marginalises now — mg is filled
  // (linearisation point, layout) and *shell is the new prior without its matrices (they are computed on the device).
  bool BatchFinish(const DevState &st, const std::shared_ptr<MargPrior> &prior_used, lio_solve_report &R, DevMarg &mg, std::shared_ptr<MargPrior> *shell);
  void ApplyOdomState(const OdomState &st);   // CalculateLaserOdom's outcome as the rounds left it (Estimator.cc:1242-1359)
  // frames pivot+1 .. W as the moments kernels read them (this rank's share of the slots when sharded); R, t are the caller's.
  // Returns the largest frame's slot count.
  int FillMomentFrames(MomentFrame *fr, int slot_base) const;

  // test hooks
  void SetWindow(const double *Ps, const double *Rs, const double *Vs, const double *Bas, const double *Bgs, const double g[3]);
  void SetSurfStack(int frame, const float *xyzi, size_t n);
  size_t GetSurfStack(int frame, float *out);
  void SetPreintegration(int frame, std::shared_ptr<Preintegration> p) { pre_integrations_[frame] = std::move(p); frames_dirty_ = true; }
  void BeginFrame(const V3d &acc, const V3d &gyr);
  size_t GetLocalMap(float *out);
  size_t GetFeatures(int frame, double *pt, double *co, double *sc);
  // lio_est_eval_lidar_moments: the lidar moments of frames pivot+1 .. pivot+Wo at caller-given T_{pivot<-i} (Rt: n_passes x Wo x 12,
  // R row-major then t), every pass inside ONE solve scope through the path the estimator is configured for; out: n_passes x Wo x 258
  // (S 16 x 16 row-major, cost, count).  A sharded estimator returns its own share (no all-reduce).  Returns the path of the last pass:
  // 0 MFMA launch pair, 2 resident kernel.
  int EvalLidarMoments(int n_passes, const double *Rt, double *out);
  void Snapshot();
  bool Restore();
  // this handle's snapshot <- a copy of src's (same configuration; clouds copied into buffers of this handle): B windows of the
  // same data at distinct addresses for the batched measurements, without replaying the sequence B times
  bool CopySnapshotOf(Estimator &src);
  // B copies of the current window's lidar factors through ONE moments launch (distinct memory per copy); returns the average
  // launch-pair duration in ms and the algorithmic bytes per launch.  false when no features have been built yet.
  bool BenchBatchedMoments(int n_windows, int reps, double *avg_ms, double *bytes);

  EstConfig cfg_;
  int W_, Wo_;
  std::vector<V3d> Ps_, Vs_, Bas_, Bgs_;
  std::vector<M3d> Rs_;
  V3d g_vec_, acc_last_, gyr_last_;
  Rigidf transform_lb_, laser_odom_transform_;
  bool inited_ = false, first_imu_ = false, init_local_map_ = false, convergence_flag_ = false;
  int cir_buf_count_ = 0;
  // initialisation stage (Estimator.cc:430-618, 858-958)
  std::vector<LaserFrame> all_laser_transforms_;
  int n_state_ = 0;    // CircularBuffer size of Ps_/Rs_/Vs_/Bas_/Bgs_
  int n_frames_ = 0;   // CircularBuffer size of pre_integrations_/all_laser_transforms_/the stacks
  int laser_odom_recv_count_ = 0, extrinsic_stage_ = 2;
  double initial_time_ = -1;
  M3d R_WI_;
  enum { EV_SKIPPED = 0, EV_FILLING = 1, EV_INIT_FAILED = 2, EV_INITIALISED = 3, EV_SOLVED = 4 };
  int last_event_ = EV_SKIPPED;
  std::shared_ptr<MargPrior> last_marg_;   // read through JoinMarg() only: a marginalization may still be running
  MargWorker marg_worker_;
  bool async_marg_ = true;                  // lio_est_config.inline_marg = 1: computed inside SolveOptimization
  unsigned marg_epoch_ = 0, marg_task_epoch_ = 0;   // Restore() bumps the epoch: a result computed for a discarded state is dropped
  // materialize: a prior that a batched solve left on the device (MargPrior::on_device) is brought to the host as well — every
  // reader of its matrices on the host needs that; the batch itself, which feeds the next solve from the device copy, does not
  void JoinMarg(bool materialize = true) {
    std::shared_ptr<MargPrior> r;
    const bool discard = marg_task_epoch_ != marg_epoch_;
    try {
      if (marg_worker_.join(r) && !discard) last_marg_ = std::move(r);
    } catch (...) {
      if (!discard) throw;  // a failure of a task whose result is dropped anyway (state restored meanwhile) is not the caller's problem
    }
    if (materialize && last_marg_) last_marg_->materialize();
  }
  std::vector<std::shared_ptr<Preintegration>> pre_integrations_;
  std::shared_ptr<Preintegration> tmp_pre_integration_;
  int laser_odom_iters_ = 0, laser_odom_kz_ = 0;
  double dbg_eval_ms_ = 0, dbg_sync_ms_ = 0; int dbg_eval_n_ = 0;  // LIO_DEBUG_TIMING: time inside LidarEval (launch + D2H + sync)
  KernelTimers timers_;
  // factor sharding across ranks (lio_est_set_factor_sharding)
  int shard_rank_ = 0, shard_world_ = 1;
  lio_allreduce_fn allreduce_ = nullptr;
  void *allreduce_user_ = nullptr;
  void *rccl_comm_ = nullptr;               // ncclComm_t (lio_est_set_factor_sharding_rccl): the all-reduce runs on stream_, in HBM
  bool Sharded() const { return shard_world_ > 1 && (allreduce_ || rccl_comm_); }
  // begun lazily by the first LidarLaunchMoments of a solve scope, stopped when the scope closes.  Public for the C entry points, which
  // use ForcePerLane, LaunchTiming, LaunchStats and BusyUs only; the protocol calls (Open .. End) are the estimator's
  ResidentMoments resident_;
  hipStream_t stream() const { return stream_; }

 private:
  friend class EstimatorBatch;   // the adoption handshake only: device_id_, AdoptStream / ReleaseAdoptedStream, feat_batch_ / feat_batch_w_
  struct ResidentScope { Estimator *e; ~ResidentScope() { e->resident_.End(e->stream_); } };   // closes a solve scope on every exit path
  void Init(), Close() noexcept;
  struct HostState;  // snapshot payload
  Rigidd LidarPose(int i, const Rigidd &lb) const;
  Rigidf RelTransform(int i, const Rigidd &T_pivot, const Rigidd &lb) const;
  bool KeepFeatures() const { return cfg_.keep_features && cfg_.imu_factor; }
  WindowPlan PlanWindow(int first_frame);   // also writes the slot layout
  void AssembleSystem(WindowParams &P, WindowSystem &sys) const;   // the problem of Estimator.cc:1660-1921 without the lidar callbacks
  void VectorToParams(WindowParams &P) const;
  void ParamsToVector(const WindowParams &P);
  void FillMomentArgs(MomentArgs &ma, int &max_slots) const;
  void LidarEval(const WindowParams &P, std::vector<FrameMoments> &m);
  void LidarLaunch(const WindowParams &P);             // asynchronous part: frame transforms + moments kernels
  void LidarLaunchMoments(const MomentArgs &ma, bool reduce = true);   // ... from a filled MomentArgs (reduce = false: a shard's own share)
  void LidarWait(std::vector<FrameMoments> &m, bool reduce = true);    // stream sync (+ all-reduce when sharded and `reduce`) + unpack
  bool LidarWaitFrame(int i, FrameMoments &fm);       // per-frame form (resident kernel only; false otherwise)
  void PushCloud(DeviceCloud &&c, size_t n, int n_before);
  void PushState(int from);

  hipStream_t stream_ = nullptr, stream2_ = nullptr;
  bool owns_stream_ = true;   // false once a batch has adopted the handle: its work is enqueued on the batch's stream
  void AdoptStream(hipStream_t s);
  void ReleaseAdoptedStream();   // the batch is gone: the handle works on a stream of its own again
  void FusePivotOnce();       // A.15: frames 0 .. pivot fused into the pivot's stack, the first time a local map is built
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
  std::vector<DeviceCloud> stacks_;
  std::vector<size_t> size_surf_stack_;
  std::vector<StampedPose> imu_stamped_;
  DeviceCloud local_, local_filtered_, scratch_cloud_, upload_;
  VoxelGridDev vox_;
  KnnGrid grid_;
  // feature slots
  DBuf<uint8_t> f_valid_;
  DBuf<float4> f_coef_;
  DBuf<float> f_score_;
  std::vector<int> slot_off_, nslots_;
  size_t total_slots_ = 0;
  // the batch whose arrays hold this window's feature slots (its last Solve ran the window on the device) and the window's index in it;
  // null once the single-window path builds features again (BuildLocalMap) or the batch is gone
  EstimatorBatch *feat_batch_ = nullptr;
  int feat_batch_w_ = -1;
  DBuf<float> d_transforms_;
  DBuf<OdomState> d_odom_;
  DBuf<double> d_odom_partials_, d_moment_partials_, d_moment_out_;
  HostBuf<double> h_moment_out_;    // pinned, coherent
  HostBuf<OdomState> h_odom_;       // pinned, coherent landing zone of the laser-odom state peeks
  // Completion words (dev.h: HostSignal) in coherent pinned memory: [0, 96) one per block of k_moment_reduce, [128] the
  // newest-frame round.  The host spins on them instead of hipStreamSynchronize (lio_est_config.stream_sync restores the synchronize calls).
  HostBuf<unsigned> h_signal_;
  unsigned signal_seq_[2] = {0, 0};
  bool host_signal_ = true;
  int device_id_ = 0;
  HostSignal moment_signal_{};
  // Restore() re-copies the per-frame containers (pre-integrations, laser transforms, stamped poses, the running pre-integration)
  // only if something touched them since they last equalled the snapshot's: a solve does not, and at hundreds of windows per
  // batch step their copies were the host's largest share of a restore + solve step
  bool frames_dirty_ = true;
  std::unique_ptr<HostState> snap_;
  std::vector<DeviceCloud> snap_stacks_;
  // ---- map refresh state (all empty while the refresh is off)
  bool map_refresh_ = false;
  std::vector<OptSlot> opt_ring_;               // CircularBuffer of Wo + 1 slots, oldest first
  long frame_seq_ = 0;                          // frames pushed so far: window slot i holds frame frame_seq_ - 1 - (n_frames_ - 1 - i)
  std::shared_ptr<DeviceCloud> corner_last_;    // corner_stack_.last()
  std::vector<std::shared_ptr<DeviceCloud>> corner_pool_;   // every corner cloud made; one nobody else holds is reused
  std::shared_ptr<DeviceCloud> AcquireCornerCloud();
  // W == Wo with de-skew on: slot 0's frame has just left the window when it is read (the reference's shared pointer keeps it alive)
  DeviceCloud opt_evicted_, snap_opt_evicted_;
  long opt_evicted_frame_ = -1;
  DeviceCloud upload_corner_;
  VoxelGridDev vox_corner_;
  MapRefreshRecord last_refresh_;
  Rigidf OptPose0() const { return OptPose(W_ - Wo_); }   // Estimator.cc:2282-2286
  // ---- full-cloud state (empty while the switch is off)
  bool full_cloud_ = false;
  std::vector<FullEntry> full_ring_;            // CircularBuffer of W + 1 entries, oldest first; the newest belongs to the window's newest frame
  DBuf<float4> full_out_;                       // RegisteredFull's output before it goes to the host
  void PushFull(const Rigidf &tes);
  void DropFullRing();
};

}  // namespace lio
