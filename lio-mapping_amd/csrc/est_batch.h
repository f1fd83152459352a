// est_batch.h — Estimator::SolveOptimization (Estimator.cc:1648-2438) for B windows at once: SURVEY.md 8(d)(ii)'s batched form.
//
// A batch adopts B estimator handles (independent windows: different vehicles, different logs, or the shards of an offline
// re-optimisation).  One call solves all of them, every stage ONE launch over all windows:
//
//   concat + voxel keys | segmented sort | tile heads | centroids     BuildLocalMap        Estimator.cc:1480-1519
//   cell keys | segmented sort | cell-sorted points + run starts      KdTreeFLANN build    :1544-1545
//   features of the frames behind the pivot                           CalculateFeatures    :970-1097
//   <= 10 x (search + fit + rows | fold + 6x6 step)                   CalculateLaserOdom   :1242-1359
//   <= max_iterations + 1 x (moments + IMU / prior / lidar-map aux row | trust-region step, one workgroup per window)
//                                                                     ceres::Solve         :1909-1990
//   aux row at the marginalization point | Schur complement + eigensolves on fp64 MFMA, one workgroup per window
//                                                                     Marginalize          MarginalizationFactor.cc:185-311
//
// The host touches a window three times per solve (descriptors, the K-NN grid's dimensions from the filter's bounds, the write-back
// of the state) and waits for the device three times per BATCH.  The marginalization's result — the next solve's prior — stays on
// the device; a host-side reader (lio_est_get_prior, a snapshot, the single-window solver) fetches it on demand.
// Per-window arithmetic does not depend on the batch: a window gives the same bits alone (B = 1, which is what
// lio_est_config.device_solve selects for a single handle) and inside any batch.  Windows whose problem the device loop does not
// take (not initialised yet, the convergence_flag_ logic changing the problem's shape, factor sharding, seven optimised frames
// on a handle that has not asked for them: Estimator::device_solve_limit_) are solved by the
// single-window path inside the same call.
//
// What the C ABI calls a batch (lio_est_batch) is a BatchParts, below: one EstimatorBatch, or two solved side by side.  The partition
// (the split rule, re-partitioning, the windows' addressing across the parts, the merged clock) lives there and nowhere else.
#pragma once
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/lio_est_push_batch.h"
#include "batch_kernels.h"
#include "est_push.h"
#include "estimator.h"
#include "mapping.h"
#include "marg_kernels.h"

namespace lio {

struct BatchClock {   // host wall clock of the last Solve(), ms
  double describe = 0, map = 0, grid_features = 0, pack = 0, solve = 0, finish = 0, fallback = 0, total = 0;
  int n_device = 0, n_host = 0, rounds = 0, iterations = 0;
  // device time of the last Solve()'s stages (HIP events on the batch's stream), ms: filter chain (concat, keys, sort, heads,
  // centroids), K-NN grids, features of the older frames, newest-frame rounds, trust-region loop, marginalization
  double dev[6] = {0, 0, 0, 0, 0, 0};
  // with the option time_kernels: summed duration and count of the last Solve()'s launches of k_bw_aux, k_bw_moments, k_bw_solve_step
  double kernel_ms[3] = {0, 0, 0};
  int kernel_launches[3] = {0, 0, 0};
  double dev_marg_wait = 0;   // of dev[3]: the stream's wait for the PREVIOUS solve's marginalization (it sits in front of the problems' upload)
};

class EstimatorBatch {
 public:
  explicit EstimatorBatch(const std::vector<Estimator *> &members);
  ~EstimatorBatch();
  EstimatorBatch(const EstimatorBatch &) = delete;
  EstimatorBatch &operator=(const EstimatorBatch &) = delete;
  int size() const { return int(m_.size()); }
  // SolveOptimization of every member; reps: size() reports, or null.  Returns the number of windows that were solved.
  int Solve(lio_solve_report *reps);
  // PushFrame of every member (include/lio_est_push_batch.h; est_push.h: the chain), frames: size() entries.  The caller has checked that no
  // member refuses its frame (Estimator::PushRefused) and that every member is initialised.  Returns synchronised with the uploads.
  void PushFrames(const lio_est_frame *frames);
  // SlideWindow of every member: one launch, no wait
  void SlideWindows();
  // ProcessLaserOdom of every (initialised) member: push, Solve, RefreshMap where it is on, slide, last_event_.  false: a member's solve failed
  bool ProcessLaserOdom(const lio_est_frame *frames, lio_solve_report *reps);
  // include/lio_est_from_odom.h: PushFrames / ProcessCompactData of every (initialised) member with the clouds read where src[w] (mapping.h:
  // OdomSweep) says, no cloud through the host.  T_in: size() poses (PushFramesFrom); T_out: size() poses that went in, or null.  The caller has checked what PushFrames'
  // caller checks, and that every member has its map.  Return synchronised.
  void PushFramesFrom(const OdomSweep *src, const lio_transform_f *T_in, const double *stamps);
  bool ProcessCompactFrom(const OdomSweep *src, const double *stamps, lio_transform_f *T_out, lio_solve_report *reps);
  const int *push_stats() const { return push_stats_; }   // of the last PushFrames (lio_est_batch_push_stats)
  const int *from_odom_stats() const { return from_stats_; }   // of the last device-fed call (lio_est_batch_from_odom_stats)
  // waits for everything the batch has enqueued (the marginalizations of the last Solve)
  void Sync();
  const BatchClock &clock();   // waits for the batch's stream (the device stage times come from events on it)
  // Test hook (lio_est_batch_stage_digest): a 64-bit digest per window of what stage `stage` of the LAST Solve() left on the device —
  // 0 filtered local map (in order), 1 K-NN grid (cell table relative to the window's base + the cell-sorted points as a multiset per
  // cell run: the placement order inside a cell is not defined), 2 feature flags, 3 plane coefficients of the set flags, 4 the newest
  // frame's Gauss-Newton state, 5 the trust-region loop's final state, 6 the final moments partials.  Waits for the batch.
  void StageDigest(int stage, unsigned long long *out);
  // Test hook (lio_est_batch_get_moments): window w's moments at the point its last Solve() accepted — S_buf at st.s_cur, Wo x 258
  // (S 16 x 16 row-major, cost, count) — and the T_{pivot<-i} of that point (Wo x 12: R row-major, t).  false: the window was not
  // solved on the device.  Waits for the batch.
  bool GetMoments(int w, double *out, double *Rt);
  // Test hook (lio_est_batch_get_linearization): window w's DevProblem, DevState, prior buffer, scaled H and aux row as the last Solve()
  // left them on the device, as the flat arrays of include/lio_test_hooks.h.  false: not solved on the device.  Waits for the batch.
  bool GetLinearization(int w, int32_t *ints, double *problem, double *state, double *aux);
  // lio_est_get_features of a member whose last Solve() ran on the device: its feature slots live in the batch's arrays, at the
  // window's own slot offsets behind these pointers.  Waits for the batch.
  void FeatureSlots(int w, const uint8_t **valid, const float4 **coef, const float **score);
  hipStream_t stream() const { return stream_; }
  int device() const { return device_id_; }
  // execution choices (batch_kernels.h: BatchKnobs) by name: lanes_per_query, loop_groups, aux_threads, finish_threads, time_kernels;
  // false: unknown name or a value the knob does not take
  bool SetOption(const char *name, int value);
  const BatchKnobs &knobs() const { return knobs_; }
  bool window_ok(int w) const { return w >= 0 && w < int(ok_.size()) && ok_[size_t(w)] != 0; }   // the last Solve() solved window w

 private:
  struct Slab {   // offsets (doubles) into a window's scratch slab
    size_t prior[2], imu, lmap, prior_out, exprior, Hcur, Sbuf, prof, marg_imu, marg_lmap, marg_prior_out, marg_A, marg_info, total;
  };
  struct Win {
    Estimator *e = nullptr;
    bool device = false;                       // on the device path in the Solve in progress
    std::shared_ptr<MargPrior> prior_used;     // the prior of the problem in flight
    std::shared_ptr<MargPrior> dev_prior[2];   // which host object each of the two device prior buffers holds
    int cur = 0;                               // buffer holding prior_used
    int bpf = 1, max_slots = 0;
    int key_bits = 0;                          // SegVoxFilter::bits_taken of the window's local map in its last solve (0: not known yet)
    int push_bits = 0;                         // ... and the most over the clouds of its last push (its own figure: a sweep is not a local map)
    size_t part_off = 0;                       // doubles into partials_
  };
  void Init(), Close() noexcept;
  // One window's sweep of a push, wherever it lies: the loop over the windows (PushAll) is stated once for PushFrames and PushFramesFrom
  struct PushInput {
    Rigidf transform_in;
    CloudSrc surf, corner;   // all of a call in one place (cloud_src.h)
    double stamp;
    MapFullSource full;      // the device's: the full cloud the window's map takes in the same launch (set false: none)
  };
  void PushAll(const PushInput *in);
  void PushFrom(const OdomSweep *src, const Rigidf *T_in, const double *stamps, bool composite);
  bool SolveRefreshSlide(lio_solve_report *reps);   // ProcessLaserOdom behind the push: Solve, RefreshMap where it is on, slide, last_event_
  void FetchPrior(int w, int buf, MargPrior &pr);
  void Materialize(int w, int buf);
  std::vector<Estimator *> m_;
  std::vector<Win> win_;
  hipStream_t stream_ = nullptr;
  // The trust-region loop runs in up to kGroups groups of windows, each a launch chain on a stream of its own: a group's step
  // kernel (one workgroup per window: a quarter of the chip at 64 windows) overlaps the other groups' moments passes.  The
  // marginalization runs on a stream of its own behind the loop and is joined before the next solve's problems go up: it
  // overlaps the next solve's filter, features and rounds.
  static constexpr int kGroups = 4;
  hipStream_t stream_grp_[kGroups] = {}, stream_marg_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_grp_[kGroups] = {}, ev_marg_ = nullptr;
  bool marg_in_flight_ = false;
  BatchKnobs knobs_;
  std::vector<char> ok_;
  int device_id_ = 0;
  hipEvent_t ev_[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> ev_k_;        // time_kernels: 4 events per iteration and group (aux | moments | step boundaries)
  int ev_k_used_ = 0;
  hipEvent_t ev_wait_[2] = {nullptr, nullptr};   // around the wait for the previous marginalization
  bool ev_wait_valid_ = false;
  bool ev_valid_ = false;
  Slab lay_{};
  BatchClock clk_;
  // pinned staging (one entry per window)
  HostBuf<BatchWin> h_win_; HostBuf<BatchGrid> h_grid_; HostBuf<OdomState> h_odom_;
  HostBuf<BatchSolve> h_bs_; HostBuf<DevProblem> h_pb_; HostBuf<DevState> h_st_; HostBuf<DevMarg> h_mg_;
  HostBuf<double> h_prior_;   // one ds_prior_mats_size(MARG_MAX_N) slot per window: priors on their way to the device
  HostBuf<int> h_nconv_;
  // device
  DBuf<BatchWin> d_win_; DBuf<BatchGrid> d_grid_; DBuf<OdomState> d_odom_;
  DBuf<BatchSolve> d_bs_; DBuf<DevProblem> d_pb_; DBuf<DevState> d_st_; DBuf<DevMarg> d_mg_;
  DBuf<double> slab_, partials_, odom_partials_;
  DBuf<float4> local_all_, filtered_all_, sorted_all_, coef_all_;
  // The one segmented voxel filter of the part (seg_vox.h): Solve's local maps and PushFrames' sweeps take turns on stream_, and each reads its
  // results behind its own wait.  Solve's K-NN cell sort borrows the filter's sort scratch between the two.
  SegVoxFilter vox_;
  DBuf<SegDesc> d_seg_;     // the K-NN cell sort's segments
  HostBuf<SegDesc> h_seg_;
  DBuf<float> score_all_;
  DBuf<int> cells_all_, nconv_;
  DBuf<uint8_t> valid_all_;
  // the per-sweep work of the members (est_push.h)
  PushChain push_;
  std::vector<PushPlan> plans_;
  int push_stats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int from_stats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t ev_slide_ = nullptr;   // behind the upload of the slide records: the next call rewrites their pinned staging
  HostBuf<BpSlide> h_slide_;
  DBuf<BpSlide> d_slide_;
};

// A batch of at least kBatchSplitFrom windows is TWO EstimatorBatch objects (the first and the second half of the windows) solved side by
// side from two host threads: one part's host phases (describe, pack, write-back), syncs and latency-bound stages fill with the other
// part's kernels (tools/batches_in_flight.py: 2 x 256 windows 20.1 k solves/s against 19.0 k for 1 x 512, 2 x 64 17.4 k against 16.1 k).
// Every window's results are those of the window alone whatever the partition (the batch's contract), so the split is an execution
// choice like the others: the option "parts" (0: by size, 1, 2).  Windows are addressed by their index in the whole batch.
class BatchParts {
 public:
  static constexpr int kBatchSplitFrom = 96;   // measured (profiles/r6_n_batch_parts.txt): 16 .. 64 windows within noise, 96: + 4 %, 128 .. 512: + 7-8 %
  explicit BatchParts(const std::vector<Estimator *> &windows) : e_(windows) { Build(); }
  bool built() const { return bool(b_[0]); }   // false: a re-partition failed and left no parts
  int size() const { return int(e_.size()); }
  // "parts" re-partitions (the options set so far are applied to the new parts); every other name is EstimatorBatch::SetOption on every part
  bool SetOption(const char *name, int value);
  void Solve(lio_solve_report *reps);   // reps: size() reports, or null
  // `steps` times: Restore() every window, Solve; then Sync.  Every part loops on its own: nothing ties the parts' steps together.  false: a
  // window had no snapshot or is not initialised (both parts stop).
  bool SolveRestored(int steps, lio_solve_report *reps);
  // include/lio_est_push_batch.h: every part pushes and slides its own windows on its own stream.  PushReady: every window is initialised and
  // none refuses its frame — the caller's check in front of PushFrames / ProcessLaserOdom, before any window is touched.
  bool PushReady() const;
  void PushFrames(const lio_est_frame *frames);
  void SlideWindows();
  bool ProcessLaserOdom(const lio_est_frame *frames, lio_solve_report *reps);   // false: a window's solve failed
  void PushStats(int out[8]) const;   // the parts' counters of the last push, added up
  // include/lio_est_from_odom.h: the arrays hold size() entries; every part takes its own windows'
  void PushFramesFrom(const OdomSweep *src, const lio_transform_f *T_in, const double *stamps);
  bool ProcessCompactFrom(const OdomSweep *src, const double *stamps, lio_transform_f *T_out, lio_solve_report *reps);   // false: a window's solve failed
  void FromOdomStats(int out[8]) const;
  void Sync();
  void StageDigest(int stage, unsigned long long *out);   // out: size() digests
  bool GetMoments(int w, double *out, double *Rt) { return part(w).GetMoments(w, out, Rt); }
  bool GetLinearization(int w, int32_t *ints, double *problem, double *state, double *aux) { return part(w).GetLinearization(w, ints, problem, state, aux); }
  // two parts: host phases ran side by side (the longer one counts); device times, counts and launches add up — the parts' stages
  // overlap on the GPU, so the summed device times exceed the wall time and every rate derived from them is a lower bound
  BatchClock clock();
 private:
  void Build(), ApplyOptions();   // Build: (re)builds the parts for the partition in force and applies the options set so far
  EstimatorBatch &part(int &w) { if (w < n1_) return *b_[0]; w -= n1_; return *b_[1]; }   // the part that holds window w; w becomes its index there
  template <typename F> void ForParts(F &&f);   // f(part, first window of the part) on every part — two parts on two host threads
  std::vector<Estimator *> e_;
  std::unique_ptr<EstimatorBatch> b_[2];   // b_[1]: the second part (null: one part)
  int n1_ = 0;                             // windows of b_[0]
  int parts_opt_ = 0;                      // 0: by size, 1, 2
  std::vector<std::pair<std::string, int>> options_;   // what SetOption has set, applied again when the partition changes
};

}  // namespace lio
