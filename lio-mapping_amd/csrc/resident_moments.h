// resident_moments.h — the host half of k_lidar_moments_resident (solve_kernels.h): one launch per solve; every
// linearisation is a doorbell write + a spin on the blocks' completion words.  The owner opens a scope (Open) for the span of a
// solve, offers every filled MomentArgs to Begin (which launches at most once per scope, or refuses), rings and waits per pass,
// and calls End when the scope closes — and before the stream changes or goes away, followed by a synchronize of that stream.
#pragma once
#include "host_solver.h"   // FrameMoments; MomentArgs and the LIO_RES_* layout through solve_kernels.h, HostBuf / DBuf through dev.h

namespace lio {

class ResidentMoments {
 public:
  // mode: lio_est_config.resident_moments (2: the launch pair's own partition; 3: the resident form's partition, launch pairs only)
  void Init(int mode);
  int Bpf(int max_slots, int nframes, int *per_lane = nullptr) const;
  void ForcePerLane(int per_lane) { per_lane_ = per_lane; }   // lio_est_force_moments_per_lane (0: Bpf's rule)
  void Open() { allowed_ = true; }
  // owner_ok: what only the owner can tell (completion words in use, no kernel timing, no sharding, the only solve in flight);
  // valid / coef: the feature slots the launch reads.  false: the pass takes the launch pair.
  bool Begin(const MomentArgs &ma, bool owner_ok, const uint8_t *valid, const float4 *coef, hipStream_t s);
  bool active() const { return active_; }   // a resident kernel is waiting on the doorbell
  int nframes() const { return nframes_; }   // ... serving passes of this many frames
  void Ring(const MomentArgs &ma);
  void WaitFrame(int f, FrameMoments &fm, hipStream_t s);   // frame f (0-based) of the pass in flight, as soon as its word is in
  void Wait(std::vector<FrameMoments> &m, hipStream_t s);   // all frames: m[f + 1]
  void End(hipStream_t s);
  // lio_est_enable_kernel_timing(-1): HIP events around every launch of the resident kernel: its dispatch-to-exit span (what rocprofv3 reports)
  void LaunchTiming(bool on) { time_launch_ = on; }
  int LaunchStats(double *total_ms, hipStream_t s);
  double BusyUs(int *passes, double *bytes) const { if (passes) *passes = passes_total_; if (bytes) *bytes = bytes_; return busy_us_; }
  void PrintDebugTiming();   // LIO_DEBUG_TIMING: the per-pass averages since the last call, then reset

 private:
  void LaunchKernel(unsigned first_seq, hipStream_t s);
  void AwaitWord(int f, hipStream_t s);
  void UnpackFrame(int f, FrameMoments &fm);
  void PassDone();
  bool configured_ = true;      // lio_est_config.resident_moments != 2
  bool never_ = false;          // resident_moments = 3
  int per_lane_ = 0;            // residuals a lane keeps in registers: 0 = chosen per window (Bpf), ForcePerLane forces 1, 2, 4, 8
  int lanes_ = 4;               // ... of the launch in flight
  bool allowed_ = false;        // inside a solve scope
  bool active_ = false;
  int bpf_ = 0, nframes_ = 0;
  unsigned seq_ = 0;            // sequence number of the last pass rung (monotonic over the life of the object)
  int relaunches_ = 0;          // launches that replaced an expired one within this solve (bounded: AwaitWord)
  unsigned launch_seq_ = 0;     // first sequence number of the launch in flight (its STOP value is derived from it)
  HostBuf<double> h_door_, h_out_;   // coherent pinned host memory: doorbell, per-frame folded records
  HostBuf<unsigned> h_words_;        // ... one completion word per frame + the relay block's word + its echo
  DBuf<double> d_relay_, d_part_;    // HBM: the doorbell as republished by the relay block; the per-block records
  long long timeout_ticks_ = 0;
  double tick_us_ = 0.01;       // microseconds per wall-clock tick
  double busy_us_ = 0, bytes_ = 0; int passes_ = 0, passes_total_ = 0;   // device-side busy time of the passes (doorbell copy seen -> sums posted), SURVEY 8(d) bytes
  MomentArgs args_{};           // the launch in flight: its frames and its feature slots
  const uint8_t *valid_ = nullptr; const float4 *coef_ = nullptr;
  bool time_launch_ = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> launch_events_;
  double launch_ms_ = 0; int launches_ = 0;
  double diag_us_[4] = {0, 0, 0, 0}, polls_ = 0, relay_us_ = 0, ring_to_done_ms_ = 0, t_ring_ = 0, echo_ms_ = 0;   // LIO_DEBUG_TIMING
};

}  // namespace lio
