// resident_moments.hip — host driver of the resident lidar-moments kernel (see resident_moments.h).  Host code only: the kernel,
// ResidentArgs and the LIO_RES_* layout are solve_kernels.{h,hip}'s.
#include "resident_moments.h"

#include <atomic>

namespace lio {
static const bool g_debug_timing = std::getenv("LIO_DEBUG_TIMING") != nullptr;   // read once: the solve is a hot path

// Resident kernels hold their CUs until the host (or a peer block) feeds them, so the blocks of ALL of them must be co-resident:
// a process that drives many windows admits only as many as fit (four moments kernels of ~100 blocks);
// a solve that is not admitted takes the launch path, with the same results.
static std::atomic<int> g_resident_moments{0};
static const int kMaxResidentMoments = 4;

void ResidentMoments::Init(int mode) {
  configured_ = mode != 2;
  never_ = mode == 3;
  d_relay_.reserve(size_t(LIO_MAX_FRAMES) * LIO_RES_DOOR);
  LIO_HIP(hipMemset(d_relay_.p, 0, sizeof(double) * LIO_MAX_FRAMES * LIO_RES_DOOR));
  d_part_.reserve(size_t(LIO_RES_MAX_BLOCKS) * LIO_MOMENT_OUT);
  LIO_HIP(hipMemset(d_part_.p, 0, sizeof(double) * LIO_RES_MAX_BLOCKS * LIO_MOMENT_OUT));   // flags: no pass has sequence number 0
  h_door_.alloc(size_t(LIO_MAX_FRAMES) * LIO_RES_DOOR, hipHostMallocCoherent, true);
  h_out_.alloc(size_t(LIO_MAX_FRAMES) * LIO_RES_OUT, hipHostMallocCoherent, true);   // the diagnostic slots are read whether or not the kernel fills them
  h_words_.alloc(LIO_MAX_FRAMES + 2, hipHostMallocCoherent, true);   // + the relay block's word + its echo
  int khz = 0, dev = 0;
  LIO_HIP(hipGetDevice(&dev));
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;   // 100 MHz on gfx9
  tick_us_ = 1e3 / double(khz);
  timeout_ticks_ = (long long)(0.2 * 1e3 * khz);   // 200 ms without a doorbell: the block posts LIO_RES_EXPIRED and exits
}

// Blocks per frame of the resident form's partition (0: the window does not fit) and, in *per_lane, the residuals a lane keeps.
// Fewer residuals per lane = more blocks = a shorter accumulate phase (1.7 us of MFMA per wave at four, 0.85 at two); the frame
// fold costs one memory round trip as long as a frame's blocks fit one batch of loads (RES_FOLD_BATCH = 64).  So: the smallest
// per-lane count whose blocks are all co-resident (<= 256) with at most 64 per frame.  A pure function of the window's slot
// counts, so the partition — and with it every bit of the result — does not depend on how a pass is executed.
int ResidentMoments::Bpf(int max_slots, int nframes, int *per_lane) const {
  if (per_lane) *per_lane = 0;
  if (!configured_) return 0;
  for (int r : {1, 2, 4, 8}) {
    if (per_lane_ > 0 && r != per_lane_) continue;
    const int b = resident_blocks_per_frame(max_slots, nframes, r);
    if (b > 0 && (b <= 64 || r == 8 || per_lane_ > 0)) { if (per_lane) *per_lane = r; return b; }
  }
  return 0;
}

void ResidentMoments::LaunchKernel(unsigned first_seq, hipStream_t s) {
  ResidentArgs ra{h_door_.p, h_out_.p, h_words_.p, first_seq, timeout_ticks_, d_relay_.p, d_part_.p, g_debug_timing ? 1 : 0};
  launch_seq_ = first_seq;   // (a launch's STOP value is derived from it; see AwaitWord for the one case where the HBM copy must be cleared)
  launch_lidar_moments_resident(args_, ra, lanes_, valid_, coef_, s);
}

// The resident kernel of this solve: launched behind everything the feature stage enqueued on s; it returns when the host
// writes LIO_RES_STOP (End) or after timeout_ticks_ without a doorbell.
bool ResidentMoments::Begin(const MomentArgs &ma, bool owner_ok, const uint8_t *valid, const float4 *coef, hipStream_t s) {
  if (!allowed_ || never_ || !owner_ok) return false;
  int max_slots = 0;
  for (int k = 0; k < ma.nframes; ++k) max_slots = std::max(max_slots, ma.fr[k].nslots);
  int per_lane = 0;
  if (Bpf(max_slots, ma.nframes, &per_lane) != ma.blocks_per_frame || ma.blocks_per_frame <= 0) return false;
  if (seq_ > 0xF0000000u) {   // 32-bit sequence numbers: start over long before they wrap (no launch is in flight here)
    LIO_HIP(hipStreamSynchronize(s));
    LIO_HIP(hipMemset(d_part_.p, 0, sizeof(double) * LIO_RES_MAX_BLOCKS * LIO_MOMENT_OUT));
    std::memset(h_words_.p, 0, sizeof(unsigned) * (LIO_MAX_FRAMES + 2));
    seq_ = 0;
  }
  if (g_resident_moments.fetch_add(1) >= kMaxResidentMoments) { g_resident_moments.fetch_sub(1); return false; }
  struct Admission { bool keep = false; ~Admission() { if (!keep) g_resident_moments.fetch_sub(1); } } admission;   // released if the launch throws
  args_ = ma; valid_ = valid; coef_ = coef; lanes_ = per_lane;
  bpf_ = ma.blocks_per_frame; nframes_ = ma.nframes;
  for (int f = 0; f < nframes_; ++f) {   // idle doorbell: neither the expected sequence number nor STOP
    __atomic_store_n(reinterpret_cast<unsigned long long *>(h_door_.p + f * LIO_RES_DOOR + 7), 0ull, __ATOMIC_RELEASE);
    __atomic_store_n(reinterpret_cast<unsigned long long *>(h_door_.p + f * LIO_RES_DOOR + 15), 0ull, __ATOMIC_RELEASE);
  }
  if (time_launch_) {
    hipEvent_t a, b;
    LIO_HIP(hipEventCreate(&a)); LIO_HIP(hipEventCreate(&b));
    LIO_HIP(hipEventRecord(a, s));
    launch_events_.push_back({a, b});
  }
  relaunches_ = 0;
  LaunchKernel(seq_ + 1, s);
  active_ = true; admission.keep = true;
  return true;
}

int ResidentMoments::LaunchStats(double *total_ms, hipStream_t s) {
  LIO_HIP(hipStreamSynchronize(s));
  for (auto &ev : launch_events_) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { launch_ms_ += ms; ++launches_; }
    (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second);
  }
  launch_events_.clear();
  if (total_ms) *total_ms = launch_ms_;
  return launches_;
}

void ResidentMoments::Ring(const MomentArgs &ma) {
  t_ring_ = now_ms();
  const unsigned seq = ++seq_;
  const double sd = double(seq);
  for (int f = 0; f < nframes_; ++f) {
    double *d = h_door_.p + f * LIO_RES_DOOR;
    const MomentFrame &fr = ma.fr[f];
    // payload first, the sequence slot of each cache line last (x86 keeps the order of stores; the GPU reads a line at a time)
    for (int k = 0; k < 7; ++k) d[k] = fr.R[k];
    __atomic_store_n(reinterpret_cast<unsigned long long *>(d + 7), *reinterpret_cast<const unsigned long long *>(&sd), __ATOMIC_RELEASE);
    d[8] = fr.R[7]; d[9] = fr.R[8]; d[10] = fr.t[0]; d[11] = fr.t[1]; d[12] = fr.t[2]; d[13] = 0.0; d[14] = 0.0;
    __atomic_store_n(reinterpret_cast<unsigned long long *>(d + 15), *reinterpret_cast<const unsigned long long *>(&sd), __ATOMIC_RELEASE);
  }
  if (g_debug_timing) {   // ring -> the relay's echo of the sequence number: the inbound PCIe leg + one word back
    const volatile unsigned *echo = h_words_.p + LIO_MAX_FRAMES + 1;
    for (unsigned long it = 0; it < 2000000ul && __atomic_load_n(echo, __ATOMIC_ACQUIRE) != seq_; ++it) __builtin_ia32_pause();
    echo_ms_ += now_ms() - t_ring_;
  }
}

// Waits for frame f's completion word of the pass in flight.  A relay timeout (this host thread was held up for > 200 ms before
// it rang) can only show while NO frame of the pass has been posted: the relay gives up between passes, and a pass that was
// started is posted whole.
void ResidentMoments::AwaitWord(int f, hipStream_t s) {
  const unsigned seq = seq_;
  const volatile unsigned *w = h_words_.p;
  for (unsigned long it = 1;; ++it) {
    if (__atomic_load_n(w + f, __ATOMIC_ACQUIRE) == seq) return;
    if (__atomic_load_n(w + LIO_MAX_FRAMES, __ATOMIC_ACQUIRE) == LIO_RES_EXPIRED) {
      if (__atomic_load_n(w + f, __ATOMIC_ACQUIRE) == seq) return;
      if (f > 0 && __atomic_load_n(w + 0, __ATOMIC_ACQUIRE) == seq) throw DeviceError("resident moments kernel gave up in the middle of a pass");
      // let that launch drain and start a new one for the pass that is pending; its doorbell is still rung.  Twice at most: a
      // kernel that keeps expiring is not being scheduled whole (its blocks are not co-resident) and no retry will change that.
      LIO_HIP(hipStreamSynchronize(s));
      if (++relaunches_ > 2) throw DeviceError("resident moments kernel expired three times within one solve (its blocks are not co-resident?)");
      h_words_.p[LIO_MAX_FRAMES] = 0;
      // The expired relay left ITS stop value in the HBM copy of the doorbell.  If that launch never served a pass, the one that
      // replaces it starts at the same sequence number and has the same stop value: clear the copy, or the new workers leave on it
      // before the new relay republishes the pending pass.
      LIO_HIP(hipMemsetAsync(d_relay_.p, 0, sizeof(double) * LIO_MAX_FRAMES * LIO_RES_DOOR, s));
      LaunchKernel(seq, s);
      continue;
    }
    __builtin_ia32_pause();
    if ((it & 0xFFFFu) == 0) {
      const hipError_t e = hipStreamQuery(s);
      if (e != hipErrorNotReady && e != hipSuccess) throw DeviceError(std::string("resident moments pass failed: ") + hipGetErrorString(e));
      if (e == hipSuccess && h_words_.p[LIO_MAX_FRAMES] != LIO_RES_EXPIRED && __atomic_load_n(w + f, __ATOMIC_ACQUIRE) != seq)
        throw DeviceError("resident moments kernel ended without posting its pass");   // the kernel is gone although nobody stopped it
    }
  }
}

void ResidentMoments::UnpackFrame(int f, FrameMoments &fm) {
  // the device posts the upper triangle of the 13 x 13 tile (it is symmetric bit for bit); S is the padded 16 x 16 tile
  static const struct TriMap { int at[256]; TriMap() { for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) { const int a = std::min(i, j), b = std::max(i, j); at[i * 16 + j] = (b < 13) ? a * 13 - a * (a - 1) / 2 + (b - a) : -1; } } } tri;
  const double *rec = h_out_.p + size_t(f) * LIO_RES_OUT;
  for (int k = 0; k < 256; ++k) fm.S[k] = tri.at[k] >= 0 ? rec[tri.at[k]] : 0.0;
  fm.cost = rec[LIO_RES_NTRI]; fm.count = rec[LIO_RES_NTRI + 1];
}

// bookkeeping of a finished pass (all frames in): device-side phase stamps, busy time, algorithmic bytes
void ResidentMoments::PassDone() {
  const int nf = nframes_;
  double busy = 0, polls = 0;
  for (int f = 0; f < nf; ++f) {
    const double *rec = h_out_.p + size_t(f) * LIO_RES_OUT;
    for (int q = 0; q < 4; ++q) diag_us_[q] += rec[258 + q] * tick_us_ / nf;
    polls += rec[262] / nf;
    relay_us_ += rec[263] * tick_us_ / nf;
    busy = std::max(busy, rec[261]);
  }
  busy_us_ += busy * tick_us_;   // doorbell copy seen -> sums posted, slowest frame
  { double nres = 0; for (int f = 0; f < nf; ++f) nres += args_.fr[f].nslots; bytes_ += 60.0 * nres; }   // 60 B per lidar residual
  polls_ += polls; ++passes_; ++passes_total_;
  if (g_debug_timing) ring_to_done_ms_ += now_ms() - t_ring_;
}

void ResidentMoments::WaitFrame(int f, FrameMoments &fm, hipStream_t s) {
  AwaitWord(f, s);
  UnpackFrame(f, fm);
  if (f == nframes_ - 1) PassDone();
}

void ResidentMoments::Wait(std::vector<FrameMoments> &m, hipStream_t s) {
  for (int f = 0; f < nframes_; ++f) AwaitWord(f, s);
  for (int f = 0; f < nframes_; ++f) UnpackFrame(f, m[f + 1]);
  PassDone();
}

void ResidentMoments::End(hipStream_t s) {
  allowed_ = false;
  if (!active_) return;
  const double stop = LIO_RES_STOP(launch_seq_);
  const unsigned long long bits = *reinterpret_cast<const unsigned long long *>(&stop);
  for (int f = 0; f < nframes_; ++f) {
    __atomic_store_n(reinterpret_cast<unsigned long long *>(h_door_.p + f * LIO_RES_DOOR + 7), bits, __ATOMIC_RELEASE);
    __atomic_store_n(reinterpret_cast<unsigned long long *>(h_door_.p + f * LIO_RES_DOOR + 15), bits, __ATOMIC_RELEASE);
  }
  active_ = false;   // the kernel leaves within one poll; whatever is enqueued on s next is ordered behind it
  g_resident_moments.fetch_sub(1);
  if (time_launch_ && !launch_events_.empty()) (void)hipEventRecord(launch_events_.back().second, s);
}

void ResidentMoments::PrintDebugTiming() {
  if (!g_debug_timing || !passes_) return;
  std::fprintf(stderr, "[lio_hip timing] resident moments: %d passes; folding block, from the doorbell copy seen (us): accumulated %.2f, parked %.2f, all flags in %.2f, sums posted %.2f; relay detect -> copy seen %.2f; host ring -> moments unpacked %.2f; HBM polls %.1f; %d worker blocks\n",
               passes_, diag_us_[0] / passes_, diag_us_[1] / passes_, diag_us_[2] / passes_, diag_us_[3] / passes_,
               relay_us_ / passes_, 1e3 * ring_to_done_ms_ / passes_, polls_ / passes_, bpf_ * nframes_);
  std::fprintf(stderr, "[lio_hip timing] resident moments: host ring -> relay's echo seen %.2f us (the host waits for it only under LIO_DEBUG_TIMING)\n",
               1e3 * echo_ms_ / passes_);
  echo_ms_ = 0;
  diag_us_[0] = diag_us_[1] = diag_us_[2] = diag_us_[3] = polls_ = relay_us_ = ring_to_done_ms_ = 0; passes_ = 0;
}

}  // namespace lio
