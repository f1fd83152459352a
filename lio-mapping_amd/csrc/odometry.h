// odometry.h — PointOdometry (LOAM scan-to-scan step) on the GPU.
// Reference: src/point_processor/PointOdometry.cc:237-292 (TransformToStart/End), :294-683 (Process).
#pragma once
#include <memory>

#include "cloud_kernels.h"
#include "cloud_src.h"
#include "hmath.h"

namespace lio {

struct OdoChain;

class OdometryDev {
 public:
  OdometryDev(float scan_period, int io_ratio, int max_iter, bool no_deskew);
  ~OdometryDev();
  void Process(const float *sharp, size_t n_sharp, const float *less_sharp, size_t n_ls, const float *flat, size_t n_flat, const float *less_flat,
               size_t n_lf);
  // n independent sensors, one sweep each, through one launch chain on o[0]'s stream (lio_odom_process_batch, include/lio_odom_batch.h):
  // array k of every argument belongs to o[k].  Process is the chain of one, and every sensor of a batch ends in the state it leaves, bit
  // for bit.  The chain's scratch stays with o[0].  Sensors whose max_iter differ are processed one after the other, a chain of one each.
  // in[k]: o[k]'s clouds, all of a call in one place (cloud_src.h).  The device's (lio_odom_process_batch_from_pp,
  // include/lio_frontend_batch.h): one launch copies them and sets every sensor's starting state, no copy per sensor.
  struct Clouds { CloudSrc c[4]; };   // sharp, less sharp, flat, less flat
  static void ProcessBatch(OdometryDev *const *o, int n, const Clouds *in);
  size_t GetLastCloud(int which, float *out);
  // What the next stage (include/lio_map_from_odom.h, lio_est_from_odom.h) reads of the handle, where it lies on the device; nothing of the
  // handle changes.  last: what GetLastCloud answers (0 corner, 1 surf).  to_end: what FullToEnd runs a cloud through (cloud_kernels.h).
  struct DeviceView { CloudSrc last[2]; ToEnd to_end; };
  DeviceView View() const {
    return DeviceView{{CloudSrc::device(last_corner_.p, n_last_corner_), CloudSrc::device(last_surf_.p, n_last_surf_)},
                      ToEnd{enable_odom_ && to_end_ready_ ? d_state_.p : nullptr, time_factor_, no_deskew_ ? 1 : 0}};
  }
  bool processed() const { return inited_; }   // a process call has completed
  // TransformToEnd(full_cloud_) with the last Process's transform_es_ (:725-730); a byte copy while the odometry is disabled
  void FullToEnd(const float *xyzi, size_t n, float *out);
  // the correspondence search of one iteration on caller-given clouds and transform_es_ (lio_odom_correspondences,
  // include/lio_test_hooks.h): corner_idx n_sharp x 2, surf_idx n_flat x 3, sel_out (n_sharp + n_flat) x 3
  void Correspondences(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_last_corner,
                       const float *last_surf, size_t n_last_surf, const Rigid<float> &T, int32_t *corner_idx, int32_t *surf_idx, float *sel_out);
  // the rows of one iteration on caller-given clouds, correspondences and transform_es_ (lio_gn_rows_odom, include/lio_test_hooks.h): ok_out
  // n_sharp + n_flat, rows_out x 7, partials_out nb x 28 with nb <= 64
  void Rows(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_last_corner, const float *last_surf,
            size_t n_last_surf, const int32_t *corner_idx, const int32_t *surf_idx, const Rigid<float> &T, int iter, uint8_t *ok_out, float *rows_out,
            int32_t *nb_out, double *partials_out);

  Rigid<float> transform_es_, transform_sum_;
  int iterations_done_ = 0, last_num_sel_ = 0;
  int last_kz_ = 0;                         // degeneracy test of iteration 0 (:584-615): leading update components masked
  std::vector<Rigid<float>> es_trace_;      // transform_es_ after every iteration of the last Process (lio_odom_get_iteration_trace)
  bool enable_odom_ = true;

 private:
  friend struct OdoChain;
  float scan_period_, time_factor_;
  int io_ratio_, max_iter_;
  bool no_deskew_, inited_ = false;
  hipStream_t stream_ = nullptr;
  DBuf<float4> sharp_, flat_, less_sharp_, less_flat_, last_corner_, last_surf_, full_;
  bool to_end_ready_ = false;  // a Process has run TransformToEnd: d_state_ holds the transform_es_ it used
  size_t n_last_corner_ = 0, n_last_surf_ = 0;
  DBuf<OdomState> d_state_;
  void Accumulate(const OdomState &st);   // the host's end of a step that ran with the odometry enabled (:654-663)
  std::unique_ptr<OdoChain> chain_;       // the chain of the calls with this handle first (allocated on first use): table, indices, partials, traces, mailbox
  OdoChain &Chain();
  // the table and grids of a chain of this handle alone over caller-given clouds and transform_es_ (Correspondences, Rows)
  OdoChain &HookTable(const float *sharp, size_t n_sharp, const float *flat, size_t n_flat, const float *last_corner, size_t n_last_corner,
                      const float *last_surf, size_t n_last_surf, const Rigid<float> &T);
  DBuf<float> d_sel_;          // 3 floats per query (Correspondences), 7 (Rows)
  KnnGrid grid_c_, grid_s_;    // the grids over last_corner_ / last_surf_ that exceed LIO_ODOM_BATCH_GRID_CELLS_MAX cells
};

// the scan-to-scan step (odo_update_step) on device sums and a device state, in place (lio_gn_step family 1, include/lio_test_hooks.h)
void launch_gn_odo_step(const double *sums, OdomState *st, int iter, hipStream_t s);

}  // namespace lio
