/* lio_full_cloud.h — the full-resolution sweep on the device and the registered clouds served from it.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The calls below exist in the
 * product only, like those of lio_ext.h; the oracle does not implement them.  Plain C99.
 *
 * The full-resolution cloud is the third block of /compact_data.  The reference carries it to the sweep's end in the odometry
 * (PointOdometry.cc:261-292, :725-730), registers it in the scan-to-map stage while the IMU is not initialised
 * (PointMapping.cc:1244-1251: /cloud_registered), keeps a copy per window frame in the estimator (Estimator.cc:482: full_stack_) and
 * corrects the newest copy at the end of every solve (:2355-2420).  Everything is off by default: while lio_est_set_full_cloud is 0 and
 * no lio_map_set_full_cloud was made, no call of lio_c.h or lio_ext.h does or holds anything for it.
 */
#ifndef LIO_FULL_CLOUD_H
#define LIO_FULL_CLOUD_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Where an entry of the estimator's full-cloud ring stands. */
#define LIO_FULL_MAP_FRAME 1  /* pushed before initialisation: registered by the scan-to-map stage, integer intensities */
#define LIO_FULL_SENSOR_RAW 2 /* pushed after initialisation, not yet corrected: the sweep as it came, ring + rel_time intensities */
#define LIO_FULL_SENSOR_END 3 /* corrected by a completed solve: at the sweep's end, intensities kept */

/* PointOdometry::TransformToEnd(full_cloud_) of a publishing step (PointOdometry.cc:261-292 called at :725-730), with the transform_es_
 * of the last lio_odom_process, on the device, through the per-point body that carries that step's less-sharp and less-flat clouds:
 * s = time_factor * (w - int(w)) (0 under no_deskew); p -= s t; w = int(w); rotate by slerp(id, s, q_e).conjugate(), which this form
 * does NOT normalise; rotate by q_e; + t.  A byte copy while the odometry is disabled (lio_odom_enable(h, 0), :727) and before the
 * first publishing step: the first lio_odom_process only stores its clouds and returns before anything is published (:302-310), so
 * the full cloud of that sweep passes through untouched.  xyzi_out may equal xyzi.  n == 0 is fine. */
int lio_odom_full_to_end(lio_odom *h, const float *xyzi, size_t n, float *xyzi_out);

/* CompactDataHandler's full_cloud_ (PointMapping.cc:212-224) on the device; n == 0 clears it.  Works on lio_est_map(h) too: this is how
 * a caller of lio_est_process_laser_odom / lio_est_push_frame hands the cloud of the coming frame in. */
int lio_map_set_full_cloud(lio_map *h, const float *xyzi, size_t n);

/* full_cloud_ as it is now: returns the count and copies the points when xyzi_or_null is not NULL.  After a lio_map_process that ran
 * with the init flag off it is the /cloud_registered cloud (PointMapping.cc:1105 -> :1244-1248): every point mapped by the
 * transform_tobe_mapped_ that process ended with (PointAssociateToMap, :303-314: rot * p + pos, intensity kept).  After
 * lio_map_set_init_flag(h, 1) nothing touches it.
 * Deviation: a cloud is mapped ONCE per set.  A second lio_map_process without a new lio_map_set_full_cloud leaves it alone (the
 * reference's in-place loop cannot meet the same cloud twice either: HasNewData demands a new one). */
size_t lio_map_get_full_cloud(const lio_map *h, float *xyzi_or_null);

/* The estimator's full_stack_, 0 (default) | 1.  While it is on:
 *   - lio_est_process_compact hands the decoded full block to the estimator's map (lio_map_set_full_cloud) before the step;
 *   - every pushed frame copies the map's current full cloud, device to device, into a ring of window_size + 1 entries that is indexed
 *     like the window (Estimator.cc:482); an empty copy is allowed;
 *   - every completed solve of the handle (lio_est_solve_optimization, lio_est_process_laser_odom, lio_est_process_compact,
 *     lio_est_batch_solve for an adopted member) corrects the newest entry once, in place, on the estimator's stream:
 *     TransformToEnd(full_stack_.last(), transform_es_, 10, keep_intensity = true) (:2355-2420 under update_laser_imu; this form
 *     normalises the conjugate, :88, and keeps the intensity).  transform_es_ is the one the frame's surf cloud was pushed with; it is
 *     the identity under cutoff_deskew and with both de-skew switches off.  A second solve of the same window does not correct again;
 *   - lio_est_restore and lio_est_copy_snapshot drop the destination's ring: snapshots do not carry full clouds.
 * While it is off nothing of this is done or held, and turning it off drops the ring. */
int lio_est_set_full_cloud(lio_est *h, int on);

/* The ring entry of window frame `frame` (window_size - opt_window_size + 1 is /local/full_points, Estimator.cc:2372-2375): returns the
 * count, copies the points when xyzi_or_null is not NULL and stores LIO_FULL_* in *state_or_null.  Returns 0 and leaves the state
 * untouched for a frame without an entry. */
size_t lio_est_get_full_stack(const lio_est *h, int frame, float *xyzi_or_null, int *state_or_null);

/* A LIO_FULL_SENSOR_END entry mapped into the world by its frame's optimised lidar pose: rot = Rs[frame] * q_lb.conjugate().normalized(),
 * pos = Ps[frame] - rot * t_lb evaluated in double and cast once to float (Estimator.cc:2284-2286, :2293-2295, :2311), then
 * rot * p + pos in fp32, intensity kept.  Out of place: the ring entry is not modified.  Every output pointer may be NULL.
 * LIO_ERR_STATE for an entry in any other state, a frame without an entry and before initialisation. */
int lio_est_get_registered_full(const lio_est *h, int frame, lio_transform_f *T_out_or_null, size_t *n_out, float *xyzi_or_null);

/* TEST HOOK.  The transform_es_ kept with the ring entry of window frame `frame`.  LIO_ERR_STATE for a frame without an entry. */
int lio_est_get_full_transform_es(const lio_est *h, int frame, lio_transform_f *T_es);

/* TEST HOOK.  The estimator's TransformToEnd (Estimator.cc:62-103) on a given cloud, on the device.  keep_intensity = 0 runs the
 * production launch that de-skews the surf and corner clouds of a pushed frame (the ring is stripped from the intensity);
 * keep_intensity = 1 the form of lio_est_set_full_cloud.  Both come from one device body: their x y z are the same bits.
 * xyzi_out may equal xyzi.  n == 0 is fine and writes nothing. */
int lio_deskew_to_end(const float *xyzi, size_t n, const lio_transform_f *T_es, float time_factor, int keep_intensity, float *xyzi_out);

#ifdef __cplusplus
}
#endif
#endif
