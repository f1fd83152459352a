/* lio_ext.h — the product's entry points beyond the shared ABI.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The calls below exist
 * in the product only; the oracle does not implement them.  Plain C99.
 *
 * They complete the reference's estimator loop with its mapping half: after every solved window the frame that leaves
 * the optimisation window is added to the 21 x 21 x 11 cube map at its optimised pose (Estimator.cc:703-708), and the
 * 5 x 5 x 5 surround of that map is served down-sampled (PointMapping.cc:1217-1241: /laser_cloud_surround).
 */
#ifndef LIO_EXT_H
#define LIO_EXT_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The estimator's PointMapping base as a lio_map: BORROWED.  It is owned by the lio_est, valid until lio_est_destroy,
 * created on first use with the estimator's filter sizes, and must not be passed to lio_map_destroy.  Every lio_map_*
 * call works on it; lio_est_process_compact uses this same object.  NULL on a NULL handle or a device failure. */
lio_map *lio_est_map(lio_est *h);

/* The map-database refresh, 0 (default) | 1.  While it is on, every pushed frame also fills the optimisation-window
 * buffers of Estimator.cc:177-183 (mask, cube centre, valid list, transform, surf and corner stack per slot of a ring of
 * opt_window_size + 1; pushed at :467-485), corner clouds are kept for it (before initialisation the clouds as pushed,
 * afterwards de-skewed and filtered at corner_filter_size like the surf cloud), and lio_est_process_laser_odom /
 * lio_est_process_compact call lio_est_refresh_map between SolveOptimization and SlideWindow once initialised.  The
 * initialising step does not refresh (:590-618).  While it is off nothing of this is done or held, and turning it off
 * drops the ring.  A handle adopted by a batch is refreshed by the caller after lio_est_batch_solve. */
int lio_est_set_map_refresh(lio_est *h, int on);

/* Estimator.cc:703-708 on the current window: call after a solve and before the slide.  Slot 0's transform is first
 * replaced by the optimised lidar pose of frame window_size - opt_window_size (:2282-2286, computed in double and cast to
 * float; the reference does this under update_laser_imu, which every shipped configuration sets: always on here).
 * Returns 1 when the map was updated, 0 when slot 0 is masked or the ring is not full (:626), LIO_ERR_STATE before
 * initialisation.  The clouds never leave the device. */
int lio_est_refresh_map(lio_est *h);

/* laser_cloud_surround_downsampled_ (PointMapping.cc:1223-1234): the cubes of the last lio_map_process's 5 x 5 x 5
 * surround (every in-range cube, in the field of view or not) in list order, each cube's corner points and then its surf
 * points, through pcl's VoxelGrid at `leaf` (the reference publishes at map_filter_size = 0.6).  Returns the count and
 * copies the points (x y z intensity) when xyzi_or_null is not NULL; 0 before the first lio_map_process.  Through
 * lio_est_map the same call serves an estimator. */
size_t lio_map_get_surround(lio_map *h, float leaf, float *xyzi_or_null);

/* TEST HOOK.  The arguments of the last lio_est_refresh_map, whether it updated the map (*applied = 1) or was masked
 * (0): transform, cube centre, valid list (<= 125 entries) and the two stacks as lio_map_update_map_database takes
 * them.  The surf stack is the window frame's cloud that slot 0 names, as it is NOW: read it before the next pushed
 * frame.  Every output pointer may be NULL.  LIO_ERR_STATE before the first refresh or when the frame has left the window. */
int lio_est_get_last_map_refresh(const lio_est *h, int *applied, lio_transform_f *T, int cube_center[3], uint32_t *valid_idx, int *n_valid,
                                 size_t *n_corner, float *corner_xyzi_or_null, size_t *n_surf, float *surf_xyzi_or_null);

#ifdef __cplusplus
}
#endif
#endif
