/* lio_map_batch.h — the scan-to-map step for many independent sensors through one launch chain.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The call below exists in the product
 * only, like those of lio_ext.h, lio_full_cloud.h and lio_odom_batch.h; the oracle does not implement it.  Plain C99.
 *
 * A host that steps many sensors already batches the feature extraction (lio_pp_process_batch), the scan-to-scan
 * odometry (lio_odom_process_batch, lio_odom_process_batch_from_pp) and the window solves (lio_est_batch_*).  lio_map_process in between
 * costs three launches per Gauss-Newton round, two or three convergence peeks and host waits at the layout pass, the voxel-filter counts,
 * the from-map bounds and the map update, for a few thousand queries; here the sensors of one call share the rounds' launches and every
 * wait is one pass over the handles.
 */
#ifndef LIO_MAP_BATCH_H
#define LIO_MAP_BATCH_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most sensors one call takes; more give LIO_ERR_CAPACITY. */
#define LIO_MAP_BATCH_MAX_SENSORS 1024

/* PointMapping::Process (PointMapping.cc:765-1110) or MapBuilder::ProcessMap (MapBuilder.cc:527-558) for n_sensors independent handles, one
 * sweep each.  Entry k of every argument belongs to handles[k]; the clouds and transform_sum are what lio_map_process takes.  Outputs (any
 * may be null) are arrays of n_sensors.
 *
 * Same bits as alone.  Every handle ends in exactly the state lio_map_process on it alone would have left: lio_map_get_transform_tobe_mapped,
 * lio_map_get_degeneracy, lio_map_get_cloud (all four), lio_map_get_cube, lio_map_get_cube_state, lio_map_get_score_point_coeff,
 * lio_map_get_surround and lio_map_get_full_cloud answer bit for bit what they would after the single call, and the next lio_map_process,
 * lio_map_process_batch or lio_map_update_map_database of the handle behaves as after it.  The two calls may be mixed freely over a handle's
 * life.  A sensor's row sums are formed over the partition it has alone (its own block count), by the device code lio_map_process runs.
 *
 * Per-sensor state.  Inside one call each of these applies to the sensor it belongs to while the others iterate: a handle whose from-map
 * clouds are not > 10 corner and > 100 surf points (PointMapping.cc:327-329) runs no round and no TransformUpdate; a handle with an empty
 * filtered stack runs the loop dry (iterations == num_max_iterations); a handle with lio_map_set_init_flag(h, 1) neither associates the
 * odometry increment nor updates its map; a MapBuilder handle on a call that skip_count skips only updates its map; a full cloud set on a
 * handle (lio_map_set_full_cloud) is registered once, as by the single call.  A sensor that converges stays frozen while the others go on;
 * the chain ends at the first peek (after rounds 6, 8 and 10, as in the single call) that finds every iterating sensor converged, or after
 * num_max_iterations.
 *
 * Per-sensor parameters.  corner_filter_size, surf_filter_size and skip_count may differ freely between the handles.  min_match_sq_dis,
 * min_plane_dis, num_max_iterations and the 6-DoF / 4-DoF route (map_builder with enable_4d) are parameters of the shared launches: if
 * they are not equal over the handles of a call, the call processes the handles one after the other as lio_map_process does — the same
 * results, no shared chain.
 *
 * Arguments are checked before any device work and before any handle changes: a null handle or array (transform_sum included),
 * n_sensors < 1, a null cloud with a non-zero count or the same handle twice give LIO_ERR_ARG; n_sensors > LIO_MAP_BATCH_MAX_SENSORS gives
 * LIO_ERR_CAPACITY, and so does a sensor whose pose would carry its cube window beyond the range of the packed cube keys (about 24.7 km
 * from the map's origin, see lio_map_process in lio_c.h).  A handle borrowed from an estimator (lio_est_map, lio_ext.h) gives LIO_ERR_STATE: its estimator steps it, and taking
 * such handles into a batch is left to a later version.  A device failure gives LIO_ERR_DEVICE.
 *
 * Ownership.  Results live in each handle's own buffers, as after lio_map_process.  The chain's scratch (record tables, the concatenated
 * stack and its round results, partial sums, bounds) is kept by handles[0] and freed with it; it holds no results, so a later call with
 * other handles invalidates nothing.  The shared launches run on handles[0]'s stream; the call returns synchronised.  Like every lio_map_*
 * call it must not run concurrently with another call on one of its handles. */
int lio_map_process_batch(lio_map *const *handles, int n_sensors,
                          const float *const *corner_last_xyzi, const size_t *n_corner,
                          const float *const *surf_last_xyzi, const size_t *n_surf,
                          const lio_transform_f *transform_sum,
                          lio_transform_f *transform_aft_mapped_out, int32_t *iterations_out, int32_t *num_selected_out);

#ifdef __cplusplus
}
#endif
#endif
