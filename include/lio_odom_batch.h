/* lio_odom_batch.h — the scan-to-scan odometry for many independent sensors through one launch chain.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The call below exists in the product
 * only, like those of lio_ext.h and lio_full_cloud.h; the oracle does not implement it.  Plain C99.
 *
 * A host that steps many sensors already batches the feature extraction (lio_pp_process_batch) and the window solves
 * (lio_est_batch_*).  lio_odom_process in between costs up to 25 x 2 launches, a correspondence launch every fifth iteration and four to
 * five host waits for a few hundred queries; here the sensors of one call share those launches and waits.
 */
#ifndef LIO_ODOM_BATCH_H
#define LIO_ODOM_BATCH_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most sensors one call takes; more give LIO_ERR_CAPACITY. */
#define LIO_ODOM_BATCH_MAX_SENSORS 1024

/* PointOdometry::Process (PointOdometry.cc:294-683) for n_sensors independent sensors, one sweep each, through ONE launch chain.
 * Array k of every argument belongs to handles[k]; the four clouds are what lio_odom_process takes.  Outputs (any may be null) are
 * arrays of n_sensors.  Every handle ends in exactly the state lio_odom_process on it alone would have left, bit for bit.
 *
 * Same bits as alone.  After the call lio_odom_get_iteration_trace (records and kz), lio_odom_get_last_cloud, lio_odom_full_to_end and
 * the next lio_odom_process or lio_odom_process_batch of a handle answer exactly what they would after lio_odom_process of the same
 * sweep on that handle alone; the two calls may be mixed freely over a handle's life.  A sensor's row sums are formed over the
 * partition it has alone (its own block count and stride), by the device code lio_odom_process runs.
 *
 * Per-sensor state.  Inside one call each of these applies to the sensor it belongs to while the others iterate: a handle on its first
 * call only stores its clouds (:302-310); a handle with lio_odom_enable(h, 0) only packs; a handle whose previous clouds are not > 10
 * corner and > 100 surf points keeps its transform_es_ and runs zero iterations; a handle with no sharp and no flat points runs its
 * iterations with zero selected rows.  A sensor that converges stays frozen while the others go on; the chain ends at the first look
 * (every fifth iteration) that finds every iterating sensor converged, or after num_max_iterations.
 *
 * Per-sensor parameters.  scan_period, io_ratio and no_deskew may differ between the handles.  If num_max_iterations differs between
 * them, the call processes the handles one after the other as lio_odom_process does: the same results, no shared chain.
 *
 * Arguments are checked before any device work and before any handle changes: a null handle or array, n_sensors < 1, a null cloud
 * with a non-zero count or the same handle twice give LIO_ERR_ARG; n_sensors > LIO_ODOM_BATCH_MAX_SENSORS gives LIO_ERR_CAPACITY.  A
 * device failure gives LIO_ERR_DEVICE.
 *
 * Ownership.  Results live in each handle's own buffers, as after lio_odom_process.  The chain's scratch (argument table, partial sums,
 * index table, trace table, mailbox) is kept by handles[0] and freed with it; it holds no results, so a later call with other handles
 * invalidates nothing.  The chain runs on handles[0]'s stream; the other handles are idle, since every lio_odom_* call returns
 * synchronised.  Like every lio_odom_* call it must not run concurrently with another call on one of its handles. */
int lio_odom_process_batch(lio_odom *const *handles, int n_sensors,
                           const float *const *sharp_xyzi, const size_t *n_sharp,
                           const float *const *less_sharp_xyzi, const size_t *n_less_sharp,
                           const float *const *flat_xyzi, const size_t *n_flat,
                           const float *const *less_flat_xyzi, const size_t *n_less_flat,
                           lio_transform_f *transform_sum_out, lio_transform_f *transform_es_out,
                           int32_t *iterations_out, int32_t *num_selected_out);

#ifdef __cplusplus
}
#endif
#endif
