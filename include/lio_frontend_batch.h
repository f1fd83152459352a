/* lio_frontend_batch.h — the feature extraction handed to the scan-to-scan odometry on the device, for many sensors in one call.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The call below exists in the product
 * only, like those of lio_ext.h, lio_full_cloud.h and lio_odom_batch.h; the oracle does not implement it.  Plain C99.
 *
 * A host that steps many sensors runs lio_pp_process_batch[_device], then lio_odom_process_batch, then
 * lio_est_batch_*.  The processor leaves a sweep's four feature clouds in device memory; lio_pp_get_cloud brings them to the host and
 * lio_odom_process_batch sends the same floats back: four copies with a wait each and five uploads per sensor.  Here the odometry takes
 * them where they lie.
 */
#ifndef LIO_FRONTEND_BATCH_H
#define LIO_FRONTEND_BATCH_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The batched odometry (this call and lio_odom_process_batch) builds the 5 m grids over all previous clouds of a call with a handful of
 * launches shared by every grid of at most this many cells.  Grids above this are built per sensor; results do not depend on it. */
#define LIO_ODOM_BATCH_GRID_CELLS_MAX 131072

/* lio_odom_process_batch (lio_odom_batch.h) with the four clouds of handles[k] taken from pp[k] on the device.  Outputs (any may be
 * null) are arrays of n_sensors.
 *
 * Same state as alone.  handles[k] ends in exactly the state lio_odom_process(handles[k], ...) would leave when given the four clouds
 * that lio_pp_get_cloud(pp[k], LIO_PP_SHARP ... LIO_PP_LESS_FLAT) returns, bit for bit, for everything lio_odom_batch.h lists: the
 * transforms, the iterations, the selected rows, lio_odom_get_iteration_trace (records and kz), both lio_odom_get_last_cloud,
 * lio_odom_full_to_end, and the next lio_odom_process, lio_odom_process_batch or lio_odom_process_batch_from_pp of the handle.  The
 * three calls may be mixed freely over a handle's life.
 *
 * Which pp[k] are accepted.  Any lio_pp whose last process call completed: lio_pp_process, lio_pp_process_rings, lio_pp_process_async
 * (waited for here), lio_pp_process_batch, lio_pp_process_batch_device or lio_pp_process_rings_batch; its results may lie in its own
 * storage or in the storage a batch shares.  Handles of different sensor types may be mixed in one call.  The same lio_pp may appear
 * more than once (several odometry handles fed the same sweep).  The same lio_odom twice is LIO_ERR_ARG.
 *
 * Refused handles.  A pp[k] that has never processed, a pp[k] whose shared results a later lio_pp_process_batch of other handles
 * overwrote (what lio_pp_get_cloud refuses, lio_c.h), and a pp[k] whose last call ended over capacity give LIO_ERR_STATE.  Null arrays
 * or entries and n_sensors < 1 give LIO_ERR_ARG; n_sensors > LIO_ODOM_BATCH_MAX_SENSORS gives LIO_ERR_CAPACITY.  All of this is checked
 * before any device work and before any handle changes.  A device failure gives LIO_ERR_DEVICE.
 *
 * The processors are only read.  After the call every lio_pp_* accessor answers what it answered before.  The storage a batch shares
 * is locked while the clouds are taken, and the call returns synchronised: a later lio_pp_process_batch may reuse the storage.
 *
 * Everything else is lio_odom_process_batch's: the per-sensor state (first call, packer, previous clouds too short, no queries), the
 * per-sensor parameters, one-after-the-other processing when num_max_iterations differs between the handles, the scratch kept by
 * handles[0] and the stream the chain runs on.  No cloud crosses to the host: one launch copies every sensor's clouds into its handle's
 * buffers and sets the state its iterations start from. */
int lio_odom_process_batch_from_pp(lio_odom *const *handles, lio_pp *const *pp, int n_sensors,
                                   lio_transform_f *transform_sum_out, lio_transform_f *transform_es_out,
                                   int32_t *iterations_out, int32_t *num_selected_out);

#ifdef __cplusplus
}
#endif
#endif
