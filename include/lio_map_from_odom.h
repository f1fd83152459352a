/* lio_map_from_odom.h — the scan-to-scan odometry handed to the scan-to-map step on the device, for many sensors in one call.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The call below exists in the product
 * only, like those of lio_ext.h, lio_full_cloud.h, lio_odom_batch.h, lio_frontend_batch.h and lio_map_batch.h; the oracle does not
 * implement it.  Plain C99.
 *
 * A host that steps many sensors runs lio_pp_process_batch[_device], lio_odom_process_batch_from_pp and
 * lio_map_process_batch.  Between the last two it brings both previous clouds of every odometry handle to the host
 * (lio_odom_get_last_cloud, a copy and a wait each) for lio_map_process_batch to upload again, and with the full-resolution cloud on
 * (lio_full_cloud.h) the sweep crosses three times more: lio_pp_get_cloud, lio_odom_full_to_end (up, a kernel, down) and
 * lio_map_set_full_cloud.  Here the map handles take all of it where it lies: the pre-initialisation chain of B sensors is three calls and
 * no cloud leaves the device.
 */
#ifndef LIO_MAP_FROM_ODOM_H
#define LIO_MAP_FROM_ODOM_H

#include "lio_c.h"
#include "lio_map_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lio_map_process_batch (lio_map_batch.h) with the clouds and transform_sum of handles[k] taken from odom[k], and its full cloud from
 * pp_or_null[k] through odom[k], on the device.  Outputs (any may be null) are arrays of n_sensors.
 *
 * Same state as the host route.  handles[k] ends in exactly the state, bit for bit, that this leaves:
 *
 *     nc = lio_odom_get_last_cloud(odom[k], 0, corner);  ns = lio_odom_get_last_cloud(odom[k], 1, surf);
 *     T  = transform_sum_ of odom[k]  (what its last process call wrote to transform_sum_out)
 *     if (pp_or_null && pp_or_null[k]) {
 *         F = lio_pp_get_cloud(pp[k], LIO_PP_RINGS);  lio_odom_full_to_end(odom[k], F, nF, F);
 *         lio_map_set_full_cloud(handles[k], F, nF);            (nF == 0 clears it)
 *     }
 *     lio_map_process_batch(handles, ..., corner, nc, surf, ns, T, ...)
 *
 * for everything lio_map_batch.h lists: lio_map_get_transform_tobe_mapped, lio_map_get_degeneracy, lio_map_get_cloud (all four),
 * lio_map_get_cube, lio_map_get_cube_state, lio_map_get_score_point_coeff, lio_map_get_surround, lio_map_get_full_cloud and the handle's
 * next call; the three outputs match too.  lio_map_process, lio_map_process_batch and this call may be mixed freely over a handle's life.
 *
 * The full cloud follows lio_odom_full_to_end: a copy while odom[k] is disabled (lio_odom_enable) or has not had its first publishing
 * step, otherwise TransformToEnd with the transform_es_, scan period and deskew switch of odom[k] as they lie on the device.  A null
 * pp_or_null, or a null entry, leaves that handle's full cloud as it is.
 *
 * The sources are only read.  After the call every lio_odom_* and lio_pp_* accessor answers what it answered before, and the next process
 * call of an odom[k] or pp[k] behaves as if this call had not been made.  The same lio_odom or lio_pp may appear more than once (one
 * sensor feeding a PointMapping handle and a MapBuilder handle).  The same lio_map twice is LIO_ERR_ARG.  The storage a lio_pp_process_batch
 * shares is locked while it is read, and the call returns synchronised: a later odometry or processor call may overwrite its buffers.
 *
 * io_ratio is not applied: which sweeps reach the map stays the caller's decision, as on the host route.
 *
 * Everything else is lio_map_process_batch's: the per-sensor state (too few from-map points, an empty filtered stack, the init flag, a
 * MapBuilder handle on a skipped call), the per-sensor parameters, one-after-the-other processing when the launch parameters differ
 * between the handles (each handle still takes its clouds on the device), the scratch kept by handles[0] and the stream the chain runs
 * on.  One launch reads every sensor's stack clouds where the odometry keeps them and writes every full cloud into its map handle; no
 * staging buffer and no upload per handle.
 *
 * Refusals, all made before any device work and before any handle changes (a handle's full cloud included).  LIO_ERR_ARG: a null
 * handles or odom array, a null handles[k] or odom[k], n_sensors < 1, the same lio_map twice.  LIO_ERR_CAPACITY: n_sensors >
 * LIO_MAP_BATCH_MAX_SENSORS, or a sensor whose pose would carry its cube window beyond the range of the packed cube keys
 * (lio_map_batch.h).  LIO_ERR_STATE: an odom[k] that has never processed; a pp[k] that has never processed, whose last call ended over
 * capacity, or whose shared results a later lio_pp_process_batch of other handles overwrote (what lio_odom_process_batch_from_pp
 * refuses); a map borrowed from an estimator (lio_est_map, lio_ext.h).  A device failure gives LIO_ERR_DEVICE. */
int lio_map_process_batch_from_odom(lio_map *const *handles, lio_odom *const *odom, lio_pp *const *pp_or_null,
                                    int n_sensors, lio_transform_f *transform_aft_mapped_out,
                                    int32_t *iterations_out, int32_t *num_selected_out);

#ifdef __cplusplus
}
#endif
#endif
