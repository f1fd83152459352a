/* lio_est_from_odom.h — the scan-to-scan odometry handed to the windows of an estimator batch on the device.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The calls below exist in the product
 * only, like those of lio_ext.h, lio_full_cloud.h, lio_map_from_odom.h and lio_est_push_batch.h; the oracle does not implement them.
 * Plain C99.
 *
 * After IMU initialisation a window takes its sweep through lio_est_process_compact, or through lio_est_batch_process_laser_odom
 * (lio_est_push_batch.h) with host pointers.  Either way the host first brings both previous clouds of the odometry handle down
 * (lio_odom_get_last_cloud, a copy and a wait each) and, with the full-resolution cloud on (lio_full_cloud.h), the processor's ring cloud
 * down, up through lio_odom_full_to_end, down and up again; the estimator then uploads the same floats once more.  Here the windows take
 * all of it where it lies: the post-initialisation step of B sensors is lio_pp_process_batch[_device], lio_odom_process_batch_from_pp
 * and lio_est_batch_process_compact_from_odom, and no cloud leaves the device.
 *
 * The arrays hold lio_est_batch_size(batch) entries; entry w belongs to window w (the order of lio_est_batch_create).
 *
 * The sources are only read.  After a call every lio_odom_* and lio_pp_* accessor answers what it answered before, and the next process
 * call of an odom[w] or pp[w] behaves as if this call had not been made.  The same lio_odom or lio_pp may feed more than one window.  The
 * storage a lio_pp_process_batch shares is locked while it is read, and the calls return synchronised: a later odometry or processor call
 * may overwrite its buffers.  The single calls, the host-fed batched calls of lio_est_push_batch.h and these may be mixed freely over a
 * handle's life.
 *
 * io_ratio is not applied: which sweeps reach the estimator stays the caller's decision, as in lio_map_process_batch_from_odom.
 *
 * Refusals, all made before any window, map or device work is touched, in this order.  LIO_ERR_ARG: a null batch; a null odom or stamps
 * array; a null transform_in array (the push call); a null odom[w].  LIO_ERR_STATE: a dissolved batch; a window that is not initialised
 * (such windows keep the per-handle route); a window whose lio_est_push_frame would refuse (de-skew from the IMU poses and no IMU sample
 * yet); a window with imu_factor off (the composite only, as lio_est_process_compact); an odom[w] that has never processed; a pp[w] that
 * has never processed, whose last call ended over capacity, or whose shared results a later lio_pp_process_batch of other handles
 * overwrote (what lio_map_process_batch_from_odom refuses).  LIO_ERR_CAPACITY: the limits of lio_est_batch_push_frames — more than
 * INT_MAX - 255 points in one cloud or more than 2^30 in the call, the full clouds included.  Without a device there is no batch; a device
 * failure gives LIO_ERR_DEVICE.
 */
#ifndef LIO_EST_FROM_ODOM_H
#define LIO_EST_FROM_ODOM_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PushFrame of every window, clouds taken from odom[w] (and the full cloud from pp_or_null[w] through odom[w]) on the device.
 *
 * Same bits as the host route.  Every window ends in exactly the state, for every getter and for the handle's next call of any kind, that
 * this leaves:
 *
 *     nc = lio_odom_get_last_cloud(odom[w], 0, corner);   ns = lio_odom_get_last_cloud(odom[w], 1, surf);
 *     if (pp_or_null && pp_or_null[w] && window w has lio_est_set_full_cloud on) {
 *         F = lio_pp_get_cloud(pp[w], LIO_PP_RINGS);  lio_odom_full_to_end(odom[w], F, nF, F);
 *         lio_map_set_full_cloud(lio_est_map(window w), F, nF);          (nF == 0 clears it)
 *     }
 *     frames[w] = { transform_in[w], surf, ns, corner, nc, stamps[w] };   then   lio_est_batch_push_frames(batch, frames)
 *
 * A null pp_or_null, a null entry, or a window whose full cloud is off leaves that window's map full cloud as it is. */
int lio_est_batch_push_frames_from_odom(lio_est_batch *batch, lio_odom *const *odom, lio_pp *const *pp_or_null,
                                        const lio_transform_f *transform_in, const double *stamps);

/* ProcessCompactData (Estimator.cc:776-856) of every (initialised) window, the message never built.  Per window it equals, on a twin
 * handle with lio_est_config.device_solve = 1 (a batch of one),
 *
 *     n   = lio_compact_encode(transform_sum_ of odom[w], corner, nc, surf, ns, pp[w] ? F : empty, ...);
 *     rc  = lio_est_process_compact(twin, compact, n, stamps[w], &transform_to_init_out[w], &reports[w]);
 *
 * with corner, surf and F as above: the prediction of the map's transform_tobe_mapped_ from the IMU-propagated body motion, its
 * transform_sum_, the receive counter and last_event, the map refresh between solve and slide, and the message's third block — a window
 * with its full cloud on and no pp[w] has its map's full cloud cleared, as an empty third block does.  Outputs may be null.
 * LIO_ERR_STATE after the windows were stepped: a window's solve failed. */
int lio_est_batch_process_compact_from_odom(lio_est_batch *batch, lio_odom *const *odom, lio_pp *const *pp_or_null,
                                            const double *stamps, lio_transform_f *transform_to_init_out_or_null,
                                            lio_solve_report *reports_or_null);

/* Counters of the batch's last call of either kind, summed over its parts:
 *   [0] clouds the chain read from a device source
 *   [1] clouds copied device-to-device as they are (both de-skew switches off)
 *   [2] full clouds written into a window's map (a cleared one counts)
 *   [3] host-to-device copies of cloud data (must be 0)
 *   [4..7] 0
 * lio_est_batch_push_stats (lio_est_push_batch.h) covers these calls too. */
int lio_est_batch_from_odom_stats(const lio_est_batch *batch, int *out8);

#ifdef __cplusplus
}
#endif
#endif
