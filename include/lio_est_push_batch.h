/* lio_est_push_batch.h — the per-sweep work of an estimator (PushFrame, SlideWindow) for the windows of a batch through one launch chain.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The calls below exist in the product
 * only, like those of lio_map_batch.h; the oracle does not implement them.  Plain C99.
 *
 * lio_est_batch_solve runs every stage of SolveOptimization as one launch over all windows, but a caller who steps B windows still had to
 * give every window its next sweep (lio_est_push_frame: an upload, a de-skew launch, the voxel filter's six launches and a host wait, per
 * window, twice with the map refresh on) and slide every window (lio_est_slide_window: one launch each).  Here the clouds of one call share
 * the launches: de-skew + keys, key layout, the segmented sort's passes, run heads, centroids — and ONE host wait per part of the batch.
 *
 * Same bits.  After lio_est_batch_push_frames every window is in exactly the state that lio_est_push_frame(window w, &frames[w].transform_in,
 * frames[w].surf_xyzi, ...) for w = 0 .. B - 1 leaves: every getter answers the same bits and the handle's next call of any kind behaves the
 * same; likewise lio_est_batch_slide_windows against lio_est_slide_window, and lio_est_batch_process_laser_odom against
 * lio_est_process_laser_odom on initialised windows (last_event, the receive counter and the map refresh included), the solve being the
 * batched one (lio_est_batch_solve; for a single handle: lio_est_config.device_solve).  The single and the batched calls may be mixed freely
 * over a handle's life.  A cloud the shared filter chain cannot take (a point beyond +-1023 cells in x or y or +-254 cells in z of the leaf
 * size, more cells than the sort's passes order, PCL's "leaf size too small") is redone by the handle's own filter inside the call; which way
 * a cloud went does not show in its bits.
 *
 * Every window must be initialised (as for lio_est_batch_solve); a fleet that is still initialising uses the per-handle calls.
 *
 * Refusals change nothing: they come before any window is touched and before any device work.  LIO_ERR_ARG: a null batch or frames array, a
 * null cloud pointer with a non-zero count.  LIO_ERR_STATE: a dissolved batch, a window that is not initialised, a window for which
 * lio_est_push_frame would refuse the frame (de-skew from the IMU poses asked for — enable_deskew without cutoff_deskew — and no IMU sample
 * processed yet).  LIO_ERR_CAPACITY: the clouds of one call hold more than 2^30 points.  A device failure gives LIO_ERR_DEVICE.
 *
 * The calls return synchronised with the uploads: the caller may reuse its host buffers on return.  Like every call on a batch they must not
 * run concurrently with another call on the batch or on one of its windows.
 */
#ifndef LIO_EST_PUSH_BATCH_H
#define LIO_EST_PUSH_BATCH_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One window's next sweep: what lio_est_push_frame takes.  Host pointers; corner_xyzi is read only while the window's map refresh is on. */
typedef struct {
  lio_transform_f transform_in;
  const float *surf_xyzi;   size_t n_surf;
  const float *corner_xyzi; size_t n_corner;
  double stamp;
} lio_est_frame;

/* PushFrame of every window; frames[w] belongs to window w of the batch (the order of lio_est_batch_create). */
int lio_est_batch_push_frames(lio_est_batch *batch, const lio_est_frame *frames);

/* SlideWindow of every window: one launch for the whole batch part, no host wait. */
int lio_est_batch_slide_windows(lio_est_batch *batch);

/* ProcessLaserOdom of every (initialised) window: push, lio_est_batch_solve, the map refresh where a handle has it on, slide.
 * reports_or_null: lio_est_batch_size reports.  LIO_ERR_STATE after the whole step when a window's solve failed, as lio_est_process_laser_odom
 * reports it for that window. */
int lio_est_batch_process_laser_odom(lio_est_batch *batch, const lio_est_frame *frames, lio_solve_report *reports_or_null);

/* Counters of the batch's last lio_est_batch_push_frames (or the push of lio_est_batch_process_laser_odom), summed over its parts:
 *   [0] clouds whose centroids came from the shared chain   [1] clouds redone by the single-window filter   [2] clouds taken as they are (both
 *   de-skew switches off: no filter)   [3] host waits of the call (one per part that had a cloud; the waits inside the single-window filter of
 *   [1] are its own)   [4] sort passes run   [5 .. 7] 0.
 * A window contributes its surf cloud and, with its map refresh on, its corner cloud: [0] + [1] + [2] = clouds of the call. */
int lio_est_batch_push_stats(const lio_est_batch *batch, int *out8);

#ifdef __cplusplus
}
#endif
#endif
