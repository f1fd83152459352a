/* lio_est_wide.h — the device trust-region loop for seven optimised frames (window 12 / optimisation window 7, the
 * reference's config/indoor_test_config.yaml).
 *
 * The product only (liblio_hip.so); the oracle does not implement these calls.  Plain C99.
 *
 * Seven optimised frames are 126 tangent unknowns (120 with a constant extrinsic), n_pad = 128: the largest problem whose
 * H the step kernel holds in LDS (docs/wide_window.md).  The device loop and the single-window host path agree to about
 * 1e-7, not in bits, so a window of seven keeps the host path until its handle asks for the device loop here.
 */
#ifndef LIO_EST_WIDE_H
#define LIO_EST_WIDE_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIO_DEVICE_SOLVE_LIMIT_DEFAULT 6
#define LIO_DEVICE_SOLVE_LIMIT_MAX 7

/* The largest optimisation window of this handle that the device loop takes: 6 (default) or 7.  It holds wherever the
 * device loop can serve the handle: as a member of any lio_est_batch and for a lio_est_config.device_solve = 1 handle (a
 * batch of one).  A batch may mix handles with and without it; a handle whose opt_window_size exceeds its limit is
 * solved by the single-window path inside the same call, as before.  With 7 the whole chain of such a window runs on
 * the device: packing, aux row, moments and step, write-back, the marginalization, and the prior stays resident between
 * solves; lio_est_batch_get_linearization, _get_moments and _stage_digest serve it like a smaller window.
 * The limit is a choice of the handle, not part of its state: lio_est_snapshot / _restore / _copy_snapshot leave it
 * alone.  It takes effect at the next solve (a solve is one blocking call: there is no state in which it is refused).
 * LIO_ERR_ARG: NULL handle, or a value other than 6 or 7. */
int lio_est_set_device_solve_limit(lio_est *h, int max_opt_window);

/* The handle's current limit; LIO_ERR_ARG (negative) on a NULL handle. */
int lio_est_get_device_solve_limit(const lio_est *h);

#ifdef __cplusplus
}
#endif
#endif
