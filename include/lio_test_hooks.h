/* lio_test_hooks.h — test hooks that pin single kernels of the product to plain references (no reference counterpart).
 *
 * Kept apart from lio_c.h, the ABI the drop-in classes and hosts link against: a library built against an earlier lio_c.h — an
 * oracle kept from an earlier revision of the test infrastructure — still provides all of it.  Both libraries export every symbol
 * declared here (tests/test_abi.py).  Plain C99. */
#ifndef LIO_TEST_HOOKS_H_
#define LIO_TEST_HOOKS_H_

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The lidar moments of frames pivot+1 .. pivot+Wo of the current window (after lio_est_build_local_map), at caller-given
 * T_{pivot<-i}, through the path the estimator is configured for.
 * Rt: n_passes x Wo x 12 (R row-major, t); out: n_passes x Wo x 258 (S 16x16 row-major, cost, count) with
 * S = sum_k rho'_k z_k z_k^T, z = [w (x) [p;1]; d] (13 values padded to 16), rho' = 1 / (1 + r^2), cost = 0.5 sum log(1 + r^2).
 * All passes run inside ONE solve scope, so with the resident form they are passes 1..n of one resident launch.  With factor sharding
 * the result is this rank's share, before any all-reduce.  path_out_or_null: 0 MFMA launch pair, 2 resident kernel (the oracle: -1;
 * 1, the VALU launch pair of earlier versions, is no longer returned).  The oracle forms the defining sums serially in fp64 over its
 * own feature slots.  LIO_ERR_STATE when the handle's feature slots live in a batch (its last solve ran in one): lio_est_build_local_map
 * first. */
int lio_est_eval_lidar_moments(lio_est *, int n_passes, const double *Rt, double *out, int *path_out_or_null);

/* Residuals per lane of the resident moments kernel (and the partition of the factor slots that goes with it) for the handle's later
 * solves and lio_est_eval_lidar_moments calls: 1, 2, 4 or 8 forces that count, 0 restores the rule that picks it per window.  Any
 * other value: LIO_ERR_ARG.  The oracle checks the argument and otherwise ignores it. */
int lio_est_force_moments_per_lane(lio_est *, int per_lane);

/* What stage 6 of lio_est_batch_stage_digest stands for, as numbers — the normal-equation moments of window `window` at the point its
 * last lio_est_batch_solve accepted (Wo x 258: S 16x16 row-major, cost, count) and the T_{pivot<-i} they were evaluated at (Rt: Wo x 12,
 * R row-major then t), read from the device state.  LIO_ERR_STATE when the window was not solved on the device.  Waits for the batch.
 * The oracle returns zeros. */
int lio_est_batch_get_moments(lio_est_batch *, int window, double *out, double *Rt);

#ifdef __cplusplus
}
#endif
#endif /* LIO_TEST_HOOKS_H_ */
