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

/* The five-nearest-neighbour walk every lidar residual of the product starts from (csrc/cloud_device.h: knn_scan_group<5, LPQ>, the body
 * CalculateFeatures, CalculateLaserOdom, the batched windows, scan-to-map and the keyframe batch all call), on its own.
 * Product: uploads map and queries (xyzi, 4 floats per point), builds the cell grid over the map's own bounds with cell size `cell`
 * (lio_knn's grid at cell = sqrt(radius_sq) * 1.0001f + 1e-6f) and runs the walk in one launch of 256-thread blocks with
 * LPQ = lanes_per_query lanes per query: 1, 4 or 8, the forms the product launches; any other value is LIO_ERR_ARG, as are a null
 * pointer and a cell that is not a positive finite number.
 * The WHOLE list comes back, with no radius cut (the product cuts later, in the plane fit):
 *   idx_out[m * 5]          original map indices, ascending by (squared distance, index); a missing entry is -1
 *   sqd_out[m * 5]          the fp32 squared distances (d = dx*dx; d += dy*dy; d += dz*dz); a missing entry is +inf
 *   nbr_xyz_out[m * 5 * 3]  the coordinates the walk's POSITIONS in the cell-sorted map point at (what the plane fit would load);
 *                           a missing entry is zeros
 * What is searched: with c(v) = int(floorf(v * (1.0f / cell))) in fp32 per axis, the grid spans cells c(min) - 1 .. c(max) + 1 of the
 * map's finite bounds (an empty map: bounds 0); a query whose cell lies in the grid sees every map point whose cell is within +-1 of
 * its own on every axis; a query outside the grid, or with a NaN / inf coordinate, finds nothing (all -1 / +inf / zeros) and does
 * not disturb the other queries of its wave.  Map points are expected finite.
 * The oracle states the same contract as a serial loop over cells; it checks lanes_per_query and otherwise ignores it. */
int lio_knn_walk(const float *map_xyzi, size_t n_map, const float *query_xyzi, size_t m, float cell, int lanes_per_query,
                 int32_t *idx_out, float *sqd_out, float *nbr_xyz_out);

/* The fit that turns a query's five neighbours into a residual's coefficients and decides whether the residual exists, on
 * caller-given neighbours (csrc/cloud_device.h: features_fit<MAPPING>, the body CalculateFeatures, CalculateLaserOdom, the batched
 * windows, scan-to-map, MapBuilder and the keyframe batch call; csrc/cloud_kernels.hip: line_features_fit, the corner branch of
 * scan-to-map and of the keyframe batch).
 *   form             0 plane fit of the estimator; 1 plane fit of PointMapping (sign follows pd2); 2 plane fit of MapBuilder (fitted
 *                    sign kept); 3 line fit.  Any other value: LIO_ERR_ARG, as is a null pointer.
 *   nbr_xyz[m*5*3]   the five neighbours of every query, in the order the walk returns them
 *   fifth_sqd[m]     what the walk reports as the fifth squared distance; +inf stands for "fewer than five found"
 *   stack_xyzi[m*4]  the queries in the sensor frame; the fit sees sel = rotate(T.q, p) + T.p
 *   fixed_pz[3]      the FOV apex point of forms 1 - 3 (form 0 uses rotate(T.q, (0, 0, 10)) + T.p and ignores it)
 * Out, m entries each: valid, coeff (4 floats), score (forms 1 - 3: 0), abs_coeff (4 floats; forms 0 and 3: 0).  An invalid query
 * returns zeros in all of them.  m == 0 is fine.
 * Product: uploads, then ONE launch with a query per lane that calls the same device functions the production kernels call, with the
 * uploaded neighbours as the map and positions 5 i .. 5 i + 4.  Oracle: the fit functions its own loops call, serially. */
int lio_fit_five(int form, const float *nbr_xyz, const float *fifth_sqd, const float *stack_xyzi, size_t m, const lio_transform_f *T,
                 const float *fixed_pz, float min_match_sq_dis, float min_plane_dis, uint8_t *valid, float *coeff, float *score,
                 float *abs_coeff);

/* The correspondence search every scan-to-scan residual starts from (csrc/odometry.hip: k_ob_corr, one wave per query, launched by
 * PointOdometry's Process at every fifth iteration), on its own and stateless: PointOdometry.cc:237-259 (TransformToStart), :342-385
 * (corner: closest and second), :440-494 (surf: closest, second and third).  Clouds are xyzi, intensity = ring + relative time.
 *   sel      TransformToStart of the query at transform_es: s = (1 / scan_period) * (intensity - int(intensity)), 0 with no_deskew;
 *            a query with s < 0 or s > 1.001 passes through unchanged (and is searched for as it stands); otherwise
 *            sel = conj(slerp(identity, s, q_es)) * (p - s t_es), the conjugate not normalised.
 *   closest  the point of the previous cloud (last_corner for a sharp query, last_surf for a flat one) with the smallest fp32 squared
 *            distance to sel (d = dx*dx; d += dy*dy; d += dz*dz); among equal distances the lower index; accepted only if d < 25.
 *   window   with cs = int(intensity[closest]): j = closest + 1 .. upward until the first j with int(intensity[j]) > cs + 2.5 — nothing
 *            at or behind that j is seen —, then j = closest - 1 .. 0 downward until the first int(intensity[j]) < cs - 2.5.
 *   corner   second: upward candidates of ring > cs, downward candidates of ring < cs.
 *   surf     second: upward ring <= cs, downward ring >= cs;  third: upward ring > cs, downward ring < cs.
 *   a slot takes its candidate with the smallest distance below 25; among equal distances the first in walk order: any upward
 *   candidate before any downward one, nearer to closest first.  A missing entry is -1; without closest all entries are -1.
 * corner_idx: n_sharp x 2 (closest, second); surf_idx: n_flat x 3 (closest, second, third); sel_out: (n_sharp + n_flat) x 3, sharp first.
 * The intensity of a query enters through s alone.  A query with a NaN or infinite coordinate, or (unless no_deskew) a NaN intensity,
 * has no finite sel: it finds nothing (all -1; its sel_out row is not specified) and does not disturb the other queries.  An infinite
 * intensity is a time ratio outside [0, 1.001] like any other (the query passes through); with no_deskew s = 0 whatever the intensity.
 * The previous clouds are expected finite.  Empty previous clouds give all -1; n_sharp == n_flat == 0 is fine.  A null required pointer
 * (a cloud pointer may be null when its count is 0) or a scan_period that is not positive and finite: LIO_ERR_ARG.  The > 10 / > 100
 * size gate of Process (:335) is not applied.
 * Product: uploads the clouds into a device object of its own, fills the one-sensor table and builds the two 5 m grids with the steps
 * Process runs (OdoChain::FillTable, OdoChain::MakeGrids), launches k_ob_corr ONCE over that table, and fills sel_out from a separate
 * one-query-per-lane kernel that calls the same odo_to_start.  Oracle: the functions its own Process loop calls, serially. */
int lio_odom_correspondences(const float *sharp_xyzi, size_t n_sharp, const float *flat_xyzi, size_t n_flat,
                             const float *last_corner_xyzi, size_t n_last_corner, const float *last_surf_xyzi, size_t n_last_surf,
                             const lio_transform_f *transform_es, float scan_period, int no_deskew,
                             int32_t *corner_idx /* n_sharp x 2 */, int32_t *surf_idx /* n_flat x 3 */,
                             float *sel_out /* (n_sharp + n_flat) x 3, sharp first */);

/* ---- The 6x6 Gauss-Newton loops from the rows onward.  Every pose of the product passes through one of three loops — scan-to-scan
 * odometry (csrc/odometry.hip: k_ob_rows, k_ob_update, for one sensor and for a batch), scan-to-map and the keyframe batch
 * (csrc/cloud_kernels.hip: k_kf_rows with k_kf_update, over a batch of keyframes or the map handle's table of one) and the estimator's newest-frame loop (k_odom_round,
 * k_odom_update_wide, and k_bw_odom_round / k_bw_odom_update of the batched windows) — and all of them form fp32 rows (A | b) per selected
 * residual, add a_i a_j, a_i b and a count into 28 fp64 sums through a chain of folds, and run one serial step on the sums.  The sums
 * are laid out as the upper triangle of A^T A row by row (21), A^T b (6), the row count (1). */

/* The state a step works on: csrc/cloud_kernels.h OdomState, word for word. */
typedef struct {
  float T[8];          /* qx qy qz qw px py pz, and a pad; the scan-to-scan step (family 1) leaves float(rows selected) in the pad */
  int32_t converged;   /* set by the abort test; never cleared */
  int32_t iters;       /* iter + 1 after every step, also after one that had too few rows */
  int32_t degenerate;  /* kz > 0, decided at iter 0 and carried */
  int32_t kz;          /* eigenvalues of A^T A below the family's threshold at iter 0: the leading kz components of the step are masked */
  int32_t nsel;        /* rows selected: int(sums[27]) */
} lio_gn_state;

/* The rows of the scan-to-map family (csrc/cloud_device.h: odom_row_form, the function odom_row_accumulate — k_kf_rows,
 * k_odom_round and the batched windows — forms every row with) and the partials of ONE production rows launch.
 *   form            the production `b_from_coef`: 0 estimator (b = -(w . (R p + t) + c.w)), 1 scan-to-map (b = -c.w), 2 MapBuilder
 *                   (b = -c.w and the rotation columns times R^-1 diag(5e-3, 5e-3, 1)).  Any other value: LIO_ERR_ARG.
 *   stack_xyzi      m queries in the sensor frame (intensity unused); valid[m]; coeff[m * 4] = (w, c.w) as a fit returns them
 *   T               the pose the rows are formed at; a non-finite component is LIO_ERR_ARG
 *   ok_out[m]       1 where a row exists: valid != 0
 *   rows_out[m * 7] a0 .. a5, b in fp32; zeros where ok is 0.  a = (-(w^T R skew(p)) [form 2: R^-1 diag(5e-3, 5e-3, 1)], w)
 *   nb_out          odom_rows_blocks(m), the block count production launches with
 *   partials_out    nb x 28 doubles; nb never exceeds 256, and the caller provides 256 x 28 (m == 0: one row of zeros)
 * Product: ONE launch through launch_kf_rows over a table of one record with the production block count; rows_out comes from a separate one-query-per-lane
 * kernel that calls the same odom_row_form.  Oracle: the row function its own loops (Estimator::CalculateLaserOdom,
 * PointMapping::OptimizeTransformTobeMapped) call, serially; nb_out = 1 and its partial is one row of plain fp64 sums of the fp32
 * products.  A null required pointer (an input may be null when m is 0): LIO_ERR_ARG. */
int lio_gn_rows_map(int form, const float *stack_xyzi, size_t m, const uint8_t *valid, const float *coeff, const lio_transform_f *T,
                    uint8_t *ok_out, float *rows_out, int32_t *nb_out, double *partials_out);

/* The rows of the scan-to-scan loop (csrc/odometry.hip: odo_row_coeff and odo_row_of, the two functions k_ob_rows forms every row
 * with) and the partials of ONE production rows launch, on caller-given clouds and correspondences: PointOdometry.cc:391-435 (edge
 * coefficients), :497-531 (plane coefficients), A.7 (the weight s, 1 before iteration 5), :548-571 (the row).  Clouds, transform_es,
 * scan_period and no_deskew as in lio_odom_correspondences; corner_idx (n_sharp x 2) and surf_idx (n_flat x 3) as it returns them or as
 * the caller states them.
 *   a sharp query has a row when its second index is >= 0, s > 0.1 and the distance ld2 != 0; a flat query when its second and third
 *   are >= 0, s > 0.1 and pd2 != 0 (a collinear triple gives a non-finite pd2, which passes `!= 0`, and a non-finite row: the
 *   behaviour of the reference program, kept)
 *   ok_out[n_sharp + n_flat], rows_out[(n_sharp + n_flat) * 7] (r0 .. r5, b; zeros where ok is 0), sharp first
 *   nb_out = max(1, min(ceil(nq / 256), 64)), partials_out nb x 28 doubles; the caller provides 64 x 28
 * An index outside [-1, size of its cloud), a second or third index without a closest one (the search never returns that, and the rows
 * read the closest point whenever the others exist; so -1 in the closest slot is a case only together with -1 in the others, never on
 * its own), a null required pointer, a non-finite transform, a scan_period that is not positive
 * and finite, or a negative iter: LIO_ERR_ARG.
 * Product: uploads into a device object of its own, launches k_ob_rows ONCE over the one-sensor table Process fills; rows_out comes from a
 * separate one-query-per-lane kernel that calls the same two functions.  Oracle: the functions its own Process loop calls, serially;
 * nb_out = 1 and one partial of plain fp64 sums of the fp32 products. */
int lio_gn_rows_odom(const float *sharp_xyzi, size_t n_sharp, const float *flat_xyzi, size_t n_flat, const float *last_corner_xyzi,
                     size_t n_last_corner, const float *last_surf_xyzi, size_t n_last_surf, const int32_t *corner_idx, const int32_t *surf_idx,
                     const lio_transform_f *transform_es, float scan_period, int no_deskew, int iter, uint8_t *ok_out, float *rows_out,
                     int32_t *nb_out, double *partials_out);

/* The fixed-order fold of `nblocks` partials (28 doubles each) into sums_out[28].
 *   wide 0   reduce_partials28 (csrc/cloud_kernels.h) on a 256-thread block: k_kf_update, k_ob_update
 *   wide 1   fold_partials28_wide (csrc/cloud_device.h) on a 1024-thread block: k_odom_update_wide, k_bw_odom_update
 * One launch that calls the production function and copies the 28 shared sums out.  nblocks == 0 gives zeros.  The oracle adds the rows
 * serially, ascending.  A null pointer (partials may be null when nblocks is 0), a negative nblocks or another `wide`: LIO_ERR_ARG. */
int lio_gn_fold(const double *partials, int nblocks, int wide, double *sums_out);

/* The serial step behind the sums: fp32 A^T A, A^T b <- sums; qr_solve<float, 6, 6>; at iter 0 kz = count_eigs_below(threshold) and
 * degenerate = kz > 0; the leading kz components of X masked; t += X[3..5], q = q * deltaQ(X[0..2]) (left_update: deltaQ * q); a
 * non-finite t component resets to 0; converged when the rotation in degrees and 100 |X[3..5]| are both below the abort value.
 *   family 0   odom_update_from_sums (csrc/cloud_device.h): threshold 100, abort at 0.05; a step with min_rows > 0 and fewer rows leaves
 *              T untouched and sets nsel and iters alone
 *   family 1   odo_update_step (csrc/odometry.hip): threshold 10, abort at 0.1, fewer than 10 rows leave T untouched; min_rows and
 *              left_update must be 0; T[7] = float(rows), which the hook also reports in nsel
 * Product: one launch, thread 0 calls the production function on a copy of state_in.  Oracle: the statements after the sums of its
 * own loops (GaussNewtonStep, oracle/liomath.h), which accumulate in fp32 and so take float(sums).  Null pointers, another family, a
 * negative iter or min_rows, or a non-finite state_in->T[0..6]: LIO_ERR_ARG (non-finite SUMS are a case, not an error). */
int lio_gn_step(int family, const double *sums, const lio_gn_state *state_in, int iter, int min_rows, int left_update,
                lio_gn_state *state_out);

/* Round 0, keep 0, of the estimator's newest-frame loop through launch_odom_round: search + fit + rows per block (k_odom_round<4> or
 * <8>) and fold + step (k_odom_update_wide).  The grid is built over the map as lio_calculate_features builds it.
 *   lanes_per_query   4 or 8 (what the product launches); anything else is LIO_ERR_ARG
 *   nb_out            odom_round_blocks(m, lanes_per_query) = max(1, ceil(m * lanes_per_query / 256)); partials_out holds nb x 28
 *                     doubles, and the caller provides that many
 *   state_out         the state after k_odom_update_wide, started from T with every other word zero
 * The oracle runs one pass of its own loop body (CalculateFeatures, rows, GaussNewtonStep): nb_out = 1, one partial.  m == 0 launches
 * nothing: state_out is the initial state and nb_out = 0.  Rounds with kept features (keep = 1, round > 0) are covered end to end only
 * (tests/test_gpu_parity.py).  Null required pointers, a non-finite T or thresholds that are not positive and finite: LIO_ERR_ARG. */
int lio_gn_round(const float *map_xyzi, size_t n_map, const float *stack_xyzi, size_t m, const lio_transform_f *T, float min_match_sq_dis,
                 float min_plane_dis, int lanes_per_query, int32_t *nb_out, double *partials_out, lio_gn_state *state_out);

/* ---- The device-resident trust-region loop (csrc/solve_step.h: k_bw_aux, k_bw_solve_step), stopped early and read out as numbers. */

/* n >= 0 replaces lio_est_config.max_num_iterations for the handle's later solves (read at every solve: the packed problem and the
 * length of the batch's launch chain); a negative n is LIO_ERR_ARG.  n = 0 stops the device loop behind its first linearisation, n = 1
 * behind the decision on its first candidate.  The oracle applies it to its own loop. */
int lio_est_set_max_num_iterations(lio_est *, int n);

/* What the last lio_est_batch_solve left on the device for window `window`: the problem the kernels read, the loop's state and the aux
 * row of the last launch A that ran for the window (evaluated at `cand`).  Waits for the batch.  LIO_ERR_STATE when the window was not
 * solved on the device; a null pointer or a window outside the batch is LIO_ERR_ARG.  The oracle returns zeros.  Every array has a
 * fixed size (the LIO_DSL_* counts below); entries beyond what the window uses are zero.  F = 8 frames, the most a window optimises + 1.
 *   ints     [0] Wo [1] n [2] ex_col [3] n_prior [4] have_prior [5] use_ex_prior [6] n_keep [7] it [8] successful [9] termination
 *            [10] need_host [11] ntrace [12] n_pad [13] started [14] done [15] max_iterations
 *            [16, 144)   prior_col[128]: tangent column of H -> column of the prior, -1: none
 *            [144, 194)  the kept blocks of the prior, 10 x (kind: 0 pose 1 speed-bias 2 extrinsic, index, size, offset in the prior's
 *                        tangent vector, offset in x0)
 *            [194, 201)  present[7] of the IMU factors
 *   problem  [0, 90) x0 of the kept blocks  [90, 93) ex_prior_pos  [93, 97) ex_prior_rot (w, x, y, z)
 *            [97 + 470 i, ..) IMU factor i < 7: dp 3 | dq 4 (w, x, y, z) | dv 3 | ba 3 | bg 3 | g 3 | sum_dt | jac 225 | sqrt_info 225
 *            [3387, ..) the prior the solve READ, np = n_prior: JtJ np x np | lin_jac np x np | lin_res np | Jtr0 np
 *   state    a parameter set is pose F x 7 (p, q as x y z w) | speed-bias F x 9 | extrinsic 7 = 135 doubles
 *            [0, 135) x, the accepted point  [135, 270) cand  [270, 354) cand_Rt 7 x 12 (R row-major, t)
 *            [354, 482) scale  [482, 610) g (scaled)  [610, 614) costs0 (marg, pim, ppp, extrinsic prior)  [614, 654) trace
 *            [654, 664) radius, mu, alpha, dogleg_norm, model_change, step_norm, x_cost, x_norm, gmax, n_lidar
 *            [664, 664 + n n) Hcur, the scaled H at x: the stored upper triangle mirrored into a full row-major n x n
 *   aux      [0, 6524) imu_out 7 x 932 (J^T J 30 x 30 | J^T r 30 | cost | present)  [6524, 8260) lmap 7 x 248 (L 18 x 13 | l 13 | pad)
 *            [8260, 8341) prior_out (J^T r np | cost)  [8341, 8385) exprior_out (J^T J 6 x 6 | J^T r 6 | cost | pad)
 *            [8385, 10191) the lidar moments the last launch B folded, at cand, 7 x 258 (S 16 x 16 row-major, cost, count): the slot
 *                        of lio_est_batch_get_moments when x equals cand (first linearisation, accepted step), the other one otherwise */
#define LIO_DSL_INTS 208
#define LIO_DSL_PROBLEM (3387 + 2 * 80 * 80 + 2 * 80)
#define LIO_DSL_STATE (664 + 128 * 128)
#define LIO_DSL_AUX 10191
int lio_est_batch_get_linearization(lio_est_batch *, int window, int32_t *ints, double *problem, double *state, double *aux);

#ifdef __cplusplus
}
#endif
#endif /* LIO_TEST_HOOKS_H_ */
