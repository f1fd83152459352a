/* lio_seg_bounds.h — a door for tests into the bounds pass that the sensor chains share.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The call below exists in the product
 * only, like those of lio_ext.h; the oracle does not implement it.  Plain C99.
 *
 * The scan-to-scan odometry and the scan-to-map step ask for the bounds of all their clouds in one pass (two launches over a table of
 * clouds), and the voxel filter's exact path runs the same per-block code on its one cloud.  The chains clamp a point outside its grid
 * into the border cells, so a wrong bound would cost speed or neighbours, not fail: this call hands the pass's own results out.
 */
#ifndef LIO_SEG_BOUNDS_H
#define LIO_SEG_BOUNDS_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the pass leaves per cloud, for the points that are finite in x, y and z: their minimum and maximum, the cell bounds
 * minb = floor(mn * inv_leaf) and divb = floor(mx * inv_leaf) - minb + 1 of pcl::VoxelGrid, its "leaf size too small" guard
 * (the product over the axes of (int64)((mx - mn) * inv_leaf) + 1 exceeds INT32_MAX) and the number of such points.  A cloud
 * without such a point has n_valid = 0 and nothing else defined. */
typedef struct lio_seg_bounds_out {
  float mn[3], mx[3];
  int32_t minb[3], divb[3];
  int32_t overflow;
  int32_t n_valid;
} lio_seg_bounds_out;

/* Uploads the nseg clouds (xyzi[k]: n[k] points of x y z i; may be null where n[k] == 0) and runs the pass ONCE over all of them, as
 * the chains launch it.  out: nseg entries.  LIO_ERR_ARG: a null array, nseg < 1, a null cloud with a count, inv_leaf not positive;
 * LIO_ERR_CAPACITY: a cloud of 2^31 points or more. */
int lio_seg_bounds(const float *const *xyzi, const size_t *n, int nseg, float inv_leaf, lio_seg_bounds_out *out);

#ifdef __cplusplus
}
#endif
#endif
