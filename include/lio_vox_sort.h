/* lio_vox_sort.h — a witness and a door for tests into the voxel filter's sort.
 *
 * include/lio_c.h is the ABI that the product (liblio_hip.so) and the CPU oracle both implement.  The calls below exist in the product
 * only, like those of lio_ext.h; the oracle does not implement them.  Plain C99.
 *
 * The filter behind lio_voxel_grid, Estimator::PushFrame and Estimator::BuildLocalMap sorts (voxel key, point index) pairs between its key
 * pass and its centroid pass (docs/voxel_sort.md).  Which sort runs is a pure function of the number of points:
 *   LIO_VOX_SORT_SAMPLE    a sample sort in three launches: splitters, bucket scatter, bucket sort + compaction
 *   LIO_VOX_SORT_SINGLE    one launch sorts the keys directly, by rank, splitters and scatter skipped (n <= LIO_VOX_SORT_SINGLE_MAX)
 *   LIO_VOX_SORT_LIBRARY   the library's radix sort: a bucket of the sample sort was full and the run was redone, or n > LIO_VOX_SORT_SAMPLE_MAX
 * The values are the points' own indices, so every path gives the stable sort by key, bit for bit.
 */
#ifndef LIO_VOX_SORT_H
#define LIO_VOX_SORT_H

#include "lio_c.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIO_VOX_SORT_SAMPLE 0
#define LIO_VOX_SORT_SINGLE 1
#define LIO_VOX_SORT_LIBRARY 2

/* The sizing rule of the sample sort, for n keys with LIO_VOX_SORT_SINGLE_MAX < n <= LIO_VOX_SORT_SAMPLE_MAX:
 *   buckets  NB = ceil(n / LIO_VOX_SORT_MEAN_BUCKET), each with room for LIO_VOX_SORT_BUCKET_CAP pairs
 *   sample   S = LIO_VOX_SORT_OVERSAMPLE * NB keys, taken at the positions floor((j + 0.5) * n / S), j = 0 .. S - 1
 *   splitter b (b = 1 .. NB - 1) = the sorted sample's entry LIO_VOX_SORT_OVERSAMPLE * b; a key's bucket = the number of splitters <= key */
#define LIO_VOX_SORT_SINGLE_MAX 4096
#define LIO_VOX_SORT_BUCKET_CAP 4096
#define LIO_VOX_SORT_MEAN_BUCKET 384
#define LIO_VOX_SORT_OVERSAMPLE 8
#define LIO_VOX_SORT_SAMPLE_MAX (1024 * 384)

/* Sorts n caller-given keys with values 0 .. n - 1 through exactly the code the filter runs between its key pass and its tile-heads pass,
 * the redo through the library included.  keys_out / vals_out: n entries each, the stable sort by key.  path_out (may be null): the
 * LIO_VOX_SORT_* path that produced the result.  LIO_ERR_ARG: a null array or n == 0. */
int lio_vox_sort_pairs(const uint32_t *keys, size_t n, uint32_t *keys_out, uint32_t *vals_out, int *path_out);

/* Counters of the scratch filter behind lio_voxel_grid on the calling thread, in LIO_VOX_SORT_* order: filter runs whose result came from
 * the sample sort, from the direct one-launch sort, and from the library's sort.  lio_vox_sort_pairs does not count. */
int lio_vox_sort_stats(uint64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
