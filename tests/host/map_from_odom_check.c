/* include/lio_map_from_odom.h compiled by a C compiler (C99, not C++, not ctypes) and linked with the product: the argument checks that
 * need no device.  Built and run by tests/test_map_from_odom_abi.py; exit status 0, or the number of the check that failed. */
#include "lio_map_from_odom.h"

#include <stdio.h>

int main(void) {
  lio_map *no_map[2] = {NULL, NULL};
  lio_odom *no_odom[2] = {NULL, NULL};
  lio_pp *no_pp[2] = {NULL, NULL};
  int marker = 0;
  lio_map *some_map[2] = {(lio_map *)&marker, NULL};     /* never dereferenced: an argument check refuses the call before */
  lio_odom *some_odom[2] = {(lio_odom *)&marker, NULL};
  lio_transform_f T[2];
  int32_t it[2] = {7, 7}, sel[2] = {9, 9};
  T[0].p[0] = 4.5f; T[1].q[3] = 2.5f;
  if (lio_map_process_batch_from_odom(NULL, no_odom, no_pp, 2, T, it, sel) != LIO_ERR_ARG) return 1;        /* no handle array */
  if (lio_map_process_batch_from_odom(no_map, NULL, no_pp, 2, T, it, sel) != LIO_ERR_ARG) return 2;         /* no odometry array */
  if (lio_map_process_batch_from_odom(no_map, no_odom, no_pp, 0, T, it, sel) != LIO_ERR_ARG) return 3;      /* n_sensors < 1 */
  if (lio_map_process_batch_from_odom(no_map, no_odom, NULL, -3, T, it, sel) != LIO_ERR_ARG) return 4;
  if (lio_map_process_batch_from_odom(no_map, no_odom, no_pp, 2, T, it, sel) != LIO_ERR_ARG) return 5;      /* null entries */
  if (lio_map_process_batch_from_odom(some_map, no_odom, NULL, 1, T, it, sel) != LIO_ERR_ARG) return 6;     /* a null odometry */
  if (lio_map_process_batch_from_odom(no_map, some_odom, NULL, 1, T, it, sel) != LIO_ERR_ARG) return 7;     /* a null map */
  if (lio_map_process_batch_from_odom(some_map, some_odom, no_pp, 2, T, it, sel) != LIO_ERR_ARG) return 8;  /* the second entries are null */
  if (lio_map_process_batch_from_odom(no_map, no_odom, NULL, LIO_MAP_BATCH_MAX_SENSORS + 1, NULL, NULL, NULL) != LIO_ERR_CAPACITY) return 9;
  if (it[0] != 7 || it[1] != 7 || sel[0] != 9 || sel[1] != 9 || T[0].p[0] != 4.5f || T[1].q[3] != 2.5f) return 10;   /* outputs untouched */
  printf("%s %d\n", lio_backend(), LIO_MAP_BATCH_MAX_SENSORS);
  return 0;
}
