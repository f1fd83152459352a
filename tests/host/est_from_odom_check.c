/* include/lio_est_from_odom.h compiled by a C compiler (C99, not C++, not ctypes) and linked with the product: the argument checks that
 * need no device.  Built and run by tests/test_est_from_odom_abi.py; exit status 0, or the number of the check that failed. */
#include "lio_est_from_odom.h"

#include <stdio.h>
#include <string.h>

int main(void) {
  int marker = 0;
  lio_est_batch *some = (lio_est_batch *)&marker;   /* never dereferenced: an argument check refuses the call before */
  lio_odom *odom[2] = {NULL, NULL};
  lio_pp *pp[2] = {NULL, NULL};
  lio_transform_f T[2];
  lio_solve_report reps[2];
  double stamps[2] = {0.1, 0.2};
  int stats[8] = {7, 7, 7, 7, 7, 7, 7, 7};
  memset(T, 0, sizeof(T));
  memset(reps, 0, sizeof(reps));
  T[0].q[3] = 1.f; T[1].q[3] = 1.f; T[1].p[0] = 5.f;
  reps[0].iterations = 41; reps[1].iterations = 43;
  if (lio_est_batch_push_frames_from_odom(NULL, odom, pp, T, stamps) != LIO_ERR_ARG) return 1;             /* no batch */
  if (lio_est_batch_push_frames_from_odom(some, NULL, pp, T, stamps) != LIO_ERR_ARG) return 2;             /* no odometry array */
  if (lio_est_batch_push_frames_from_odom(some, odom, pp, T, NULL) != LIO_ERR_ARG) return 3;               /* no stamps */
  if (lio_est_batch_push_frames_from_odom(some, odom, NULL, NULL, stamps) != LIO_ERR_ARG) return 4;        /* no transforms */
  if (lio_est_batch_process_compact_from_odom(NULL, odom, pp, stamps, T, reps) != LIO_ERR_ARG) return 5;
  if (lio_est_batch_process_compact_from_odom(some, NULL, pp, stamps, T, reps) != LIO_ERR_ARG) return 6;
  if (lio_est_batch_process_compact_from_odom(some, odom, NULL, NULL, NULL, NULL) != LIO_ERR_ARG) return 7;
  if (lio_est_batch_process_compact_from_odom(NULL, odom, NULL, stamps, NULL, NULL) != LIO_ERR_ARG) return 8;
  if (lio_est_batch_from_odom_stats(NULL, stats) != LIO_ERR_ARG) return 9;
  if (lio_est_batch_from_odom_stats(some, NULL) != LIO_ERR_ARG) return 10;
  if (reps[0].iterations != 41 || reps[1].iterations != 43 || stats[0] != 7 || stats[7] != 7 || T[1].p[0] != 5.f) return 11;   /* outputs untouched */
  printf("%s %d\n", lio_backend(), (int)(sizeof(stats) / sizeof(stats[0])));
  return 0;
}
