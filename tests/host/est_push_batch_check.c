/* include/lio_est_push_batch.h compiled by a C compiler (C99, not C++, not ctypes) and linked with the product: the argument checks that
 * need no device.  Built and run by tests/test_est_push_batch_abi.py; exit status 0, or the number of the check that failed. */
#include "lio_est_push_batch.h"

#include <stdio.h>
#include <string.h>

int main(void) {
  int marker = 0;
  lio_est_batch *some = (lio_est_batch *)&marker;   /* never dereferenced: an argument check refuses the call before */
  lio_est_frame frames[2];
  lio_solve_report reps[2];
  int stats[8] = {7, 7, 7, 7, 7, 7, 7, 7};
  memset(frames, 0, sizeof(frames));
  memset(reps, 0, sizeof(reps));
  frames[0].transform_in.q[3] = 1.f; frames[1].transform_in.q[3] = 1.f;
  reps[0].iterations = 41; reps[1].iterations = 43;
  if (lio_est_batch_push_frames(NULL, frames) != LIO_ERR_ARG) return 1;                  /* no batch */
  if (lio_est_batch_push_frames(some, NULL) != LIO_ERR_ARG) return 2;                    /* no frames */
  if (lio_est_batch_slide_windows(NULL) != LIO_ERR_ARG) return 3;
  if (lio_est_batch_process_laser_odom(NULL, frames, reps) != LIO_ERR_ARG) return 4;
  if (lio_est_batch_process_laser_odom(some, NULL, reps) != LIO_ERR_ARG) return 5;
  if (lio_est_batch_process_laser_odom(NULL, frames, NULL) != LIO_ERR_ARG) return 6;
  if (lio_est_batch_push_stats(NULL, stats) != LIO_ERR_ARG) return 7;
  if (lio_est_batch_push_stats(some, NULL) != LIO_ERR_ARG) return 8;
  if (reps[0].iterations != 41 || reps[1].iterations != 43 || stats[0] != 7 || stats[7] != 7) return 9;   /* outputs untouched */
  if (sizeof(frames[0].n_surf) != sizeof(size_t) || sizeof(frames[0].stamp) != sizeof(double)) return 10;
  printf("%s %d\n", lio_backend(), (int)sizeof(lio_est_frame));
  return 0;
}
