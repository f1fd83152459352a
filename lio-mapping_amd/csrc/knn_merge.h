// knn_merge.h — merging two ascending five-entry K-NN lists by a fixed network, for the host and for the HIP kernels.
//
// An entry is (key, j): the 64-bit key of knn_key (cloud_device.h: the squared distance's bit pattern above the point's original index) and
// the point's position in the cell-sorted map.  A list is ascending by key and padded with the sentinel (key of (INFINITY, INT_MAX), j = 0).
//
// Why a merge may replace the insertions it stands for, bit for bit: the lists that meet here are disjoint (every candidate of a query is
// seen by exactly one sub-lane, once), the order on real keys is strict (original indices are distinct), and sentinels are equal to one
// another in key AND position.  So the five smallest of the union and their order are unique: every correct merge returns the same keys and
// positions as pushing the other list's entries one by one through knn_insert (docs/knn_merge.md).
//
// No device intrinsics here: tests/host/knn_merge_check.cc compiles this file with a host compiler and holds it to std::sort exhaustively.
#pragma once
#include "hmath.h"

namespace lio {

// compare-exchange: afterwards (ka, ja) <= (kb, jb) by key; equal keys stay where they are
LIO_HD void knn_cx(unsigned long long &ka, int &ja, unsigned long long &kb, int &jb) {
  const bool sw = kb < ka;
  const unsigned long long tk = sw ? ka : kb;
  const int tj = sw ? ja : jb;
  ka = sw ? kb : ka;
  ja = sw ? jb : ja;
  kb = tk; jb = tj;
}

// Sorts a BITONIC five (ascending, then descending; either part may be empty) ascending in five compare-exchanges: the bitonic merge network
// of eight entries whose first three are "minus infinity" — of its twelve comparators the seven that touch such an entry do nothing.
// (An arbitrary five would need nine.)  knn_merge5's selects produce exactly such a five.
LIO_HD void knn_sort5(unsigned long long (&k)[5], int (&j)[5]) {
  knn_cx(k[0], j[0], k[4], j[4]);
  knn_cx(k[1], j[1], k[3], j[3]);
  knn_cx(k[2], j[2], k[4], j[4]);
  knn_cx(k[1], j[1], k[2], j[2]);
  knn_cx(k[3], j[3], k[4], j[4]);
}

// (bk, bj) <- the five smallest of the ascending fives (bk, bj) and (ok, oj), ascending.  min(b[k], o[4 - k]), k = 0..4, ARE the five smallest
// of the ten (of b[0..k] and o[0..4-k], six entries, at most five can be among them, so one of b[k], o[4 - k] is not; the smaller of the two
// is, or neither), and they form a bitonic five: ascending while b[k] is the smaller, descending from where o[4 - k] takes over.
LIO_HD void knn_merge5(unsigned long long (&bk)[5], int (&bj)[5], const unsigned long long (&ok)[5], const int (&oj)[5]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 5; ++k) {
    const bool o = ok[4 - k] < bk[k];
    bk[k] = o ? ok[4 - k] : bk[k];
    bj[k] = o ? oj[4 - k] : bj[k];
  }
  knn_sort5(bk, bj);
}

// (bk, bj) <- the five smallest of the ascending five (bk, bj) and FOUR entries (ck, cj) in any order, ascending: the four are sorted by the
// five-comparator network, then merged as above with the sentinel as the fifth — min(b[0], sentinel) is b[0], so that select is not made.
// An entry that must not enter carries a key at or above the sentinel's (a distance that is NaN gives one above it): it sorts behind the
// real ones and no select takes it, because b[k] never exceeds the sentinel.  ck, cj are used up.
LIO_HD void knn_merge4(unsigned long long (&bk)[5], int (&bj)[5], unsigned long long (&ck)[4], int (&cj)[4]) {
  knn_cx(ck[0], cj[0], ck[1], cj[1]);
  knn_cx(ck[2], cj[2], ck[3], cj[3]);
  knn_cx(ck[0], cj[0], ck[2], cj[2]);
  knn_cx(ck[1], cj[1], ck[3], cj[3]);
  knn_cx(ck[1], cj[1], ck[2], cj[2]);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 1; k < 5; ++k) {
    const bool o = ck[4 - k] < bk[k];
    bk[k] = o ? ck[4 - k] : bk[k];
    bj[k] = o ? cj[4 - k] : bj[k];
  }
  knn_sort5(bk, bj);
}

}  // namespace lio
