// knn_merge_check — csrc/knn_merge.h compiled for the host and held to std::sort, exhaustively (tests/test_knn_merge.py).
//
// A network of compare-exchanges and selects that is right for every ORDER PATTERN of its inputs is right for all inputs (it only
// compares), so: for every (na, nb) real entries in 0..5 of the two lists, every way to deal na + nb ranked keys out to them (at most
// C(10, 5) = 252), the lists padded with sentinels, under three key maps — distinct distances with indices running against them, ONE
// distance for all (the index alone decides), distances shared by pairs.  knn_merge5 must return the first five of std::sort over the
// union, keys and positions.  knn_merge4 (four unsorted candidates, among them "no candidate" slots and keys above the sentinel's) the
// same, for every dealing AND every arrangement of the four slots.
//
// usage: knn_merge_check            -> prints the number of cases checked, exit status 1 and the first failures on stderr if any differ
//        knn_merge_check planted    -> the same checks against a knn_merge5 whose network lacks its last comparator and a knn_merge4 that
//                                      does not sort the four: prints how many cases noticed (the test expects both to be non-zero)
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "knn_merge.h"

using lio::knn_cx;
typedef unsigned long long u64;
typedef std::pair<u64, int> Entry;   // (key, position)

static u64 key_of(float d, int idx) {
  uint32_t b;
  std::memcpy(&b, &d, 4);
  return (u64(b) << 32) | uint32_t(idx);
}
static const u64 SENT = (u64(0x7F800000u) << 32) | uint32_t(INT_MAX);   // knn_key(INFINITY, INT_MAX)
static const u64 NANKEY = (u64(0x7FC00000u) << 32) | 7u;               // a NaN distance: above the sentinel

// rank r (0 = smallest) of n under key map `km` -> key; the keys ascend strictly with r under all three
static u64 ranked_key(int km, int r, int n) {
  if (km == 0) return key_of(0.25f * float(r + 1), 1000 + (n - r));   // distinct distances, indices descending
  if (km == 1) return key_of(1.5f, 10 + r);                            // one distance
  return key_of(0.5f * float(r / 2 + 1), 20 + r);                      // distances shared by pairs
}

struct Merge5 { void operator()(u64 (&bk)[5], int (&bj)[5], const u64 (&ok)[5], const int (&oj)[5]) const { lio::knn_merge5(bk, bj, ok, oj); } };
struct Merge4 { void operator()(u64 (&bk)[5], int (&bj)[5], u64 (&ck)[4], int (&cj)[4]) const { lio::knn_merge4(bk, bj, ck, cj); } };
// planted errors
struct Merge5Short {
  void operator()(u64 (&k)[5], int (&j)[5], const u64 (&ok)[5], const int (&oj)[5]) const {
    for (int i = 0; i < 5; ++i) if (ok[4 - i] < k[i]) { k[i] = ok[4 - i]; j[i] = oj[4 - i]; }
    knn_cx(k[0], j[0], k[4], j[4]); knn_cx(k[1], j[1], k[3], j[3]); knn_cx(k[2], j[2], k[4], j[4]); knn_cx(k[1], j[1], k[2], j[2]);
  }
};
struct Merge4Unsorted {
  void operator()(u64 (&bk)[5], int (&bj)[5], u64 (&ck)[4], int (&cj)[4]) const {
    const u64 ok[5] = {ck[0], ck[1], ck[2], ck[3], SENT};
    const int oj[5] = {cj[0], cj[1], cj[2], cj[3], 0};
    lio::knn_merge5(bk, bj, ok, oj);
  }
};

static long g_cases = 0, g_bad = 0;
static void report(const char *what, int km, const Entry *got, const std::vector<Entry> &want) {
  if (++g_bad > 5) return;
  std::fprintf(stderr, "%s differs (key map %d): got", what, km);
  for (int i = 0; i < 5; ++i) std::fprintf(stderr, " (%016llx, %d)", got[i].first, got[i].second);
  std::fprintf(stderr, "  want");
  for (int i = 0; i < 5; ++i) std::fprintf(stderr, " (%016llx, %d)", want[i].first, want[i].second);
  std::fprintf(stderr, "\n");
}
static void hold(const char *what, int km, const u64 (&bk)[5], const int (&bj)[5], std::vector<Entry> all) {
  std::sort(all.begin(), all.end());
  Entry got[5];
  bool same = true;
  for (int i = 0; i < 5; ++i) { got[i] = Entry(bk[i], bj[i]); same = same && got[i] == all[i]; }
  ++g_cases;
  if (!same) report(what, km, got, all);
}

template <class M5>
static void check_merge5(M5 merge) {
  for (int km = 0; km < 3; ++km)
    for (int na = 0; na <= 5; ++na)
      for (int nb = 0; nb <= 5; ++nb) {
        const int n = na + nb;
        for (unsigned mask = 0; mask < (1u << n); ++mask) {   // bit r set: rank r goes to list A
          if (__builtin_popcount(mask) != na) continue;
          u64 ak[5], bk[5]; int aj[5], bj[5], ia = 0, ib = 0;
          std::vector<Entry> all;
          for (int r = 0; r < n; ++r) {
            const Entry e(ranked_key(km, r, n), 100 + 7 * r);
            if ((mask >> r) & 1u) { ak[ia] = e.first; aj[ia++] = e.second; } else { bk[ib] = e.first; bj[ib++] = e.second; }
            all.push_back(e);
          }
          for (; ia < 5; ++ia) { ak[ia] = SENT; aj[ia] = 0; all.push_back(Entry(SENT, 0)); }
          for (; ib < 5; ++ib) { bk[ib] = SENT; bj[ib] = 0; all.push_back(Entry(SENT, 0)); }
          merge(ak, aj, bk, bj);
          hold("knn_merge5", km, ak, aj, all);
        }
      }
}

template <class M4>
static void check_merge4(M4 merge) {
  for (int km = 0; km < 3; ++km)
    for (int nb = 0; nb <= 5; ++nb)
      for (int nc = 0; nc <= 4; ++nc)
        for (int fill = 0; fill < 2; ++fill) {   // what the 4 - nc other slots hold: "no candidate" (sentinel key, position -1) or a NaN distance
          if (fill == 1 && nc == 4) continue;
          const int n = nb + nc;
          for (unsigned mask = 0; mask < (1u << n); ++mask) {   // bit r set: rank r is a candidate
            if (__builtin_popcount(mask) != nc) continue;
            u64 b0[5]; int j0[5], ib = 0, ic = 0;
            Entry cand[4];
            std::vector<Entry> all;
            for (int r = 0; r < n; ++r) {
              const Entry e(ranked_key(km, r, n), 100 + 7 * r);
              if ((mask >> r) & 1u) cand[ic++] = e; else { b0[ib] = e.first; j0[ib++] = e.second; }
              all.push_back(e);
            }
            for (; ic < 4; ++ic) cand[ic] = fill ? Entry(NANKEY, 900 + ic) : Entry(SENT, -1);
            for (; ib < 5; ++ib) { b0[ib] = SENT; j0[ib] = 0; all.push_back(Entry(SENT, 0)); }
            for (int i = 0; i < 5; ++i) all.push_back(Entry(SENT, 0));   // so that five entries always exist; equal to the list's own padding
            int perm[4] = {0, 1, 2, 3};
            do {
              u64 bk[5], ck[4]; int bj[5], cj[4];
              for (int i = 0; i < 5; ++i) { bk[i] = b0[i]; bj[i] = j0[i]; }
              for (int i = 0; i < 4; ++i) { ck[i] = cand[perm[i]].first; cj[i] = cand[perm[i]].second; }
              merge(bk, bj, ck, cj);
              hold("knn_merge4", km, bk, bj, all);
            } while (std::next_permutation(perm, perm + 4));
          }
        }
}

int main(int argc, char **argv) {
  const bool planted = argc > 1 && std::strcmp(argv[1], "planted") == 0;
  if (planted) {
    check_merge5(Merge5Short());
    const long bad5 = g_bad;
    g_bad = 0;
    check_merge4(Merge4Unsorted());
    std::printf("planted: knn_merge5 without its last comparator noticed in %ld cases, knn_merge4 without its sort in %ld\n", bad5, g_bad);
    return 0;
  }
  check_merge5(Merge5());
  const long n5 = g_cases;
  check_merge4(Merge4());
  std::printf("knn_merge5: %ld cases, knn_merge4: %ld cases, %ld differ\n", n5, g_cases - n5, g_bad);
  return g_bad ? 1 : 0;
}
