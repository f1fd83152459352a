// wide_lds_check.hip — the step kernel's LDS carve (csrc/solve_step.h: carve_lds, ds_lds_doubles) for every window the device loop
// takes: Wo = 1 .. 7, free and constant extrinsic.  Host code only; tests/test_wide_window_lds.py builds it with the address and
// undefined-behaviour sanitizers and runs it.
//
// Checked per (n_pad, Wo):
//   * every array lies inside ds_lds_doubles(n_pad, Wo) * 8 bytes (and is written end to end on a heap block of exactly that size);
//   * two arrays whose lifetimes overlap occupy disjoint bytes — lifetimes as phases P1 .. P8 of solve_step, written out below from the
//     statements that touch each array, not from the carve;
//   * the total is at most 160 KiB, the LDS of a workgroup;
//   * the control block holds StepCtl, and a launch sized for the largest window of a group holds every smaller window's carve.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "solve_step.h"

using namespace lio;

struct Span {
  const char *name;
  const double *p;
  size_t len;      // doubles
  int first, last; // phases of solve_step in which the array holds something that is read later (inclusive)
};

// The lifetimes (solve_step, phases P1 .. P8):
//   A      all phases (Sx / LS of P1 - P3 live in it, then H)
//   tmp    P1 (cost and count per frame) .. P5 (the decision reads them), and scratch of P7's Cauchy step
//   zb     P2 / P3 (ds_lidar_blocks writes it) .. P4 (the lidar pass reads it); dead behind the barrier that ends P4
//   part   P4 (the prior's column of every tangent column) .. P7 (the factorisation's scratch)
//   gz     P4 (g is assembled in it) .. P7 (right-hand side and solution of the factorisation)
//   hdiag, scale, g            first written in P6; read through P7 (scale: P8)
//   diag, grad, gn, step       P6's reject branch reloads them, P7 computes them; step and scale are read in P8
//   invd, xinv                 inside ds_ldlt_solve (P7) only
//   red    block reductions of P6 .. P8
//   ctl    all phases
static std::vector<Span> spans(const StepLds &L, int n_pad, int Wo) {
  const size_t v = size_t(n_pad);
  return {
      {"A", L.A, v * (v + 1), 1, 8},
      {"tmp", L.tmp, v, 1, 7},
      {"zb", L.zb, size_t(Wo) * 344, 2, 4},
      {"part", L.part, DS_PART, 4, 7},
      {"gz", L.gz, v, 4, 7},
      {"hdiag", L.hdiag, v, 6, 7},
      {"scale", L.scale, v, 6, 8},
      {"g", L.g, v, 6, 7},
      {"diag", L.diag, v, 6, 7},
      {"grad", L.grad, v, 6, 7},
      {"gn", L.gn, v, 6, 7},
      {"step", L.step, v, 6, 8},
      {"invd", L.invd, v, 7, 7},
      {"xinv", L.xinv, v * DS_NB, 7, 7},
      {"red", L.red, 64, 6, 8},
      {"ctl", reinterpret_cast<const double *>(L.ctl), 32, 1, 8},
  };
}

int main() {
  int bad = 0;
  const size_t limit = 160 * 1024;
  static_assert(sizeof(StepCtl) <= 32 * sizeof(double), "the control block's 32 doubles hold StepCtl");
  std::printf("  Wo  ex    n n_pad  doubles    bytes  headroom  shared bytes\n");
  struct Shape { int n_pad, Wo; };
  std::vector<Shape> shapes;
  for (int Wo = 1; Wo <= DS_MAX_WO; ++Wo)
    for (int ex = 0; ex < 2; ++ex) {
      const int n = 15 * (Wo + 1) + 6 * ex, n_pad = (n + DS_NB - 1) / DS_NB * DS_NB;
      shapes.push_back({n_pad, Wo});
      const size_t total = ds_lds_doubles(n_pad, Wo), bytes = total * sizeof(double);
      if (n_pad > DS_MAX_NPAD) { std::printf("FAIL Wo %d ex %d: n_pad %d beyond DS_MAX_NPAD\n", Wo, ex, n_pad); ++bad; }
      if (bytes > limit) { std::printf("FAIL Wo %d ex %d: %zu bytes of LDS, a workgroup has %zu\n", Wo, ex, bytes, limit); ++bad; continue; }
      double *base = static_cast<double *>(std::malloc(bytes));   // exactly the launch's size: a write past it is the sanitizer's
      if (!base) return 2;
      const StepLds L = carve_lds(base, n_pad, Wo);
      const std::vector<Span> sp = spans(L, n_pad, Wo);
      size_t shared = 0;
      for (size_t i = 0; i < sp.size(); ++i) {
        const Span &a = sp[i];
        if (a.p < base || a.p + a.len > base + total) { std::printf("FAIL Wo %d ex %d: %s leaves the block\n", Wo, ex, a.name); ++bad; continue; }
        if ((reinterpret_cast<uintptr_t>(a.p) - reinterpret_cast<uintptr_t>(base)) % sizeof(double)) { std::printf("FAIL %s is not aligned\n", a.name); ++bad; }
        double *w = const_cast<double *>(a.p);
        for (size_t k = 0; k < a.len; ++k) w[k] = double(i);       // end to end
        for (size_t j = 0; j < i; ++j) {
          const Span &b = sp[j];
          const bool bytes_meet = a.p < b.p + b.len && b.p < a.p + a.len;
          const bool lives_meet = a.first <= b.last && b.first <= a.last;
          if (bytes_meet && lives_meet) { std::printf("FAIL Wo %d ex %d: %s (P%d-P%d) and %s (P%d-P%d) share bytes\n", Wo, ex, a.name, a.first, a.last, b.name, b.first, b.last); ++bad; }
          if (bytes_meet) {
            const double *lo = a.p > b.p ? a.p : b.p, *hi = a.p + a.len < b.p + b.len ? a.p + a.len : b.p + b.len;
            shared += size_t(hi - lo) * sizeof(double);
          }
        }
      }
      std::printf("  %2d  %2d  %3d   %3d  %7zu  %7zu  %8zu  %12zu\n", Wo, ex, n, n_pad, total, bytes, limit - bytes, shared);
      std::free(base);
    }
  // launch_bw_step sizes a launch by the largest n_pad and the largest Wo of its windows: every window's own carve must fit it
  for (const Shape &a : shapes)
    for (const Shape &b : shapes) {
      const int np = a.n_pad > b.n_pad ? a.n_pad : b.n_pad, wo = a.Wo > b.Wo ? a.Wo : b.Wo;
      if (ds_lds_doubles(np, wo) < ds_lds_doubles(a.n_pad, a.Wo)) { std::printf("FAIL a launch for (%d, %d) does not hold (%d, %d)\n", np, wo, a.n_pad, a.Wo); ++bad; }
      if (ds_lds_doubles(np, wo) * sizeof(double) > limit) { std::printf("FAIL a launch for (%d, %d) exceeds the workgroup's LDS\n", np, wo); ++bad; }
    }
  std::printf(bad ? "%d FAILURES\n" : "OK\n", bad);
  return bad ? 1 : 0;
}
