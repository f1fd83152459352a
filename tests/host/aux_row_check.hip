// Stand-alone check (host code only, built with hipcc by tests/test_ds_ref.py): the aux row of launch A (csrc/solve_step.h: aux_imu,
// aux_lmap, aux_prior, aux_exprior), the relative lidar poses and the first linearisation of launch B (solve_step with
// max_iterations = 0: phases P1 - P6 and the loop head), replayed by the one-thread host executor on problems read from a file.
// It computes nothing of its own: tests/ds_cases.py writes the problems, tests/ds_ref.py holds the reference, the test compares.
//
//   aux_row_check <input> <output>
//
// Input (text; integers in decimal, doubles as C99 hex floats): the number of cases, then per case
//   Wo n ex_col n_prior have_prior use_ex_prior n_keep | keep n_keep x (kind index size offset x0_offset) | prior_col[n] | present[Wo]
//   pose (Wo + 1) x 7 | sb (Wo + 1) x 9 | ex 7 | prior_x0 90 | ex_prior_pos 3 | ex_prior_rot 4 (w x y z)
//   per IMU factor dp 3 dq 4 dv 3 ba 3 bg 3 g 3 sum_dt jac 225 sqrt_info 225 | prior JtJ lin_jac lin_res Jtr0 and one pad | S Wo x 258
// Output per case: imu_out Wo x 932 | lmap Wo x 248 | prior_out n_prior + 1 | exprior_out 44 | cand_Rt Wo x 12 | scale n | g n |
//   Hcur n x n (mirrored) | costs0 4 | it termination done need_host
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "solve_step.h"
using namespace lio;

namespace {
FILE *in = nullptr, *out = nullptr;
int geti() { int v = 0; if (std::fscanf(in, "%d", &v) != 1) { std::fprintf(stderr, "aux_row_check: integer expected\n"); std::exit(2); } return v; }
double getd() {
  char tok[64];
  if (std::fscanf(in, "%63s", tok) != 1) { std::fprintf(stderr, "aux_row_check: number expected\n"); std::exit(2); }
  char *end = nullptr;
  const double v = std::strtod(tok, &end);
  if (end == tok || *end != 0) { std::fprintf(stderr, "aux_row_check: bad number %s\n", tok); std::exit(2); }
  return v;
}
void getv(double *p, size_t n) { for (size_t k = 0; k < n; ++k) p[k] = getd(); }
void putv(const double *p, size_t n) { for (size_t k = 0; k < n; ++k) std::fprintf(out, "%a ", p[k]); std::fprintf(out, "\n"); }

int one_case() {
  std::vector<DevProblem> pbv(1);
  std::vector<DevState> stv(1);
  DevProblem &pb = pbv[0];
  DevState &st = stv[0];
  std::memset(&pb, 0, sizeof(pb));
  pb.Wo = geti(); pb.n = geti(); pb.ex_col = geti(); pb.n_prior = geti(); pb.have_prior = geti(); pb.use_ex_prior = geti(); pb.n_keep = geti();
  const int Wo = pb.Wo, n = pb.n, np = pb.n_prior;
  if (Wo < 1 || Wo > DS_MAX_WO || n < 1 || n > DS_MAX_NPAD || np < 0 || np > 128 || pb.n_keep < 0 || pb.n_keep > DS_MAX_KEEP) return 2;
  pb.n_pad = (n + DS_NB - 1) / DS_NB * DS_NB; pb.ld = pb.n_pad + 1;
  pb.max_iterations = 0; pb.bpf = 1; pb.conv_flag_in = 1; pb.imu_on = 1;
  for (int b = 0; b < pb.n_keep; ++b) { pb.keep_kind[b] = geti(); pb.keep_index[b] = geti(); pb.keep_size[b] = geti(); pb.keep_idx[b] = geti(); pb.keep_x0[b] = geti(); }
  for (int i = 0; i < DS_MAX_NPAD + 8; ++i) pb.prior_col[i] = -1;
  for (int i = 0; i < n; ++i) pb.prior_col[i] = geti();
  for (int i = 0; i < Wo; ++i) pb.pim[i].present = geti();
  WindowParams P;
  P.Wo = Wo; P.pose.resize(Wo + 1); P.sb.resize(Wo + 1);
  for (int i = 0; i <= Wo; ++i) getv(P.pose[i].data(), 7);
  for (int i = 0; i <= Wo; ++i) getv(P.sb[i].data(), 9);
  getv(P.ex.data(), 7);
  getv(pb.prior_x0, DS_MAX_KEEP * 9);
  getv(pb.ex_prior_pos, 3); getv(pb.ex_prior_rot, 4);
  for (int i = 0; i < Wo; ++i) {
    DevPim &d = pb.pim[i];
    getv(d.dp, 3); getv(d.dq, 4); getv(d.dv, 3); getv(d.ba, 3); getv(d.bg, 3); getv(d.g, 3); d.sum_dt = getd();
    getv(d.jac, 225); getv(d.sqrt_info, 225);
  }
  std::vector<double> prior_mats(ds_prior_mats_size(np) + 1);
  getv(prior_mats.data(), prior_mats.size());
  // the moments as one block's partials per frame (bpf = 1): the fold of P1 is then the identity
  std::vector<double> partials(size_t(Wo) * LIO_MOMENT_OUT, 0.0);
  for (int f = 0; f < Wo; ++f) getv(&partials[size_t(f) * LIO_MOMENT_OUT], 258);

  ds_init_state(P, st);
  std::vector<double> imu_out(size_t(Wo) * DS_IMU_OUT), lmap(size_t(Wo) * DS_LMAP_OUT), prior_out(size_t(np) + 8), exprior_out(DS_EXP_OUT),
      Hcur(size_t(pb.n_pad) * pb.ld), S_buf(size_t(2) * Wo * LIO_MOMENT_OUT), lds(ds_lds_doubles(pb.n_pad, Wo)), aux_lds(2048);
  HostExec x;
  // ---- launch A's aux row, as k_bw_aux calls it
  for (int i = 0; i < Wo; ++i) {
    aux_imu(x, pb.pim[i], st.cand.pose[i], st.cand.sb[i], st.cand.pose[i + 1], st.cand.sb[i + 1], &imu_out[size_t(i) * DS_IMU_OUT], aux_lds.data());
    aux_lmap(x, st.cand.pose[0], st.cand.pose[i + 1], st.cand.ex, &lmap[size_t(i) * DS_LMAP_OUT], aux_lds.data());
  }
  if (pb.have_prior) aux_prior(x, pb, prior_mats.data(), st.cand, prior_out.data(), aux_lds.data());
  if (pb.use_ex_prior) aux_exprior(x, pb, st.cand, exprior_out.data());
  // ---- launch B
  StepBuffers B{prior_mats.data(), partials.data(), imu_out.data(), lmap.data(), prior_out.data(), exprior_out.data(), Hcur.data(), S_buf.data(), nullptr};
  solve_step(x, pb, st, B, lds.data());

  putv(imu_out.data(), imu_out.size());
  putv(lmap.data(), lmap.size());
  putv(prior_out.data(), size_t(np) + 1);
  putv(exprior_out.data(), DS_EXP_OUT);
  putv(&st.cand_Rt[0][0], size_t(Wo) * 12);
  putv(st.scale, n);
  putv(st.g, n);
  std::vector<double> H(size_t(n) * n);
  for (int r = 0; r < n; ++r)
    for (int c = r; c < n; ++c) H[size_t(r) * n + c] = H[size_t(c) * n + r] = Hcur[size_t(r) * pb.ld + c];
  putv(H.data(), H.size());
  putv(st.costs0, 4);
  std::fprintf(out, "%d %d %d %d\n", st.it, st.termination, st.done, st.need_host);
  // the accepted point's moments are the ones just folded, and x has not moved
  const double *Sc = S_buf.data() + size_t(st.s_cur) * Wo * LIO_MOMENT_OUT;
  for (int f = 0; f < Wo; ++f)
    for (int k = 0; k < 258; ++k) if (Sc[size_t(f) * LIO_MOMENT_OUT + k] != partials[size_t(f) * LIO_MOMENT_OUT + k]) return 3;
  if (std::memcmp(&st.x, &st.cand, sizeof(DevParams)) != 0) return 4;
  return 0;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: aux_row_check <input> <output>\n"); return 2; }
  in = std::fopen(argv[1], "r");
  out = std::fopen(argv[2], "w");
  if (!in || !out) { std::fprintf(stderr, "aux_row_check: cannot open the files\n"); return 2; }
  const int cases = geti();
  int bad = 0;
  for (int c = 0; c < cases && !bad; ++c) bad = one_case();
  std::fclose(in);
  if (std::fclose(out) != 0) bad = 2;
  if (bad) std::fprintf(stderr, "aux_row_check: failed with %d\n", bad);
  return bad;
}
