// gw_sched.h -- HOST side of the wave-per-pairing type g kernel (pairing_gw.cuh): one pairing as a straight line of packed schedule
// entries (wave_sched.h: the entry, the by-name builder, the Miller loop; one track).  The order of the programs depends on the curve's
// constants only -- the signed digits of r (cc_miller_no_denom_affine, the loop of ecc/d_param.c:321-422 that ecc/g_param.c shares) and
// the bits of Phi_10(q) / r (lucas_even of cc_tatepower, g_param.c:471-558) -- so the host writes it once per object.
// tools/gw_gen.py holds the same sequence on Python integers (sequence / flat_schedule); tests compare.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "gw_tables.h"
#include "wave_sched.h"

namespace pbc { namespace gw {
using namespace wave;

inline void build_final(Builder &B, const uint32_t *phik, int phikbits) {
  // cc_tatepower with one inversion (pairing_d.cuh d_final_exp)
  B.run("fe1"); B.op(OP_BZERO); B.run("fe2"); B.op(OP_INV); B.run("fe3");
  for (int j = phikbits - 1; j >= 0; j--) {                         // lucas_even: j == 0 takes the 0-branch
    const bool bit = j ? ((phik[j >> 5] >> (j & 31)) & 1) != 0 : false;
    B.run(bit ? "lucas1" : "lucas0");
  }
  B.run("fe4");
  B.op(OP_END);
}
// Sched (host_params.h WaveSched): the pairing; the Miller value alone (a TERM of a product); the product with a term's value (mul_f_u, a
// mark: the kernel repeats the entries before it) + the final exponentiation; pairing_pp_apply (line i of the table -> La, Lb, Lc: the
// first by an entry of its own, line i + 1 beside the first level of the product with line i)
template <class Sched, class Digit>
inline bool build_schedules(Sched &S, int rbits, const Digit &digit, const uint32_t *phik, int phikbits) {
  S.e.clear();
  Builder B(S.e, h_prog, h_level);
  S.off[SCHED_PAIRING] = S.e.size();
  build_miller(B, rbits, digit);
  build_final(B, phik, phikbits);
  S.off[SCHED_MILLER] = S.e.size();
  build_miller(B, rbits, digit);
  B.op(OP_END);
  S.off[SCHED_FINISH] = S.e.size();
  B.run("mul_f_u");
  B.op(OP_MARK);
  build_final(B, phik, phikbits);
  S.off[SCHED_PP] = S.e.size();
  S.lines = table_lines(rbits, digit);
  B.op(OP_LOADLINE, 0);
  int i = 0;
  for (int m = rbits - 2; m >= 0; m--) {
    const int nl = 1 + ((m > 0 && digit(m)) ? 1 : 0);
    for (int t = 0; t < nl; t++) {
      B.run("ln_eval");
      B.run_with_line("line_mul", i + 1 < S.lines ? i + 1 : -1);
      i++;
    }
    if (m > 0) B.run("f_sqr");
  }
  build_final(B, phik, phikbits);
  return B.ok;
}

} }  // namespace pbc::gw
