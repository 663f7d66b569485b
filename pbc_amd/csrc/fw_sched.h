// fw_sched.h -- HOST side of the wave-per-pairing type f kernel (pairing_fw.cuh): one pairing as a straight line of packed schedule
// entries (wave_sched.h: the entry, the by-name builder, the Miller loop; one track).  The order of the programs depends on the curve's
// constants only -- the signed digits of r (cc_miller_no_denom, ecc/f_param.c:216-233) and the bits and the sign of the BN parameter
// x (the hard part of f_tateexp, :250-283, as pairing_f.cuh f_hard_bn runs it) -- so the host writes it once per object.
// tools/fw_gen.py holds the same sequence on Python integers (miller_sequence / final_sequence / flat_schedule); tests compare.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "fw_tables.h"
#include "wave_sched.h"

namespace pbc { namespace fw {
using namespace wave;

// dst <- a^|x| by square-and-multiply on dst, conjugated for a negative x (f12_pow_x)
inline void pow_x(Builder &B, const char *dst, const char *a, uint64_t x, bool xneg) {
  const std::string d(dst), s(a);
  B.run("copy_" + d + "_" + s);
  int top = 63;
  while (top > 0 && !((x >> top) & 1)) top--;
  for (int i = top - 1; i >= 0; i--) {
    B.run("sqr_" + d + "_" + d);
    if ((x >> i) & 1) B.run("mul_" + d + "_" + d + "_" + s);
  }
  if (xneg) B.run("conj_" + d + "_" + d);
}
inline void build_final(Builder &B, uint64_t x, bool xneg) {
  // easy part: F <- F^(q^8) F^(q^6) / (F^(q^2) F), the inverse by polymod_invert's norm trick (poly.c:521-536)
  for (const char *p : {"qp2_Y_F", "qp2_Y_Y", "qp2_Y_Y", "qp2_Y_Y", "conj_U_F", "mul_Y_Y_U", "qp2_U_F", "mul_U_U_F", "qp2_T1_U", "copy_T0_T1"}) B.run(p);
  for (int i = 0; i < 4; i++) { B.run("qp2_T1_T1"); B.run("mul_T0_T0_T1"); }
  B.run("mul_T1_U_T0"); B.run("norm_T1"); B.op(OP_INV); B.run("scinv_U_T0_T1");
  B.run("mul_F_Y_U");
  // hard part: the BN vector chain (pairing_f.cuh f_hard_bn)
  pow_x(B, "FX", "F", x, xneg); pow_x(B, "FX2", "FX", x, xneg); pow_x(B, "FX3", "FX2", x, xneg);
  for (const char *p : {"frob_U_FX3", "mul_Y_U_FX3", "conj_Y_Y", "sqr_T0_Y",
                        "frob_U_FX2", "mul_Y_U_FX", "conj_Y_Y", "mul_T0_T0_Y",
                        "conj_Y_FX2", "mul_T0_T0_Y",
                        "frob_U_FX", "conj_U_U", "mul_T1_U_Y", "mul_T1_T1_T0",
                        "qp2_Y_FX2", "mul_T0_T0_Y", "sqr_T1_T1", "mul_T1_T1_T0", "sqr_T1_T1",
                        "conj_Y_F", "mul_T0_T1_Y",
                        "frob_U_F", "qp2_Y_F", "mul_FX_U_Y", "frob_U_Y", "mul_FX_FX_U", "mul_T1_T1_FX",
                        "sqr_T0_T0", "mul_F_T0_T1"}) B.run(p);
  B.op(OP_END);
}
// Sched (host_params.h WaveSched): e -- the schedules one after the other; off[] -- where each begins: the pairing; the Miller value
// alone (a TERM of a product); the product with a term's value (the three levels of mul_F_F_U, the kernel repeats them) + the final
// exponentiation
template <class Sched, class Digit>
inline bool build_schedules(Sched &S, int rbits, const Digit &digit, uint64_t x, bool xneg) {
  S.e.clear();
  Builder B(S.e, h_prog, h_level);
  S.off[SCHED_PAIRING] = S.e.size();
  build_miller(B, rbits, digit);
  build_final(B, x, xneg);
  S.off[SCHED_MILLER] = S.e.size();
  build_miller(B, rbits, digit);
  B.op(OP_END);
  S.off[SCHED_FINISH] = S.e.size();
  B.run("mul_F_F_U");
  build_final(B, x, xneg);
  S.off[SCHED_PP] = S.e.size();                                     // (no pairing_pp schedule: where the last one ends)
  return B.ok;
}

} }  // namespace pbc::fw
