// dw_sched.h -- HOST side of the wave-per-pairing type d kernel (pairing_dw.cuh): one pairing flattened into a SCHEDULE of packed
// entries (wave_sched.h).  Which level of which program runs when depends on the curve's constants only (the signed digits of r,
// the bits of Phi_6(q) / r), so the host walks the TWO TRACKS of the Miller loop and the final exponentiation ONCE per object and
// the kernel is a plain interpreter: entry -> rows -> sums (no scheduling arithmetic, no table lookups on the device; the first
// version, with the state machine in the kernel, spent ~100 scalar instructions and 5 scalar loads per level on it).
// tools/dw_gen.py holds the same walk on Python integers (Model.pairing / flat_schedule); tests compare the two.
// Four schedules per object (wave_sched.h SCHED_*): the pairing; the Miller value alone; the product with a term's value (two
// levels, the kernel repeats them) + the final exponentiation; pairing_pp_apply.
#pragma once
#include <stdint.h>
#include <vector>
#include "dw_tables.h"
#include "wave_sched.h"

namespace pbc { namespace dw {
using namespace wave;

inline uint64_t entry(int a, int b, int line = -1) {                 // a level; a, b: indices into h_level, -1: the track idles
  const LevelRef z = {0, 0, 0};
  const LevelRef &A = a >= 0 ? h_level[a] : z, &B = b >= 0 ? h_level[b] : z;
  const unsigned T = (A.lanes ? A.T : 0u) > (B.lanes ? B.T : 0u) ? A.T : (B.lanes ? B.T : 0u);
  return pack_level(A, B, T, line);
}
inline void run_levels(std::vector<uint64_t> &out, int first, int count) { for (int i = 0; i < count; i++) out.push_back(entry(first + i, -1)); }
// cc_tatepower with one inversion (pairing_d.cuh d_final_exp), then the end marker
inline void build_final(std::vector<uint64_t> &out, const uint32_t *phik, int phikbits) {
  run_levels(out, P_fe1, N_fe1);
  out.push_back(pack_op(OP_BZERO));
  run_levels(out, P_fe2, N_fe2);
  out.push_back(pack_op(OP_INV));
  run_levels(out, P_fe3, N_fe3);
  for (int j = phikbits - 1; j >= 0; j--) {                       // lucas_even (d_param.c:462-482): j == 0 takes the 0-branch
    const bool bit = j ? ((phik[j >> 5] >> (j & 31)) & 1) != 0 : false;
    run_levels(out, bit ? P_lucas1 : P_lucas0, N_lucas0);
  }
  run_levels(out, P_fe4, N_fe4);
  out.push_back(pack_op(OP_END));
}
template <class Digit>                                            // Digit(m): the signed digit of the Miller loop at position m
inline void build_miller(std::vector<uint64_t> &out, int rbits, const Digit &digit) {
  // The accumulator track: for m = rbits - 2 .. 0: product with the tangent's line; product with the chord's if the digit is
  // set (m > 0); square (m > 0) -- two levels each.  The point track: the same steps without the squares, ahead of it:
  //   * point program j leaves the COEFFICIENTS of line j in bank j % 2 and, in its first two levels, evaluates line j - 1
  //     (the other coefficient bank) into value bank (j - 1) % 2; after the last one a short program evaluates the last line;
  //   * the product with line i (both levels read value bank i % 2) starts when point program i + 1 has run two levels;
  //   * point program j starts when the product with line j - 3 is COMPLETE (its first levels overwrite that value bank).
  int fm = rbits - 2, pm = rbits - 2, fph = 0, pph = 0, lines_taken = 0, line_ready = 0, pstarted = 0, fmul_done = 0;
  int fbase = -1, flev = 0, fcount = 0, pbase = -1, plev = 0, pcount = 0;
  bool f_is_mul = false, p_exhausted = false;             // p_exhausted: the closing evaluation has been started
  for (;;) {
    if (fbase < 0) {
      while (fm >= 0 && ((fph == 1 && !(fm > 0 && digit(fm))) || (fph == 2 && fm <= 0))) { if (++fph == 3) { fph = 0; fm--; } }
      if (fm < 0) { if (pbase < 0) break; }
      else if (fph == 2) { fbase = P_f_sqr; fcount = N_f_sqr; flev = 0; f_is_mul = false; fph = 0; fm--; }
      else if (lines_taken < line_ready) {
        fbase = (lines_taken & 1) ? P_f_mul1 : P_f_mul0; fcount = N_f_mul0; flev = 0; f_is_mul = true;
        lines_taken++;
        fph++;
      }
    }
    if (pbase < 0 && !p_exhausted) {
      while (pm >= 0 && pph == 1 && !(pm > 0 && digit(pm))) { pph = 0; pm--; }
      if (pstarted < 3 || fmul_done >= pstarted - 2) {
        const int bank = pstarted & 1;
        if (pm < 0) { pbase = bank ? P_pt_eval1 : P_pt_eval0; pcount = N_pt_eval0; p_exhausted = true; }
        else if (pph == 0) { pbase = bank ? P_pt_dbl1 : P_pt_dbl0; pcount = N_pt_dbl0; pph = 1; }
        else {
          const bool neg = digit(pm) < 0;
          pbase = neg ? (bank ? P_pt_addm1 : P_pt_addm0) : (bank ? P_pt_addp1 : P_pt_addp0); pcount = N_pt_addp0;
          pph = 0; pm--;
        }
        plev = 0;
        pstarted++;
      }
    }
    out.push_back(entry(fbase >= 0 ? fbase + flev : -1, pbase >= 0 ? pbase + plev : -1));
    if (fbase >= 0 && ++flev == fcount) { fbase = -1; fmul_done += f_is_mul ? 1 : 0; }
    if (pbase >= 0) {
      ++plev;
      if (plev == 2 && pstarted >= 2) line_ready = pstarted - 1;
      if (plev == pcount) pbase = -1;
    }
  }
}
// pairing_pp_apply: the accumulator track as above; the other track only EVALUATES -- line i (coefficient bank i % 2, loaded beside
// the first level of the evaluation of line i - 1) -> value bank i % 2, two levels;
//   * the product with line i starts when its evaluation is complete;
//   * the evaluation of line i starts when the product with line i - 2 is complete (it overwrites that value bank).
template <class Digit>
inline void build_pp_miller(std::vector<uint64_t> &out, int rbits, const Digit &digit) {
  const int nl = table_lines(rbits, digit);
  out.push_back(pack_op(OP_LOADLINE, 0));
  int fm = rbits - 2, fph = 0, lines_taken = 0, evals_done = 0, fmul_done = 0, pi = 0;
  int fbase = -1, flev = 0, fcount = 0, pbase = -1, plev = 0;
  bool f_is_mul = false;
  for (;;) {
    if (fbase < 0) {
      while (fm >= 0 && ((fph == 1 && !(fm > 0 && digit(fm))) || (fph == 2 && fm <= 0))) { if (++fph == 3) { fph = 0; fm--; } }
      if (fm < 0) { if (pbase < 0) break; }
      else if (fph == 2) { fbase = P_f_sqr; fcount = N_f_sqr; flev = 0; f_is_mul = false; fph = 0; fm--; }
      else if (lines_taken < evals_done) {
        fbase = (lines_taken & 1) ? P_f_mul1 : P_f_mul0; fcount = N_f_mul0; flev = 0; f_is_mul = true;
        lines_taken++;
        fph++;
      }
    }
    if (pbase < 0 && pi < nl && (pi < 2 || fmul_done >= pi - 1)) {
      pbase = ((pi + 1) & 1) ? P_pt_eval1 : P_pt_eval0;           // pt_eval{b} evaluates the OTHER bank
      plev = 0;
      pi++;
    }
    const int line = (pbase >= 0 && plev == 0 && pi < nl) ? pi : -1;
    out.push_back(entry(fbase >= 0 ? fbase + flev : -1, pbase >= 0 ? pbase + plev : -1, line));
    if (fbase >= 0 && ++flev == fcount) { fbase = -1; fmul_done += f_is_mul ? 1 : 0; }
    if (pbase >= 0 && ++plev == N_pt_eval0) { pbase = -1; evals_done++; }
  }
}
// Sched (host_params.h WaveSched): e -- the four schedules one after the other; off[4] -- where each begins; lines -- the lines of a
// pairing_pp table
template <class Sched, class Digit>
inline bool build_schedules(Sched &S, int rbits, const Digit &digit, const uint32_t *phik, int phikbits) {
  S.e.clear();
  S.lines = table_lines(rbits, digit);
  S.off[SCHED_PAIRING] = S.e.size();
  build_miller(S.e, rbits, digit);
  build_final(S.e, phik, phikbits);
  S.off[SCHED_MILLER] = S.e.size();
  build_miller(S.e, rbits, digit);
  S.e.push_back(pack_op(OP_END));
  S.off[SCHED_FINISH] = S.e.size();
  run_levels(S.e, P_f_mul0, N_f_mul0);
  build_final(S.e, phik, phikbits);
  S.off[SCHED_PP] = S.e.size();
  build_pp_miller(S.e, rbits, digit);
  build_final(S.e, phik, phikbits);
  return true;
}

} }  // namespace pbc::dw
