// pairing_dw.cuh -- Type D (MNT, k = 6) on the five- to seven-word fields, ONE PAIRING PER WAVEFRONT (round 6; small batches):
// the type d FAMILY of the wavefront level machine (wave_vm.cuh).
//
// Same value as cc_pairing (ecc/d_param.c:570-587: cc_miller_no_denom_affine :321-422 + cc_tatepower :505-564), the
// formulas of pairing_d.cuh.  The throughput kernel runs a pairing as one lane's serial instruction stream: 2.0 M vector
// instructions, 3.9 ms through the reference's call sites whatever the batch size -- three times what one CPU core needs
// (VERDICT r5 "missing" 1).  On the machine a pairing is 1262 levels of independent lazily reduced sums (the throughput kernel:
// ~30 000 dependent products) on a slot file of 149 slots, 3.5 KB per wavefront, with BOTH tracks at work:
//   * the first lanes run the ACCUMULATOR track (f <- f * line and f <- f^2: 2 levels each), the last lanes the POINT track
//     (V <- 2V in modified Jacobian coordinates: 4 levels, V <- V +- P: 5; the line's value at Q rides in the next point
//     program) ahead of it, each advancing one level per step of the machine; the final exponentiation (Lucas ladder: 2
//     levels per exponent bit) runs on one track.
// The level programs: dw_tables.h (tools/dw_gen.py); the schedule: dw_sched.h.  Here: the set-up (byte loads, curve checks,
// twist map), the B = 0 test and the one inversion, ordinary lane code on lane 0.  Measured (profiles/r06_notes.md): one
// pairing 1.15 ms (lane kernel 4.1 ms, one CPU core 1.35 ms), up to 1024 pairings at the latency of one, 1.35 M pairings/s at 4096.
#pragma once
#include "pairing_d.cuh"
#include "wave_vm.cuh"
#include "dw_tables.h"

namespace pbc {

struct DwTables {
  static constexpr int kSlots = dw::kSlots, kRows = dw::kRows;
  static PBC_DEV const uint32_t *rows_src() { return dw::g_rows; }
  static constexpr bool kLines = true;                              // pairing_pp tables: their lines arrive in slots
  static PBC_DEV int line_slot(int line) { return dw::S_L0_a + 3 * (line & 1); }   // where a', b', c' of a pairing_pp table line go: bank (line % 2)
};

template <int ND>
struct DW {
  typedef WaveVM<ND, DwTables> VM;
  typedef TypeMNT<ND, 3> D;
  typedef typename D::fq fq;
  typedef typename D::f3 f3;
  static constexpr int L = VM::L;
  static constexpr int kCoef = 6, kF = dw::S_f_x0;                 // f.x0..2, f.y0..2
  static constexpr int kG1 = 2, kG2 = 6, kGT = 6;
  // the finish step of a product: a term's value -> value bank 0, the two levels of f_mul0 multiply it in
  static constexpr int kOperand = dw::S_V0_x0, kProdEntries = dw::N_f_mul0;
  static constexpr bool kFinishPrefetch = true, kHasMark = false;

  // ---- lane 0: constants; bytes -> slots, curve checks, twist map (d_setup_lane) ----
  static __device__ __noinline__ void setup_consts() {
    using namespace dw;
    fq one, zero, t;
    fp_set<ND>(one, fpk<ND>().one);
#pragma unroll
    for (int k = 0; k < ND; k++) zero.v[k] = 0;
    VM::put_small_consts({S_ZERO, S_ONE, S_M1, S_TWO, S_M2, S_THREE, S_FOUR, S_M8, S_SIXTEEN, S_HALF});
    fp_halve<ND>(t, D::dk(c_d.nqrinv)); fp_halve<ND>(t, t); VM::put_fq(S_QVI, t);
    VM::put_fq(S_A, D::dk(c_d.A));
    VM::put_fq(S_V, D::dk(c_d.nqr));
    for (int k = 0; k < 3; k++) {
      fl<ND> a, b;
      for (int l = 0; l < L; l++) { a.l[l] = c_d.xpwr29[(0 * 3 + k) * L + l]; b.l[l] = c_d.xpwr29[(1 * 3 + k) * L + l]; }
      VM::put(S_XP3_0 + k, a);
      VM::put(S_XP4_0 + k, b);
      VM::put_fq(S_XQ1_0 + k, D::dk(c_d.xpowq[0][k]));
      VM::put_fq(S_XQ2_0 + k, D::dk(c_d.xpowq[1][k]));
      fq xa, xb;                                      // v x^3, v x^4: the folds of v ay by in the two-level F_q^6 products
      from_limbs<ND>(xa, a);
      from_limbs<ND>(xb, b);
      fp_mul<ND>(xa, xa, D::dk(c_d.nqr));
      fp_mul<ND>(xb, xb, D::dk(c_d.nqr));
      VM::put_fq(S_VXP3_0 + k, xa);
      VM::put_fq(S_VXP4_0 + k, xb);
    }
    for (int i = 0; i < 3; i++) { VM::put_fq(S_f_x0 + i, i ? zero : one); VM::put_fq(S_f_y0 + i, zero); }     // f = 1
  }
  // the first argument: curve_is_valid_point (curve.c:57-77) on E: y^2 = x^3 + a x + b, then the point track's state
  static __device__ __noinline__ bool setup_point(const uint8_t *g1) {
    using namespace dw;
    const int NB = (int) fpk<ND>().fbytes;
    fq Px, Py, t0, t1;
    fp_load_be<ND>(Px, g1);
    fp_load_be<ND>(Py, g1 + NB);
    fp_sqr<ND>(t0, Px);
    fp_add<ND>(t0, t0, D::dk(c_d.A));
    fp_mul<ND>(t0, t0, Px);
    fp_add<ND>(t0, t0, D::dk(c_d.B));
    fp_sqr<ND>(t1, Py);
    VM::put_point_state({S_X, S_Y, S_Z, S_nZ, S_ZZ, S_ZZZ, S_Px, S_Py, S_nPy}, Px, Py);
    VM::put_fq(S_W, D::dk(c_d.A));
    return fp_eq<ND>(t0, t1);
  }
  // the second argument: the check on the twist over F_q^3, then the twist map (x, y) -> (v^-1 x, v^-2 y sqrt(v))
  // (cc_pairing, d_param.c:580-582)
  static __device__ __noinline__ bool setup_twist(const uint8_t *g2) {
    using namespace dw;
    const int NB = (int) fpk<ND>().fbytes;
    f3 Qx, Qy, u0, u1;
    D::f3_load_be(Qx, g2);
    D::f3_load_be(Qy, g2 + 3 * NB);
    D::f3_sqr(u0, Qx);
    fp_add<ND>(u0.c[0], u0.c[0], D::dk(c_d.ta));
    D::f3_mul(u0, u0, Qx);
    fp_add<ND>(u0.c[0], u0.c[0], D::dk(c_d.tb));
    D::f3_sqr(u1, Qy);
    const bool valid = D::f3_eq(u0, u1);
    D::f3_mul_fq(Qx, Qx, D::dk(c_d.nqrinv));
    D::f3_mul_fq(Qy, Qy, D::dk(c_d.nqrinv2));
    for (int i = 0; i < 3; i++) { VM::put_fq(S_Qx0 + i, Qx.c[i]); VM::put_fq(S_Qy0 + i, Qy.c[i]); }
    return valid;
  }

  static PBC_DEV bool setup_inputs(const uint8_t *g1, const uint8_t *g2) {    // (g1 == nullptr: the point track has nothing to do)
    const bool a = g1 ? setup_point(g1) : true, b = setup_twist(g2);
    return a && b;
  }

  static PBC_DEV bool lane_op(int op) {
    if (op == wave::OP_BZERO) VM::template bzero_test<3>(dw::S_wB0, dw::S_Bn0);
    else if (op == wave::OP_INV) VM::inversion(dw::S_nrm0, dw::S_ninv);
    else return false;
    return true;
  }
};

}  // namespace pbc
