// pairing_gw.cuh -- Type G (MNT, k = 10) on the five-word fields, ONE PAIRING PER WAVEFRONT (round 6; small batches).
//
// Same value as the type g pairing (ecc/g_param.c: the Miller loop of cc_miller_no_denom_affine and cc_tatepower :471-558), the
// formulas of pairing_d.cuh's TypeMNT<5, 5>.  The throughput kernel runs a pairing as one lane's instruction stream: 14.4 ms through
// the reference's call sites whatever the batch size (one CPU core: 4.3 ms).  Here a wavefront owns one pairing on the machine
// of wave_vm.cuh: every F_q element a slot of an LDS slot file (240 slots), a LEVEL = every lane computes one lazily reduced
// sum of F_q products from the slots its table row names (gw_tables.h, generated and checked against the reference's vectors on
// Python integers by tools/gw_gen.py: sums of more than eight terms are chained, over-full levels repacked), the schedule a straight
// line the host writes once per object (gw_sched.h; 2542 levels).  This file is the type g FAMILY of that machine: the set-up
// (byte loads, curve checks, twist map), ordinary code on lane 0, and which slots the B = 0 test and the one inversion work on.
#pragma once
#include "pairing_d.cuh"
#include "wave_vm.cuh"
#include "gw_tables.h"

namespace pbc {

struct GwTables {
  static constexpr int kSlots = gw::kSlots, kRows = gw::kRows;
  static PBC_DEV const uint32_t *rows_src() { return gw::g_rows; }
  static constexpr bool kLines = true;                              // pairing_pp tables: their lines arrive in slots
  static PBC_DEV int line_slot(int) { return gw::S_La; }           // La, Lb, Lc: consecutive slots
};

template <int ND>
struct GW {
  typedef WaveVM<ND, GwTables> VM;
  static constexpr int DEG = 5;
  typedef TypeMNT<ND, DEG> G;
  typedef typename G::fq fq;
  typedef typename G::f3 f5;                           // (pairing_d.cuh keeps type d's names: f3 = F_q^d)
  static constexpr int L = VM::L;
  static constexpr int kCoef = 2 * DEG, kF = gw::S_f_x0;           // f.x0..4, f.y0..4
  static constexpr int kG1 = 2, kG2 = 2 * DEG, kGT = 2 * DEG;
  // the finish step of a product: a term's value -> register u; the levels of mul_f_u, up to the schedule's mark, multiply it in
  static constexpr int kOperand = gw::S_u_x0, kProdEntries = 0;
  static constexpr bool kFinishPrefetch = false, kHasMark = true;      // OP_MARK ends mul_f_u in the finish schedule

  // ---- lane 0: constants; bytes -> slots, curve checks, twist map (d_setup_lane) ----
  static __device__ __noinline__ void setup_consts() {
    using namespace gw;
    fq t;
    VM::put_small_consts({S_ZERO, S_ONE, S_M1, S_TWO, S_M2, S_THREE, S_FOUR, S_M8, S_SIXTEEN, S_HALF});
    fp_halve<ND>(t, G::dk(c_d.nqrinv)); fp_halve<ND>(t, t); VM::put_fq(S_QVI, t);
    VM::put_fq(S_A, G::dk(c_d.A));
    const fq v = G::dk(c_d.nqr);
    VM::put_fq(S_V, v);
    fp_neg<ND>(t, v); VM::put_fq(S_NV, t);
    for (int j = 0; j < DEG - 1; j++)
      for (int k = 0; k < DEG; k++) {
        fl<ND> a;
        for (int l = 0; l < L; l++) a.l[l] = c_d.xpwr29[(j * DEG + k) * L + l];
        VM::put(S_XP5_0 + j * DEG + k, a);
        const fq xq = G::dk(c_d.xpowq[j][k]);
        VM::put_fq(S_XQ1_0 + j * DEG + k, xq);
        fp_neg<ND>(t, xq);
        VM::put_fq(S_NXQ1_0 + j * DEG + k, t);
      }
  }
  // (g1 == nullptr: pairing_pp_apply -- no first argument, the table stands for it)
  static __device__ __noinline__ bool setup_inputs(const uint8_t *g1, const uint8_t *g2) {
    using namespace gw;
    const int NB = (int) fpk<ND>().fbytes;
    fq one, Px, Py;
    fp_set<ND>(one, fpk<ND>().one);
#pragma unroll
    for (int k = 0; k < ND; k++) Px.v[k] = Py.v[k] = 0;
    f5 Qx, Qy;
    if (g1) {
      fp_load_be<ND>(Px, g1);
      fp_load_be<ND>(Py, g1 + NB);
    }
    G::f3_load_be(Qx, g2);
    G::f3_load_be(Qy, g2 + DEG * NB);
    bool valid;
    {
      // curve_is_valid_point (curve.c:57-77): E: y^2 = x^3 + a x + b; the twist over F_q^5
      fq t0, t1;
      fp_sqr<ND>(t0, Px);
      fp_add<ND>(t0, t0, G::dk(c_d.A));
      fp_mul<ND>(t0, t0, Px);
      fp_add<ND>(t0, t0, G::dk(c_d.B));
      fp_sqr<ND>(t1, Py);
      valid = fp_eq<ND>(t0, t1) | (g1 == nullptr);
      f5 u0, u1;
      G::f3_sqr(u0, Qx);
      fp_add<ND>(u0.c[0], u0.c[0], G::dk(c_d.ta));
      G::f3_mul(u0, u0, Qx);
      fp_add<ND>(u0.c[0], u0.c[0], G::dk(c_d.tb));
      G::f3_sqr(u1, Qy);
      valid &= G::f3_eq(u0, u1);
    }
    // twist map (x, y) -> (v^-1 x, v^-2 y sqrt(v)); v times the second: v^-1 y
    {
      f5 qx, qy, vqy;
      G::f3_mul_fq(qx, Qx, G::dk(c_d.nqrinv));
      G::f3_mul_fq(qy, Qy, G::dk(c_d.nqrinv2));
      G::f3_mul_fq(vqy, Qy, G::dk(c_d.nqrinv));
      for (int i = 0; i < DEG; i++) { VM::put_fq(S_Qx0 + i, qx.c[i]); VM::put_fq(S_Qy0 + i, qy.c[i]); VM::put_fq(S_VQy0 + i, vqy.c[i]); }
    }
    VM::put_point_state({S_X, S_Y, S_Z, S_nZ, S_ZZ, S_ZZZ, S_Px, S_Py, S_nPy}, Px, Py);
    VM::put_fq(S_W, G::dk(c_d.A));
    VM::put_fq(S_f_x0, one);                               // f = 1 (the other nine slots are zero from begin())
    return valid;
  }
  static PBC_DEV bool lane_op(int op) {
    if (op == wave::OP_BZERO) VM::template bzero_test<DEG>(gw::S_wB0, gw::S_Bn0);
    else if (op == wave::OP_INV) VM::inversion(gw::S_nrm, gw::S_ninv);
    else return false;
    return true;
  }
};

}  // namespace pbc
