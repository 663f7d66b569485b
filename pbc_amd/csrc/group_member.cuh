// group_member.cuh -- membership verdicts for records of G1, G2 and GT (include/pbc_hip.h
// pbc_hip_element_membership_batch): is the record a point of the curve / a unit at all, and is it killed by the group
// order r = pairing->r (include/pbc_pairing.h; type a1: the composite n)?  curve_from_bytes (ecc/curve.c:609-623) tests
// the curve equation only (curve_is_valid_point, :57-77), so a record may hold any point of E(F_q) -- of the whole twist
// for G2 of types d, f, g -- and a PBC program finds out with element_mul_mpz(t, P, r) + element_is0(t), on GT with
// element_pow_mpz(t, x, r) + element_is1(t).  Here: one unit per lane, one result byte.
//
// Points.  r is public, odd and fixed per object, and its signed digits are in every family's constant block already
// (hostbn.h naf_of_half: the Miller loops' digits of n = r >> 1, digit i at bit i + 1; type e keeps r in binary), so
// r = 2 n + 1 has the digits of n above a last digit d0 = +1.  The FAST lane runs V = [r - 1] P = [2 n] P: a Jacobian
// ladder over the digits of n (one doubling per digit, one mixed addition of +-P per non-zero digit -- wave-uniform, the
// digits are constants), one closing doubling, no table, no inversion.  [r] P = O iff V = -P, read off projectively:
// X_V = x_P Z^2, Y_V = -y_P Z^3, Z != 0.  ("Z = 0 after a last mixed addition V + P" would not do: there H = 0 covers
// V = -P, the answer O, AND V = P, a doubling the chord formulas cannot express.)  The step formulas are the incomplete
// ones: an addition that meets V = +-P (H = 0), a doubling of a point with Y = 0 and V = O all leave Z = 0, and Z = 0 is
// kept by every later step.  That happens only when the order of P divides a prefix of the digits or a prefix +- 1 (small
// or crafted orders); the lane then reports itself -- Z = 0 at the end -- and the COMPLETE lane decides it: the same
// digits, d0 included, over the complete law of ec_mul_lane (group_ops.cuh ec_dbl_jac / ec_madd_jac), verdict Z = 0.
// A lane whose Z is non-zero at the end met no exceptional step, so its V is [r - 1] P and its verdict is final.
//
// GT.  0 is no unit (INVALID), 1 is the identity; otherwise x^r by square-and-multiply over the bits of r, which are
// rebuilt from the signed digits while the loop runs (r = (plus | 1) - minus, one borrow), low bit first.  The 512-bit
// type a field powers elements of norm 1 with the Lucas ladder of element_pow_zn (group_al.cuh gt_pow_lane), which tests
// its precondition; any other element is reported and takes the generic power.
#pragma once
#include "group_more.cuh"
#include "group_al.cuh"

namespace pbc {

constexpr uint8_t kMemberInvalid = 0, kMemberOutside = 1, kMemberInside = 2, kMemberIdentity = 3;   // PBC_HIP_MEMBER_*

// ---- the group order as the constant block holds it ---------------------------------------------------------------------------
// bits(): positions 0 .. bits() - 1 carry digits, the top one is +1.  digit(m): the signed digit of r at position m >= 1
// (position 0 is d0 = +1 for every family: r is odd).  plus(m) / minus(m): the same as two bits, for the binary rebuild.
struct ROfA {                          // types a, a1 (AConst: naf_of_half of r / n)
  static PBC_DEV int bits() { return c_a.rbits; }
  static PBC_DEV uint32_t plus(int m) { return (c_a.r[m >> 5] >> (m & 31)) & 1; }
  static PBC_DEV uint32_t minus(int m) { return (c_a.rm[m >> 5] >> (m & 31)) & 1; }
};
struct ROfD {                          // types d, g
  static PBC_DEV int bits() { return c_d.rbits; }
  static PBC_DEV uint32_t plus(int m) { return (c_d.r[m >> 5] >> (m & 31)) & 1; }
  static PBC_DEV uint32_t minus(int m) { return (c_d.rm[m >> 5] >> (m & 31)) & 1; }
};
struct ROfF {                          // type f
  static PBC_DEV int bits() { return c_f.rbits; }
  static PBC_DEV uint32_t plus(int m) { return (c_f.r[m >> 5] >> (m & 31)) & 1; }
  static PBC_DEV uint32_t minus(int m) { return (c_f.rm[m >> 5] >> (m & 31)) & 1; }
};
struct ROfE {                          // type e: r in binary
  static PBC_DEV int bits() { return c_e.rbits; }
  static PBC_DEV uint32_t plus(int m) { return (c_e.r[m >> 5] >> (m & 31)) & 1; }
  static PBC_DEV uint32_t minus(int) { return 0; }
};
template <class RP>
PBC_DEV int r_digit(int m) { return m ? (int) RP::plus(m) - (int) RP::minus(m) : 1; }

// ---- points over a field policy F (group_ops.cuh: FqOps; FdOps / Fq2Ops on the twists) ---------------------------------------
// The record as every other entry point reads it: coordinates reduced mod q on load; all-zero coordinates: O (IDENTITY;
// on y^2 = x^3 + x this is the 2-torsion point (0, 0), include/pbc_hip.h "zero-filled records"); curve_is_valid_point
// otherwise.  Returns IDENTITY, INVALID, or OUTSIDE for "a finite point of the curve: go on".
template <class F>
PBC_DEV uint8_t ec_member_load(typename F::el &x, typename F::el &y, const uint8_t *in) {
  typename F::el t0, t1;
  F::load(x, in);
  F::load(y, in + F::bytes());
  F::sqr(t0, x);
  F::add(t0, t0, F::curve_a());
  F::mul(t0, t0, x);
  F::add(t0, t0, F::curve_b());
  F::sqr(t1, y);
  const bool zero = F::is0(x) & F::is0(y), on = F::eq(t0, t1);
  return zero ? kMemberIdentity : on ? kMemberOutside : kMemberInvalid;
}
// The fast lane.  `flag`: the verdict is not final, the lane needs ec_member_complete_lane.
template <class F, class RP>
PBC_DEV uint8_t ec_member_fast_lane(const uint8_t *in, bool &flag) {
  typedef typename F::el el;
  el x, y, ny = F::zero();
  const uint8_t cls = ec_member_load<F>(x, y, in);
  F::sub(ny, ny, y);
  const el ca = F::curve_a();
  el X = x, Y = y, Z = F::one();       // the top digit: V = P
  for (int m = RP::bits() - 2; m >= 1; m--) {
    ec_dbl_jac<F>(X, Y, Z, ca);
    const int d = r_digit<RP>(m);      // (wave-uniform)
    if (d) ec_madd_inc<F>(X, Y, Z, x, d > 0 ? y : ny);
  }
  ec_dbl_jac<F>(X, Y, Z, ca);          // V = [r - 1] P
  el zz, t, u;
  F::sqr(zz, Z);
  F::mul(t, x, zz);
  F::mul(u, zz, Z);
  F::mul(u, ny, u);
  const bool z0 = F::is0(Z), inside = F::eq(t, X) & F::eq(u, Y) & !z0;
  flag = cls == kMemberOutside && z0;
  return cls != kMemberOutside ? cls : inside ? kMemberInside : kMemberOutside;
}
// The complete lane: [r] P over all digits, V from O, with the case analysis of ec_madd_jac (V = O, V = -P, V = P through
// the double of P formed beforehand; the double of -P is that of P with Y negated).  Verdict: [r] P is O.
template <class F, class RP>
PBC_DEV uint8_t ec_member_complete_lane(const uint8_t *in) {
  typedef typename F::el el;
  el x, y, ny = F::zero();
  const uint8_t cls = ec_member_load<F>(x, y, in);
  F::sub(ny, ny, y);
  const el one = F::one(), ca = F::curve_a();
  el DX = x, DY = y, DZ = one, nDY = F::zero();
  ec_dbl_jac<F>(DX, DY, DZ, ca);
  F::sub(nDY, nDY, DY);
  el X = one, Y = one, Z = F::zero();
  for (int m = RP::bits() - 1; m >= 0; m--) {
    ec_dbl_jac<F>(X, Y, Z, ca);
    const int d = r_digit<RP>(m);
    if (d > 0) ec_madd_jac<F>(X, Y, Z, x, y, DX, DY, DZ, true);
    else if (d < 0) ec_madd_jac<F>(X, Y, Z, x, ny, DX, nDY, DZ, true);
  }
  return cls != kMemberOutside ? cls : F::is0(Z) ? kMemberInside : kMemberOutside;
}

// ---- the 512-bit type a field: the fast lane on the limb-form steps of element_mul_zn (group_al.cuh ec_dbl / ec_madd) ----------
// V = (X, Y) in registers, Z and Z^2 in the lane's LDS slots, as there.  P itself is NOT kept across the ladder: a Solinas
// r has one or two non-zero digits below the top, so the record is read again where it is added and for the end test, and
// the doubling chain runs on the registers of ec_dbl alone.  The end test is the head of ec_madd for V + (-P): H = x Z^2 -
// X, R = -y Z^3 - Y, both zero mod q, with Z non-zero.
template <int N>
struct MemberAL {
  typedef GAL<N> G;
  typedef AL<N> A;
  typedef typename A::el el;
  typedef typename A::jacl jacl;
  static PBC_DEV void load_point(el &Px, el &Py, const uint8_t *in, bool negate) {
    fp<N> x, y;
    fp_load_be<N>(x, in);
    fp_load_be<N>(y, in + 4 * N);
    if (negate) fp_neg<N>(y, y);       // (wave-uniform: the digit's sign)
    A::to_el(Px, x);
    A::to_el(Py, y);
  }
  static PBC_DEV uint8_t fast_lane(const uint8_t *in, bool &flag) {
    uint8_t cls;
    jacl V;
    {
      fp<N> x, y;
      fp_load_be<N>(x, in);
      fp_load_be<N>(y, in + 4 * N);
      const bool zero = fp_is0<N>(x) & fp_is0<N>(y);
      cls = zero ? kMemberIdentity : a_on_curve<N>(x, y) ? kMemberOutside : kMemberInvalid;
      A::to_el(V.X, x);
      A::to_el(V.Y, y);
    }
    const el one = G::one_el();
    A::lds_put(G::SLOT_Z, one);
    A::lds_put(G::SLOT_ZZ, one);
    for (int m = c_a.rbits - 2; m >= 1; m--) {
      if ((m & 7) == 0) pbc_fair_tick<PBC_A_FAIR_BIT>();
      G::ec_dbl(V);
      const int d = r_digit<ROfA>(m);
      if (d) {
        el Px, Py;
        load_point(Px, Py, in, d < 0);
        G::ec_madd(V, Px, Py);
      }
    }
    G::ec_dbl(V);                      // V = [r - 1] P
    el Px, nPy, t0, H, R, Zf;
    load_point(Px, nPy, in, true);
    A::muls(t0, Px, G::SLOT_ZZ);
    A::subk(H, t0, V.X, G::K16);
    A::norm(H, H);
    A::lds_get(t0, G::SLOT_Z);
    A::muls(t0, t0, G::SLOT_ZZ);
    A::mul(t0, nPy, t0);
    A::subk(R, t0, V.Y, G::K16);
    A::norm(R, R);
    A::mul(H, H, one);                 // (a product brings the differences back to the class whose words can be read)
    A::mul(R, R, one);
    A::lds_get(Zf, G::SLOT_Z);
    const bool z0 = G::is0(Zf), inside = G::is0(H) & G::is0(R) & !z0;
    flag = cls == kMemberOutside && z0;
    return cls != kMemberOutside ? cls : inside ? kMemberInside : kMemberOutside;
  }
  // GT = F_q^2: x^r for an x of norm 1 with the Lucas ladder of element_pow_zn (GAL::gt_pow_lane, which tests the norm and
  // reports any other element: `flag`, for gt_member_lane).  The ladder takes its exponent as a big-endian record: r's
  // bytes, rebuilt from the signed digits ((plus | 1) - minus, byte by byte with one borrow).
  static PBC_DEV uint8_t gt_fast_lane(const uint8_t *in, int zlen, bool &flag) {
    constexpr int NB = 4 * N;
    __attribute__((aligned(16))) uint8_t zb[4 * N + 8], o[2 * NB];
    int borrow = 0;
    for (int i = 0; i < zlen; i++) {
      const int p = (int) ((c_a.r[i >> 2] >> (8 * (i & 3))) & 0xff) | (i == 0), mi = (int) ((c_a.rm[i >> 2] >> (8 * (i & 3))) & 0xff);
      const int d = p - mi - borrow;
      zb[zlen - 1 - i] = (uint8_t) (d & 0xff);
      borrow = d < 0;
    }
    for (int i = 0; i < 2 * NB; i++) o[i] = 0;
    fp2<N> x, id, w;
    a_gt_load<N>(x, in);
    GtA<N>::one(id);
    const bool zero = fp_is0<N>(x.x) & fp_is0<N>(x.y), is_one = fp_eq<N>(x.x, id.x) & fp_eq<N>(x.y, id.y);
    const bool unitary = G::gt_pow_lane(o, in, zb, zlen);
    a_gt_load<N>(w, o);
    const bool inside = fp_eq<N>(w.x, id.x) & fp_eq<N>(w.y, id.y);
    flag = !zero & !is_one & !unitary;
    return zero ? kMemberInvalid : is_one ? kMemberIdentity : (unitary & inside) ? kMemberInside : kMemberOutside;
  }
};

// ---- GT over a field policy G (group_ops.cuh: GtA / GtE / GtD / GtF) ------------------------------------------------------------
// Field elements are compared, not their byte images: G::load takes a record into Montgomery words through a product,
// which reduces every coordinate to [0, q), so the word image of an element is unique (coddh_verdict_lane states the same).
template <class G>
PBC_DEV bool gt_member_eq(const typename G::el &a, const typename G::el &b) {
  uint32_t wa[G::WORDS_EL], wb[G::WORDS_EL], diff = 0;
  G::to_words(wa, a);
  G::to_words(wb, b);
  for (int k = 0; k < G::WORDS_EL; k++) diff |= wa[k] ^ wb[k];
  return diff == 0;
}
template <class G, class RP>
PBC_DEV uint8_t gt_member_lane(const uint8_t *in) {
  typedef typename G::el el;
  el x, id, acc;
  G::load(x, in);
  G::one(id);
  G::one(acc);
  bool zero;
  {
    uint32_t w[G::WORDS_EL], any = 0;
    G::to_words(w, x);
    for (int k = 0; k < G::WORDS_EL; k++) any |= w[k];
    zero = any == 0;
  }
  const bool is_one = gt_member_eq<G>(x, id);
  // acc = x^r, low bit first: bit i of r = (plus | 1) - minus is p ^ m ^ borrow (wave-uniform)
  const int nb = RP::bits();
  uint32_t borrow = 0;
  for (int i = 0; i < nb; i++) {
    const uint32_t p = RP::plus(i) | (uint32_t) (i == 0), m = RP::minus(i), bit = p ^ m ^ borrow;
    borrow = (~p & (m | borrow) & 1u) | (p & m & borrow);
    if (bit) G::mul(acc, acc, x);
    if (i + 1 < nb) G::mul(x, x, x);
  }
  const bool inside = gt_member_eq<G>(acc, id);
  return zero ? kMemberInvalid : is_one ? kMemberIdentity : inside ? kMemberInside : kMemberOutside;
}

}  // namespace pbc
