// group_gtdiv.cuh -- element_invert / element_div on GT and element_cmp on every group (include/pbc_hip.h
// pbc_hip_element_invert_GT_batch, pbc_hip_element_div_GT_batch, pbc_hip_element_cmp_batch).  Reference: element_invert /
// element_div (include/pbc_field.h:394, :324) -> mulg_invert / mulg_div (ecc/pairing.c:203-209) on GT; element_cmp
// (include/pbc_field.h:424) -> fp_cmp, fq_cmp, polymod_cmp, point_cmp, and curve_cmp (ecc/curve.c:375-391) on the twists
// of types d, g, f, whose points are coset representatives (ecc/curve.c:29-33).  One unit per lane.
//
// GT inverse.  GT = K[w] / (w^2 - c) over its half-degree subfield K (types a / a1: K = F_q, w = i; types d / g:
// K = F_q^d, w = sqrt(nqr); type f: K = F_q^2[Y] / (Y^3 + alpha) with Y = X^2, w = X).  With conj the map w -> -w and
// N(a) = a conj(a) in K:  a^-1 = conj(a) N(a)^-1.  Every pairing value has passed the easy part of the final
// exponentiation, so N(a) = 1 and the inverse IS the conjugate: the lane tests N(a) == 1 and only a lane that fails the
// test (or every lane, `generic`: "hip_group_slow 1") runs the inversion in K -- behind a branch, so a wave of pairing
// values never enters it.  Type e has GT = F_q and no such subfield: conj(a) = 1, N(a) = a, and every element but 1
// takes fp_inv.  Division is a conj(b) times N(b)^-1 under the same test.  0 has N = 0 and conj = 0: the zero record.
//
// Coset compare.  D = a - b on the complete affine law; D = O: equal.  Otherwise V = [c - 1] D by the walks of
// group_mpz.cuh over the shared digits of c - 1 (c: cmp_plan.h) and the end test of group_member.cuh: [c] D = O iff
// V = -D, read off projectively (X_V = x Z^2, Y_V = -y Z^3, Z != 0) -- no inversion, and not confused with an exceptional
// step.  The fast walk reports itself (Z = 0, or a table that met an exceptional step); those lanes are redone on the
// complete law over the same digits, where Z = 0 is the honest V = O (then [c] D = D != O).
#pragma once
#include "group_mpz.cuh"

namespace pbc {

// ---- the half-degree subfield of a GT policy (group_ops.cuh GtA / GtE / GtD / GtF) ----------------------------------------------
// sub, conj(r, a), norm(n, a, conj a), is_one(n), inv(r, n), scale(r, a, s) = a s for s in the subfield (r may be a)
template <class G> struct GtHalf;
template <int N>
struct GtHalf<GtA<N>> {
  typedef fp2<N> el;
  typedef fp<N> sub;
  static PBC_DEV void conj(el &r, const el &a) { r.x = a.x; fp_neg<N>(r.y, a.y); }
  static PBC_DEV void norm(sub &n, const el &a, const el &) { fp<N> t; fp_sqr<N>(n, a.x); fp_sqr<N>(t, a.y); fp_add<N>(n, n, t); }
  static PBC_DEV bool is_one(const sub &n) { fp<N> o; fp_set<N>(o, fpk<N>().one); return fp_eq<N>(n, o); }
  static PBC_DEV void inv(sub &r, const sub &n) { fp_inv<N>(r, n); }
  static PBC_DEV void scale(el &r, const el &a, const sub &s) { fp_mul<N>(r.x, a.x, s); fp_mul<N>(r.y, a.y, s); }
};
template <int N>
struct GtHalf<GtE<N>> {
  typedef fp<N> el;
  typedef fp<N> sub;
  static PBC_DEV void conj(el &r, const el &) { fp_set<N>(r, fpk<N>().one); }
  static PBC_DEV void norm(sub &n, const el &a, const el &) { n = a; }
  static PBC_DEV bool is_one(const sub &n) { fp<N> o; fp_set<N>(o, fpk<N>().one); return fp_eq<N>(n, o); }
  static PBC_DEV void inv(sub &r, const sub &n) { fp_inv<N>(r, n); }
  static PBC_DEV void scale(el &r, const el &a, const sub &s) { fp_mul<N>(r, a, s); }
};
template <int N, int DEG>
struct GtHalf<GtD<N, DEG>> {
  typedef TypeMNT<N, DEG> T;
  typedef typename T::f6 el;
  typedef typename T::f3 sub;
  static PBC_DEV void conj(el &r, const el &a) { r.x = a.x; T::f3_neg(r.y, a.y); }
  static PBC_DEV void norm(sub &n, const el &a, const el &) {      // x^2 - nqr y^2
    sub t;
    T::f3_sqr(n, a.x);
    T::f3_sqr(t, a.y);
    T::f3_mul_v(t, t);
    T::f3_sub(n, n, t);
  }
  static PBC_DEV bool is_one(const sub &n) { const sub o = FdOps<N, DEG>::one(); return T::f3_eq(n, o); }
  static PBC_DEV void inv(sub &r, const sub &n) { T::f3_inv(r, n); }
  static PBC_DEV void scale(el &r, const el &a, const sub &s) { T::f3_mul(r.x, a.x, s); T::f3_mul(r.y, a.y, s); }
};
template <int ND>
struct GtHalf<GtF<ND>> {
  typedef TypeF<ND> T;
  typedef typename T::f12 el;
  typedef typename T::g2 g2;
  struct sub { g2 c[3]; };             // c0 + c1 Y + c2 Y^2, Y = X^2, Y^3 = negalpha: the even coefficients of an f12
  static PBC_DEV void conj(el &r, const el &a) { T::f12_conj(&r, &a); }
  static PBC_DEV void norm(sub &n, const el &a, const el &ca) {
    el p;
    T::f12_mul(&p, &a, &ca);           // (the odd coefficients of a conj(a) vanish)
    for (int i = 0; i < 3; i++) n.c[i] = p.c[2 * i];
  }
  static PBC_DEV bool is_one(const sub &n) {
    const g2 o = Fq2Ops<ND>::one();
    return T::g2_eq(n.c[0], o) & Fq2Ops<ND>::is0(n.c[1]) & Fq2Ops<ND>::is0(n.c[2]);
  }
  // (a + b Y + c Y^2)^-1 = (A + B Y + C Y^2) / (a A + xi (c B + b C)),  A = a^2 - xi b c, B = xi c^2 - a b, C = b^2 - a c
  static PBC_DEV void inv(sub &r, const sub &n) {
    const g2 xi = T::fk2(c_f.negalpha);
    g2 A, B, C, t, u;
    T::g2_mul(t, n.c[1], n.c[2]);
    T::g2_mul(t, t, xi);
    T::g2_sqr(A, n.c[0]);
    T::g2_sub(A, A, t);
    T::g2_sqr(B, n.c[2]);
    T::g2_mul(B, B, xi);
    T::g2_mul(t, n.c[0], n.c[1]);
    T::g2_sub(B, B, t);
    T::g2_sqr(C, n.c[1]);
    T::g2_mul(t, n.c[0], n.c[2]);
    T::g2_sub(C, C, t);
    T::g2_mul(t, n.c[2], B);
    T::g2_mul(u, n.c[1], C);
    T::g2_add(t, t, u);
    T::g2_mul(t, t, xi);
    T::g2_mul(u, n.c[0], A);
    T::g2_add(t, t, u);
    T::g2_inv(t, t);
    T::g2_mul(r.c[0], A, t);
    T::g2_mul(r.c[1], B, t);
    T::g2_mul(r.c[2], C, t);
  }
  static PBC_DEV void scale(el &r, const el &a, const sub &s) {
    el e;
    for (int i = 0; i < 3; i++) { e.c[2 * i] = s.c[i]; T::g2_zero(e.c[2 * i + 1]); }
    T::f12_mul(&r, &a, &e);
  }
};

// out = a^-1.  Returns whether the lane ran the inversion (the host mirror reports it; the kernels ignore it).
template <class G>
PBC_DEV bool gt_invert_lane(uint8_t *out, const uint8_t *a, bool generic) {
  typedef GtHalf<G> H;
  typename G::el x, r;
  typename H::sub n;
  G::load(x, a);
  H::conj(r, x);
  H::norm(n, x, r);
  const bool slow = generic | !H::is_one(n);
  if (slow) {
    H::inv(n, n);
    H::scale(r, r, n);
  }
  G::store(out, r);
  return slow;
}
// out = a / b = a conj(b) N(b)^-1
template <class G>
PBC_DEV bool gt_div_lane(uint8_t *out, const uint8_t *a, const uint8_t *b, bool generic) {
  typedef GtHalf<G> H;
  typename G::el x, y, r;
  typename H::sub n;
  G::load(x, a);
  G::load(y, b);
  H::conj(r, y);
  H::norm(n, y, r);
  G::mul(r, x, r);
  const bool slow = generic | !H::is_one(n);
  if (slow) {
    H::inv(n, n);
    H::scale(r, r, n);
  }
  G::store(out, r);
  return slow;
}

// ---- element_cmp: 0 equal, 1 not (element_cmp's own convention) -------------------------------------------------------------------
// Z_r: the kernel runs on the constant block whose modulus is r (host_params.h zr_kargs), as zr_op_lane
template <int N>
PBC_DEV uint8_t zr_cmp_lane(const uint8_t *a, const uint8_t *b) {
  fp<N> x, y;
  fp_load_be<N>(x, a);
  fp_load_be<N>(y, b);
  return fp_eq<N>(x, y) ? 0 : 1;
}
template <class G>
PBC_DEV uint8_t gt_cmp_lane(const uint8_t *a, const uint8_t *b) {
  typename G::el x, y;
  G::load(x, a);
  G::load(y, b);
  return gt_member_eq<G>(x, y) ? 0 : 1;
}
// G1, and G2 of the symmetric types (point_cmp): records read as element_add reads them (ec_load_affine: off the curve and
// the all-zero record are O); O equals O and differs from every finite point
template <class F>
PBC_DEV uint8_t ec_cmp_plain_lane(const uint8_t *a, const uint8_t *b) {
  typename F::el x1, y1, x2, y2;
  const bool f1 = ec_load_affine<F>(x1, y1, a), f2 = ec_load_affine<F>(x2, y2, b);
  const bool same = f1 & f2 & F::eq(x1, x2) & F::eq(y1, y2), both_inf = !f1 & !f2;
  return (same | both_inf) ? 0 : 1;
}
// D = a - b; false: D = O
template <class F>
PBC_DEV bool ec_cmp_diff(typename F::el &x, typename F::el &y, const uint8_t *a, const uint8_t *b) {
  typename F::el x1, y1, x2, y2;
  const bool f1 = ec_load_affine<F>(x1, y1, a), f2 = ec_load_affine<F>(x2, y2, b);
  F::sub(y2, F::zero(), y2);
  bool f3;
  ec_add_affine<F>(x, y, f3, x1, y1, f1, x2, y2, f2);
  return f3;
}
// (X : Y : Z) is the finite point -(x, y)
template <class F>
PBC_DEV bool ec_cmp_is_neg(const typename F::el &X, const typename F::el &Y, const typename F::el &Z, const typename F::el &x, const typename F::el &y) {
  typename F::el zz, t, u, ny = F::zero();
  F::sub(ny, ny, y);
  F::sqr(zz, Z);
  F::mul(t, x, zz);
  F::mul(u, zz, Z);
  F::mul(u, ny, u);
  return F::eq(t, X) & F::eq(u, Y) & !F::is0(Z);
}
// dig / nd: the digits of c - 1 (width W); `flag`: the verdict is not final, the lane needs ec_cmp_complete_lane
template <class F, int W>
PBC_DEV uint8_t ec_cmp_fast_lane(const uint8_t *a, const uint8_t *b, const uint32_t *dig, int nd, bool &flag) {
  typename F::el x, y, X, Y, Z;
  const bool finite = ec_cmp_diff<F>(x, y, a, b);
  const bool bad = ec_mpz_fast_walk<F, W>(X, Y, Z, x, y, dig, nd);
  flag = finite & bad;
  return (finite & !ec_cmp_is_neg<F>(X, Y, Z, x, y)) ? 1 : 0;
}
template <class F>
PBC_DEV uint8_t ec_cmp_complete_lane(const uint8_t *a, const uint8_t *b, const uint32_t *dig, int nd, int w) {
  typename F::el x, y, X, Y, Z;
  const bool finite = ec_cmp_diff<F>(x, y, a, b);
  ec_mpz_complete_walk<F>(X, Y, Z, x, y, dig, nd, w);
  return (finite & !ec_cmp_is_neg<F>(X, Y, Z, x, y)) ? 1 : 0;
}

}  // namespace pbc
