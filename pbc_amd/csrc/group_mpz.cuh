// group_mpz.cuh -- element_mul_mpz / element_pow_mpz over a batch that shares ONE integer (include/pbc_hip.h
// pbc_hip_element_mul_mpz_batch): out[i] = [k] in[i] on G1 / G2, in[i]^k on GT, for a non-negative k of any length up to
// PBC_HIP_MPZ_MAX_BYTES.  Reference: element_mul_mpz / element_pow_mpz (include/pbc_field.h:292, :365) -> curve.c:713
// (f->mul_mpz = element_pow_mpz) -> generic_pow_mpz (arith/field.c:113-126: k as it stands, never reduced mod r; k = 0
// gives the identity whatever the base, :117), on GT ecc/pairing.c:215,266,274.  Group elements are unique, so any
// addition chain gives the reference's bytes.
//
// One unit per lane; the integer is the same for every lane, so its digits are WAVE-UNIFORM: the host recodes k once
// (mpz_plan.h: width-w NAF for points, plain bits for GT), uploads the string, and passes its LENGTH as a kernel
// argument.  A lane reads digit m through a uniform address in the constant address space -- a scalar load, a scalar
// branch on it -- and the ladder pays one doubling per digit and one addition only where the shared digit is non-zero
// (element_mul_zn's per-lane scalars force a regular ladder: an addition in every window, selects instead of branches).
//
// Points.  The FAST lane is element_mul_zn's: incomplete Jacobian steps, Z = 0 sticks, "Z = 0 at the end" is reported
// and nothing is written -- the result O, k a multiple of the point's order, a point of small order, an accumulator that
// meets +-(a table entry).  W = 2: no table, +-P is added.  W > 2: a per-lane table of the odd multiples P, 3P, ...,
// (2^(W-1) - 1) P, affine through one batched inversion (the construction of ec_mul_win_lane), in private memory, indexed
// by the uniform digit.  The same lane exists on the limb-form steps of the 512-bit type a field (MpzAL) and of G1 of the
// five-word fields (MpzL5).  The COMPLETE lane redoes a reported lane over the SAME digits on the complete law (ec_dbl_jac /
// ec_madd_jac with the case analysis): a width-w digit d at position p is followed by w - 1 zeros, so the bits of |d|,
// signed, occupy positions p .. p + w - 2 on their own, and the string reads as digits -1, 0, +1 without a table.
// One inversion per unit makes the result affine; O is zero bytes; an off-curve record is O (curve_from_bytes).
//
// GT.  Square-and-multiply over the bits of k from the top, for ANY field element: x^0 = 1 (also 0^0), 0^k = 0.  The
// 512-bit type a field powers elements of norm 1 with the Lucas ladder of element_pow_zn (group_al.cuh gt_pow_lane) on
// the uniform bits; the ladder tests its precondition per lane and reports every other element for the generic power.
// (Type f on the five-word field: a dense k that fits a Z_r record runs element_pow_zn's cyclotomic lane, unchanged, on
// that one record -- pbc_hip_mpz.hip f_mpz_gtpow_kernel, mpz_plan.h mpz_gt_wants_record -- with the same fallback.)
#pragma once
#include "group_member.cuh"
#include "group_l5.cuh"

namespace pbc {

// digit m of the uploaded string (int8, four to a word; m < the length the host passed -- the buffer is padded to whole words)
PBC_DEV int mpz_digit(const uint32_t *dig, int m) {
#ifndef PBC_HOSTSIM
  const uint32_t w = (uint32_t) __builtin_amdgcn_readfirstlane((int) ((const __attribute__((address_space(4))) uint32_t *) dig)[m >> 2]);
#else
  const uint32_t w = dig[m >> 2];
#endif
  return (int) (int8_t) (uint8_t) (w >> (8 * (m & 3)));
}
// The string as digits -1, 0, +1 (the complete lane): position m in [0, nd + w - 2) carries bit j of |d_(m-j)| with d's
// sign, for the one j < w - 1 whose digit is non-zero (w = 2: the digit itself).
PBC_DEV int mpz_signed_bit(const uint32_t *dig, int nd, int w, int m) {
  int sd = 0;
  for (int j = 0; j < w - 1; j++) {
    const int p = m - j;
    if (p < 0 || p >= nd) continue;
    const int d = mpz_digit(dig, p), a = d < 0 ? -d : d;
    if ((a >> j) & 1) sd = d < 0 ? -1 : 1;
  }
  return sd;
}

// (x, y) of a record: reduced mod q on load; `valid`: on the curve (curve_is_valid_point)
template <class F>
PBC_DEV bool ec_mpz_load(typename F::el &x, typename F::el &y, const uint8_t *in) {
  typename F::el t0, t1;
  F::load(x, in);
  F::load(y, in + F::bytes());
  F::sqr(t0, x);
  F::add(t0, t0, F::curve_a());
  F::mul(t0, t0, x);
  F::add(t0, t0, F::curve_b());
  F::sqr(t1, y);
  return F::eq(t0, t1);
}
// (X : Y : Z) -> affine bytes; `inf`: write O
template <class F>
PBC_DEV void ec_mpz_store(uint8_t *out, const typename F::el &X, const typename F::el &Y, const typename F::el &Z, bool inf) {
  typename F::el zi, zz, ax, ay;
  F::inv(zi, Z);
  F::sqr(zz, zi);
  F::mul(ax, X, zz);
  F::mul(zz, zz, zi);
  F::mul(ay, Y, zz);
  if (inf) { ax = F::zero(); ay = ax; }
  F::store(out, ax);
  F::store(out + F::bytes(), ay);
}

// The walk of the fast lane over a field policy F (group_ops.cuh: FqOps; FdOps / Fq2Ops on the twists), digits of width W:
// (X : Y : Z) = [k] (px, py) on the incomplete steps.  Returns true -- `bad` -- when the result cannot be trusted: k = 0,
// a table that met an exceptional step, Z = 0 at the end.  (The coset compare of group_gtdiv.cuh walks with it too.)
template <class F, int W>
PBC_DEV bool ec_mpz_fast_walk(typename F::el &X, typename F::el &Y, typename F::el &Z, const typename F::el &px, const typename F::el &py,
                              const uint32_t *dig, int nd) {
  typedef typename F::el el;
  constexpr int TE = 1 << (W - 2);     // odd multiples 1, 3, ..., 2 TE - 1
  const el one = F::one(), ca = F::curve_a();
  el tab[TE][2];
  tab[0][0] = px;
  tab[0][1] = py;
  bool bad = nd == 0;                  // k = 0: O, left to the complete lane like every other O
  if constexpr (TE > 1) {
    // 2P = (X2 : Y2 : Z2); on the isomorphic curve where 2P is affine the odd multiples follow by mixed additions and go
    // back by Z <- Z Z2; one batched inversion (ec_mul_win_lane)
    el zs[TE], cs[TE];
    X = tab[0][0]; Y = tab[0][1]; Z = one;
    ec_dbl_jac<F>(X, Y, Z, ca);
    const el X2 = X, Y2 = Y, Z2 = Z;
    {
      el zz, t;
      F::sqr(zz, Z2);
      F::mul(X, tab[0][0], zz);
      F::mul(t, zz, Z2);
      F::mul(Y, tab[0][1], t);
      Z = one;
    }
    for (int j = 1; j < TE; j++) {
      ec_madd_inc<F>(X, Y, Z, X2, Y2);
      tab[j][0] = X;
      tab[j][1] = Y;
      F::mul(zs[j], Z, Z2);
      if (j == 1) cs[1] = zs[1];
      else F::mul(cs[j], cs[j - 1], zs[j]);
    }
    bad |= F::is0(cs[TE - 1]);
    el zi;
    F::inv(zi, cs[TE - 1]);
    for (int j = TE - 1; j >= 1; j--) {
      el zinv, zz, t;
      if (j > 1) {
        F::mul(zinv, zi, cs[j - 1]);
        F::mul(zi, zi, zs[j]);
      } else {
        zinv = zi;
      }
      F::sqr(zz, zinv);
      F::mul(tab[j][0], tab[j][0], zz);
      F::mul(t, zz, zinv);
      F::mul(tab[j][1], tab[j][1], t);
    }
  }
  {
    int top = 0;                       // the top digit is positive
    if constexpr (TE > 1) top = nd ? (mpz_digit(dig, nd - 1) - 1) >> 1 : 0;
    X = tab[top][0];
    Y = tab[top][1];
    Z = one;
  }
  for (int m = nd - 2; m >= 0; m--) {
    ec_dbl_jac<F>(X, Y, Z, ca);
    const int d = mpz_digit(dig, m);   // (wave-uniform)
    if (d) {
      int idx = 0;
      if constexpr (TE > 1) idx = ((d < 0 ? -d : d) - 1) >> 1;
      el y2 = tab[idx][1];
      if (d < 0) { el ny = F::zero(); F::sub(ny, ny, y2); y2 = ny; }
      ec_madd_inc<F>(X, Y, Z, tab[idx][0], y2);
    }
  }
  return bad | F::is0(Z);
}
// The fast lane.  Returns false -- nothing written -- when the lane needs ec_mpz_complete_lane.
template <class F, int W>
PBC_DEV bool ec_mpz_fast_lane(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd) {
  typedef typename F::el el;
  el x, y, X, Y, Z;
  const bool valid = ec_mpz_load<F>(x, y, in);
  const bool bad = ec_mpz_fast_walk<F, W>(X, Y, Z, x, y, dig, nd);
  const bool handled = !valid | !bad;
  if (handled) ec_mpz_store<F>(out, X, Y, Z, !valid);
  return handled;
}
// The walk of the complete lane: (X : Y : Z) = [k] (x, y) for any point of the curve and any k; the same digits read as
// -1, 0, +1 (mpz_signed_bit), the accumulator from O, every addition with the case analysis of ec_madd_jac (V = O, V = -P,
// V = P through the double formed beforehand; the double of -P is that of P with Y negated).  Z = 0: the result is O.
template <class F>
PBC_DEV void ec_mpz_complete_walk(typename F::el &X, typename F::el &Y, typename F::el &Z, const typename F::el &x, const typename F::el &y,
                                  const uint32_t *dig, int nd, int w) {
  typedef typename F::el el;
  el ny = F::zero();
  F::sub(ny, ny, y);
  const el one = F::one(), ca = F::curve_a();
  el DX = x, DY = y, DZ = one, nDY = F::zero();
  ec_dbl_jac<F>(DX, DY, DZ, ca);
  F::sub(nDY, nDY, DY);
  X = one;
  Y = one;
  Z = F::zero();
  for (int m = nd ? nd + w - 3 : -1; m >= 0; m--) {
    ec_dbl_jac<F>(X, Y, Z, ca);
    const int d = mpz_signed_bit(dig, nd, w, m);
    if (d > 0) ec_madd_jac<F>(X, Y, Z, x, y, DX, DY, DZ, true);
    else if (d < 0) ec_madd_jac<F>(X, Y, Z, x, ny, DX, nDY, DZ, true);
  }
}
// The complete lane
template <class F>
PBC_DEV void ec_mpz_complete_lane(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd, int w) {
  typedef typename F::el el;
  el x, y, X, Y, Z;
  const bool valid = ec_mpz_load<F>(x, y, in);
  ec_mpz_complete_walk<F>(X, Y, Z, x, y, dig, nd, w);
  ec_mpz_store<F>(out, X, Y, Z, F::is0(Z) | !valid);
}

// ---- the 512-bit type a field: the fast lane on the limb-form steps of element_mul_zn (group_al.cuh ec_dbl / ec_madd) ----------
// V = (X, Y) in registers, Z and Z^2 in the lane's LDS slots.  W = 2: no table, and P is not kept across the ladder -- the
// record is read again where +-P is added (MemberAL::load_point), so the doubling chain runs on the registers of ec_dbl.
// W > 2: the table of GAL::gmul_lane (private memory, affine through one batched inversion), indexed by the uniform digit.
template <int N>
struct MpzAL {
  typedef GAL<N> G;
  typedef AL<N> A;
  typedef typename A::el el;
  typedef typename A::jacl jacl;
  // out: the lane's private staging (al_gmul_kernel's `o`); false: nothing written, the lane needs the complete routine
  template <int W>
  static PBC_DEV bool fast_lane(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd) {
    constexpr int NB = 4 * N, TE = 1 << (W - 2);
    bool valid, bad = nd == 0;
    jacl V;
    el tab[TE][2];
    {
      fp<N> x, y;
      fp_load_be<N>(x, in);
      fp_load_be<N>(y, in + NB);
      valid = a_on_curve<N>(x, y);
      A::to_el(tab[0][0], x);
      A::to_el(tab[0][1], y);
    }
    const el one = G::one_el();
    V.X = tab[0][0];
    V.Y = tab[0][1];
    A::lds_put(G::SLOT_Z, one);
    A::lds_put(G::SLOT_ZZ, one);
    if constexpr (TE > 1) {
      el Z2, zs[TE], cs[TE];
      G::ec_dbl(V);                    // 2P = (X2 : Y2 : Z2)
      const el X2 = V.X, Y2 = V.Y;
      A::lds_get(Z2, G::SLOT_Z);
      {
        el zz, t;
        A::lds_get(zz, G::SLOT_ZZ);
        A::mul(V.X, tab[0][0], zz);
        A::mul(t, zz, Z2);
        A::mul(V.Y, tab[0][1], t);
        A::lds_put(G::SLOT_Z, one);
        A::lds_put(G::SLOT_ZZ, one);
      }
      for (int j = 1; j < TE; j++) {
        el zj;
        G::ec_madd(V, X2, Y2);
        tab[j][0] = V.X;
        tab[j][1] = V.Y;
        A::lds_get(zj, G::SLOT_Z);
        A::mul(zs[j], zj, Z2);
        if (j == 1) cs[1] = zs[1];
        else A::mul(cs[j], cs[j - 1], zs[j]);
      }
      bad |= G::is0(cs[TE - 1]);
      el zi;
      G::inv(zi, cs[TE - 1]);
      for (int j = TE - 1; j >= 1; j--) {
        el zinv, zz, t, X, Y;
        if (j > 1) {
          A::mul(zinv, zi, cs[j - 1]);
          A::mul(zi, zi, zs[j]);
        } else {
          zinv = zi;
        }
        A::sqr(zz, zinv);
        X = tab[j][0];
        Y = tab[j][1];
        AL_HS(A::hs_set(X, A::U_ALMOST, 8.0); A::hs_set(Y, A::U_ALMOST, 8.0);)
        A::mul(tab[j][0], X, zz);
        A::mul(t, zz, zinv);
        A::mul(tab[j][1], Y, t);
      }
      const int top = nd ? (mpz_digit(dig, nd - 1) - 1) >> 1 : 0;    // the top digit is positive
      V.X = tab[top][0];
      V.Y = tab[top][1];
      AL_HS(A::hs_set(V.X, A::U_STRICT, 1.5); A::hs_set(V.Y, A::U_STRICT, 1.5);)
      A::lds_put(G::SLOT_Z, one);
      A::lds_put(G::SLOT_ZZ, one);
    }
    for (int m = nd - 2; m >= 0; m--) {
      if ((m & 7) == 0) pbc_fair_tick<PBC_A_FAIR_BIT>();
      G::ec_dbl(V);
      const int d = mpz_digit(dig, m);
      if (d) {
        el Px, Py;
        if constexpr (TE > 1) {
          const int idx = ((d < 0 ? -d : d) - 1) >> 1;
          Px = tab[idx][0];
          Py = tab[idx][1];
          AL_HS(A::hs_set(Px, A::U_STRICT, 1.5); A::hs_set(Py, A::U_STRICT, 1.5);)
          if (d < 0) {
            el ny;
            A::negk(ny, Py, G::K2);
            A::norm(Py, ny);
          }
        } else {
          MemberAL<N>::load_point(Px, Py, in, d < 0);
        }
        G::ec_madd(V, Px, Py);
      }
    }
    el Zf, zinv, zz, t3, ax, ay;
    A::lds_get(Zf, G::SLOT_Z);
    bad |= G::is0(Zf);
    G::inv(zinv, Zf);
    A::sqr(zz, zinv);
    A::mul(ax, V.X, zz);
    A::mul(t3, zz, zinv);
    A::mul(ay, V.Y, t3);
    fp<N> x, y;
    A::to_words(x, ax);
    A::to_words(y, ay);
    if (!valid) {
#pragma unroll
      for (int k = 0; k < N; k++) { x.v[k] = 0; y.v[k] = 0; }
    }
    const bool handled = !valid | !bad;
    if (handled) {
      fp_store_be<N>(out, x);
      fp_store_be<N>(out + NB, y);
    }
    return handled;
  }
  // GT = F_q^2: a^k for an a of norm 1 by the Lucas ladder of GAL::gt_pow_lane over the uniform BITS of k (nd of them, the
  // top one set): V_k(2 Re a) by one product and one squaring in F_q per bit, Im a^k = -(2 V_(k+1) - P V_k) / (4 Im a).
  // Returns false (nothing written) for an element of any other norm.
  static PBC_DEV bool gt_fast_lane(uint8_t *out, const uint8_t *a, const uint32_t *dig, int nd) {
    constexpr int NB = 4 * N;
    el ax, ay, P, two, v0, v1;
    bool unitary;
    {
      fp<N> x, y, one, t0, t1;
      fp_load_be<N>(x, a);
      fp_load_be<N>(y, a + NB);
      fp_set<N>(one, fpk<N>().one);
      fp_sqr<N>(t0, x);
      fp_sqr<N>(t1, y);
      fp_add<N>(t0, t0, t1);
      unitary = fp_eq<N>(t0, one);
      A::to_el(ax, x);
      A::to_el(ay, y);
      fp_dbl<N>(one, one);
      A::to_el(two, one);
    }
    A::template shl<1>(P, ax);
    A::norm(P, P);
    v0 = two;
    v1 = P;
    for (int j = nd - 1; j >= 0; j--) {
      const bool bit = mpz_digit(dig, j) != 0;       // (wave-uniform)
      el m, s;
      if ((j & 15) == 0) pbc_fair_tick<PBC_A_FAIR_BIT>();
      A::mul(m, v0, v1);
      A::subk(m, m, P, G::K4);
      A::norm(m, m);                   // V_(2n+1) = V_n V_(n+1) - P
      if (bit) s = v1; else s = v0;
      A::sqr(s, s);
      A::subk(s, s, two, G::K2);
      A::norm(s, s);                   // V_(2n+2) or V_(2n)
      if (bit) { v0 = m; v1 = s; } else { v0 = s; v1 = m; }
    }
    el t, w, yi;
    A::mul(t, v0, P);
    A::template shl<1>(v1, v1);
    A::subk(v1, v1, t, G::K2);
    A::norm(v1, v1);
    G::inv(yi, ay);
    A::mul(w, v1, yi);
    fp<N> x, y;
    A::to_words(y, w);
    fp_halve<N>(y, y);
    fp_halve<N>(y, y);
    fp_neg<N>(y, y);
    A::to_fp(x, v0);
    fp_halve<N>(x, x);
    if (unitary) {
      fp_store_be<N>(out, x);
      fp_store_be<N>(out + NB, y);
    }
    return unitary;
  }
};

// ---- G1 of the five-word fields (d159.param, f.param): the fast lane on the limb-form steps of group_l5.cuh ----------------------
// GL::dbl / GL::madd, everything in registers; W > 2: the table of GL::gmul_lane in private memory.
template <class KP>
struct MpzL5 {
  typedef GL<5, KP> L;
  typedef typename L::el el;
  template <int W>
  static PBC_DEV bool fast_lane(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd) {
    constexpr int N = 5, TE = 1 << (W - 2);
    const int NB = (int) fpk<N>().fbytes;
    const bool a_zero = c_curve.a_is_zero != 0;
    el tab[TE][2], ca, one;
    bool valid, bad = nd == 0;
    {
      fp<N> x, y, t0, t1, a, b;
      fp_load_be<N>(x, in);
      fp_load_be<N>(y, in + NB);
      fp_set<N>(a, c_curve.a);
      fp_set<N>(b, c_curve.b);
      fp_sqr<N>(t0, x);
      fp_add<N>(t0, t0, a);
      fp_mul<N>(t0, t0, x);
      fp_add<N>(t0, t0, b);
      fp_sqr<N>(t1, y);
      valid = fp_eq<N>(t0, t1);
      L::from_fq(tab[0][0], x);
      L::from_fq(tab[0][1], y);
      L::from_fq(ca, a);
      fp_set<N>(t0, fpk<N>().one);
      L::from_fq(one, t0);
    }
    el X = tab[0][0], Y = tab[0][1], Z = one;
    if constexpr (TE > 1) {
      el zs[TE], cs[TE];
      L::dbl(X, Y, Z, ca, a_zero);     // 2P = (X2 : Y2 : Z2)
      const el X2 = X, Y2 = Y, Z2 = Z;
      {
        el zz, t;
        L::template mul<4>(zz, Z2, Z2);
        L::template mul<1>(X, tab[0][0], zz);
        L::template mul<2>(t, zz, Z2);
        L::template mul<1>(Y, tab[0][1], t);
        Z = one;
      }
      for (int j = 1; j < TE; j++) {
        L::madd(X, Y, Z, X2, Y2);
        tab[j][0] = X;
        tab[j][1] = Y;
        L::template mul<2>(zs[j], Z, Z2);
        if (j == 1) cs[1] = zs[1];
        else L::template mul<1>(cs[j], cs[j - 1], zs[j]);
      }
      bad |= L::is0(cs[TE - 1]);
      el zi;
      L::inv(zi, cs[TE - 1]);
      for (int j = TE - 1; j >= 1; j--) {
        el zinv, zz, t, x, y;
        if (j > 1) {
          L::template mul<1>(zinv, zi, cs[j - 1]);
          L::template mul<1>(zi, zi, zs[j]);
        } else {
          zinv = zi;
        }
        L::sqr(zz, zinv);
        x = tab[j][0];
        y = tab[j][1];
        L::template mul<1>(tab[j][0], x, zz);
        L::template mul<1>(t, zz, zinv);
        L::template mul<1>(tab[j][1], y, t);
      }
      const int top = nd ? (mpz_digit(dig, nd - 1) - 1) >> 1 : 0;    // the top digit is positive
      X = tab[top][0];
      Y = tab[top][1];
      GL_HS(L::hs_set(X, L::U_STRICT, 2.0); L::hs_set(Y, L::U_STRICT, 2.0);)
      Z = one;
    }
    for (int m = nd - 2; m >= 0; m--) {
      L::dbl(X, Y, Z, ca, a_zero);
      const int d = mpz_digit(dig, m);   // (wave-uniform)
      if (d) {
        int idx = 0;
        if constexpr (TE > 1) idx = ((d < 0 ? -d : d) - 1) >> 1;
        el x2 = tab[idx][0], y2 = tab[idx][1];
        GL_HS(L::hs_set(x2, L::U_STRICT, 2.0); L::hs_set(y2, L::U_STRICT, 2.0);)
        if (d < 0) {
          el ny;
          L::negk(ny, y2, L::K4);      // u 3, B 4
          L::norm(y2, ny);
        }
        L::madd(X, Y, Z, x2, y2);
      }
    }
    bad |= L::is0(Z);
    el zinv, zz, t3, ax, ay;
    L::inv(zinv, Z);
    L::sqr(zz, zinv);
    L::template mul<2>(ax, X, zz);
    L::template mul<1>(t3, zz, zinv);
    L::template mul<2>(ay, Y, t3);
    fp<N> x, y;
    L::to_fq(x, ax);
    L::to_fq(y, ay);
    if (!valid) {
#pragma unroll
      for (int k = 0; k < N; k++) { x.v[k] = 0; y.v[k] = 0; }
    }
    const bool handled = !valid | !bad;
    if (handled) {
      fp_store_be<N>(out, x);
      fp_store_be<N>(out + NB, y);
    }
    return handled;
  }
};

// ---- GT over a field policy G (group_ops.cuh: GtA / GtE / GtD / GtF) ------------------------------------------------------------
// the policies' squarings (they carry products only)
template <int N> PBC_DEV void gt_mpz_sqr(GtA<N>, fp2<N> &r) { fi_sqr<N>(r, r); }
template <int N> PBC_DEV void gt_mpz_sqr(GtE<N>, fp<N> &r) { fp_sqr<N>(r, r); }
template <int N, int DEG> PBC_DEV void gt_mpz_sqr(GtD<N, DEG>, typename TypeMNT<N, DEG>::f6 &r) { TypeMNT<N, DEG>::f6_sqr(r, r); }
template <int ND> PBC_DEV void gt_mpz_sqr(GtF<ND>, typename TypeF<ND>::f12 &r) { TypeF<ND>::f12_sqr(&r, &r); }
// out = x^k over the bits of k from the top (nd bits, the top one set; nd = 0: k = 0, the result is 1 for every x)
template <class G>
PBC_DEV void gt_mpz_lane(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd) {
  typedef typename G::el el;
  el x, acc;
  G::load(x, in);
  if (nd) acc = x; else G::one(acc);
  for (int m = nd - 2; m >= 0; m--) {
    gt_mpz_sqr(G(), acc);
    if (mpz_digit(dig, m)) G::mul(acc, acc, x);      // (wave-uniform)
  }
  G::store(out, acc);
}

}  // namespace pbc
