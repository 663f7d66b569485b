// cmp_plan.h -- the integer behind element_cmp on G2 of types d, g and f (include/pbc_hip.h pbc_hip_element_cmp_batch).
// The reference treats points of those twists as coset representatives (ecc/curve.c:29-33): curve_cmp (ecc/curve.c:375-391)
// raises a - b to quotient_cmp and tests for O.  quotient_cmp is #E'(F_q^d) / r for types d and g (ecc/d_param.c:1060-1069,
// ecc/g_param.c:1336) and #E(F_q^12) / r^2 for type f (ecc/f_param.c:388-398), with the curve order of an extension from
// the trace recurrence of pbc_mpz_curve_order_extn: t_0 = 2, t_1 = t, t_(j+1) = t t_j - q t_(j-1), #E(F_q^k) = q^k + 1 - t_k.
// Pure host code, no HIP: the library, pbc_hip_diag_quotient_cmp and the tests' stand-alone program share it.
//
// The kernels walk gcd(quotient_cmp, #twist): a twist point's order divides #twist, so [quotient_cmp] D = O iff
// [gcd] D = O.  On types d / g the gcd is quotient_cmp itself; on type f, #twist = r (2q - r) and the gcd drops from
// ~q^12 / r^2 to the twist's cofactor where that divides quotient_cmp (the reference's "TODO: We can use a smaller
// quotient_cmp").
#pragma once
#include "hostbn.h"

namespace pbc_host {

struct SBig {                          // sign and magnitude (zero is never negative)
  Big m;
  bool neg = false;
};
inline SBig sbig_sub(const SBig &a, const SBig &b) {     // a - b
  SBig r;
  if (a.neg != b.neg) { r.m = Big::add(a.m, b.m); r.neg = a.neg; }
  else if (Big::cmp(a.m, b.m) >= 0) { r.m = a.m; r.m.sub(b.m); r.neg = a.neg; }
  else { r.m = b.m; r.m.sub(a.m); r.neg = !a.neg; }
  if (r.m.is_zero()) r.neg = false;
  return r;
}
inline SBig sbig_mul(const SBig &a, const SBig &b) {
  SBig r;
  r.m = Big::mul(a.m, b.m);
  r.neg = !r.m.is_zero() && a.neg != b.neg;
  return r;
}
// #E(F_q^k) for a curve over F_q of trace t (k >= 1)
inline Big curve_order_extn(const Big &q, const SBig &t, int k) {
  SBig prev, cur = t, sq;
  prev.m.w.push_back(2);
  sq.m = q;
  for (int j = 1; j < k; j++) {
    SBig next = sbig_sub(sbig_mul(t, cur), sbig_mul(sq, prev));
    prev = cur;
    cur = next;
  }
  SBig qk;
  qk.m.w.push_back(1);
  for (int j = 0; j < k; j++) qk.m = Big::mul(qk.m, q);
  qk.m.add_small(1);
  return sbig_sub(qk, cur).m;          // positive: within the Hasse interval of q^k + 1
}
inline Big big_gcd(Big a, Big b) {
  while (!b.is_zero()) {
    Big rem;
    (void) Big::div(a, b, &rem);
    a = b;
    b = rem;
  }
  return a;
}
inline void big_to_bytes(const Big &v, std::vector<uint8_t> &out) {      // big-endian magnitude, no leading zero byte
  out.clear();
  for (int i = (v.bits() + 7) / 8 - 1; i >= 0; i--) out.push_back((uint8_t) (v.w[(size_t) i >> 2] >> (8 * (i & 3))));
}

// quotient_cmp (which = 0) or the integer the kernels walk (which = 1) for the parameter text of a type d, g or f
// pairing; false: another type, a key missing, or a division that is not exact
inline bool cmp_quotient(const char *txt, size_t len, int which, std::vector<uint8_t> &out) {
  out.clear();
  std::string type;
  Big q, r, rem;
  if (!param_lookup(txt, len, "type", type) || !param_big(txt, len, "q", q) || !param_big(txt, len, "r", r) || r.is_zero()) return false;
  Big twist, quot;
  if (type == "d" || type == "g") {
    Big n, qp1 = q;
    int k = 0;
    if (!param_big(txt, len, "n", n) || !param_int(txt, len, "k", k) || k < 2 || (k & 1)) return false;
    qp1.add_small(1);
    SBig t, a, b;                      // the twist's trace: -(q + 1 - n)
    a.m = n;
    b.m = qp1;
    t = sbig_sub(a, b);
    twist = curve_order_extn(q, t, k / 2);
    quot = Big::div(twist, r, &rem);
    if (!rem.is_zero()) return false;
  } else if (type == "f") {
    Big qp1 = q, two;
    qp1.add_small(1);
    if (Big::cmp(qp1, r) < 0) return false;
    SBig t;
    t.m = qp1;
    t.m.sub(r);                        // q - r + 1
    quot = Big::div(curve_order_extn(q, t, 12), r, &rem);
    if (!rem.is_zero()) return false;
    quot = Big::div(quot, r, &rem);
    if (!rem.is_zero()) return false;
    two.w.push_back(2);
    twist = Big::mul(q, two);
    if (Big::cmp(twist, r) < 0) return false;
    twist.sub(r);
    twist = Big::mul(twist, r);        // #E'(F_q^2) = r (2q - r)
  } else {
    return false;
  }
  big_to_bytes(which ? big_gcd(quot, twist) : quot, out);
  return true;
}

}  // namespace pbc_host
