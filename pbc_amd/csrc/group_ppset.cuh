// group_ppset.cuh -- sets of fixed-base tables on G1, G2 and GT (include/pbc_hip.h pbc_hip_element_pp_set_*): m tables of
// element_pp_init (group_ops.cuh ec_pp_entry_lane / gt_pp_entry_lane: 8-bit rows, affine Montgomery words) side by side,
// table t at tabs + t * (words of one table).  Reference: element_pp_init / element_pp_pow_zn
// (include/pbc_field.h:591-625 -> element_build_base_table / element_pow_base_table, arith/field.c:243-323) once per base
// and element_mul on the results (include/pbc_field.h:280).  Three lane bodies, one unit per lane:
//   entry     unit u -> (table, row, w): the entry and its "is O" flag, the single-base bodies with a table index
//   segmented the unit's table from the call's offsets (a per-lane binary search: the entries are per-lane gathers, so
//             nothing here has to be wave-uniform), then the single-base power on that table
//   product   sum_j [z_j] B_j: ONE Jacobian accumulator over the m * zlen entries the scalar bytes select, one inversion
#pragma once
#include "group_more.cuh"

namespace pbc {

// words of one table of a curve group / of GT
template <class F> PBC_DEV size_t ec_pp_table_words(int zlen) { return (size_t) zlen * kPpRowLen * 2 * F::WORDS_EL; }
template <class G> PBC_DEV size_t gt_pp_table_words(int zlen) { return ((size_t) zlen << kPpWin) * G::WORDS_EL; }

// unit u = t * (zlen 255) + row * 255 + (w - 1) of a set: entry (row, w) of table t and flags[u] = "the entry is O"
template <class F>
PBC_DEV void ec_pp_set_entry_lane(uint32_t *tabs, uint8_t *flags, const uint8_t *bases, int zlen, size_t u) {
  const size_t per = (size_t) zlen * kPpRowLen, t = u / per;
  ec_pp_entry_lane<F>(tabs + t * ec_pp_table_words<F>(zlen), flags + t * per, bases + t * 2 * (size_t) F::bytes(), zlen, u % per);
}
// unit u = t * (zlen 256) + row * 256 + w
template <class G>
PBC_DEV void gt_pp_set_entry_lane(uint32_t *tabs, const uint8_t *bases, int zlen, size_t u) {
  const size_t per = (size_t) zlen << kPpWin, t = u / per;
  gt_pp_entry_lane<G>(tabs + t * gt_pp_table_words<G>(zlen), bases + t * (size_t) G::bytes(), u % per);
}

// the table of unit u: the t < m with offsets[t] <= u < offsets[t + 1] (offsets[0] = 0 <= u < offsets[m]; a table may
// serve no unit: equal neighbours)
PBC_DEV size_t pp_set_table_of(const uint64_t *__restrict__ offsets, size_t m, uint64_t u) {
  size_t lo = 0, hi = m;               // offsets[lo] <= u < offsets[hi]
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

// the rows of ONE table on the running Jacobian point (ec_pp_pow_lane's loop; `inf`: the point is still O).  An addition
// that meets equal or opposite operands leaves Z = 0, and Z = 0 is absorbing here (H = -X, Z3 = Z H = 0): whatever
// follows, over this table and the next ones, the lane ends with Z = 0 and is reported.
template <class F>
PBC_DEV void ec_pp_rows_acc(typename F::el &X, typename F::el &Y, typename F::el &Z, bool &inf, const uint32_t *__restrict__ tab,
                            const uint8_t *z, int zlen) {
  typedef typename F::el el;
  for (int row = 0; row < zlen; row++) {
    const uint32_t w = z[zlen - 1 - row];
    const size_t u = (size_t) row * kPpRowLen + (w ? w - 1 : 0);
    const el x2 = F::from_words(tab + u * 2 * F::WORDS_EL), y2 = F::from_words(tab + (u * 2 + 1) * F::WORDS_EL);
    el sX = X, sY = Y, sZ = Z;
    ec_madd_inc<F>(sX, sY, sZ, x2, y2);
    const bool take = w != 0, first = take & inf, add = take & !inf;
    F::cmov(X, sX, add);
    F::cmov(Y, sY, add);
    F::cmov(Z, sZ, add);
    F::cmov(X, x2, first);
    F::cmov(Y, y2, first);
    inf &= !take;
  }
}
// out = sum_{j < m} [z_j] B_j from the set's tables, z: the unit's m scalars of zlen bytes; base-major, row-minor, so that
// the loads of a wavefront at one step fall into one 255-entry row.  false (nothing written) when the lane needs the
// complete routine: equal or opposite operands met on the way, or the true sum is O while some scalar byte is not zero.
template <class F>
PBC_DEV bool ec_pp_set_prod_lane(uint8_t *out, const uint32_t *__restrict__ tabs, size_t m, const uint8_t *z, int zlen) {
  typedef typename F::el el;
  const int NB = F::bytes();
  const el one = F::one();
  const size_t tw = ec_pp_table_words<F>(zlen);
  el X = one, Y = one, Z = one;
  bool inf = true;
  for (size_t j = 0; j < m; j++) ec_pp_rows_acc<F>(X, Y, Z, inf, tabs + j * tw, z + j * (size_t) zlen, zlen);
  const bool bad = !inf & F::is0(Z);
  el zinv, zz, ax, ay;
  F::inv(zinv, Z);
  F::sqr(zz, zinv);
  F::mul(ax, X, zz);
  F::mul(zz, zz, zinv);
  F::mul(ay, Y, zz);
  if (inf) { ax = F::zero(); ay = ax; }              // every scalar is 0
  if (!bad) {
    F::store(out, ax);
    F::store(out + NB, ay);
  }
  return !bad;
}
// The COMPLETE lane of the same sum: [z_j] B_j on the complete ladder (ec_mul_lane: any record, any scalar), base after
// base, folded left to right with the complete affine law (group_more.cuh ec_add_affine) on the records the ladder
// writes -- the bytes of m element_mul_zn results folded with element_add.
template <class F>
PBC_DEV void ec_pp_set_prod_complete_lane(uint8_t *out, const uint8_t *bases, size_t m, const uint8_t *z, int zlen) {
  typedef typename F::el el;
  const size_t L = 2 * (size_t) F::bytes();
  el ax = F::zero(), ay = ax;
  bool af = false;
  for (size_t j = 0; j < m; j++) {
    __attribute__((aligned(16))) uint8_t o[8 * F::WORDS_EL];
    ec_mul_lane<F>(o, bases + j * L, z + j * (size_t) zlen, zlen);
    el x, y;
    const bool f = ec_load_affine<F>(x, y, o);
    ec_add_affine<F>(ax, ay, af, ax, ay, af, x, y, f);
  }
  ec_store_affine<F>(out, ax, ay, af);
}
// GT: the plain product of the m * zlen entries (entry w = 0 of a row is the identity): no exceptional case
template <class G>
PBC_DEV void gt_pp_set_prod_lane(uint8_t *out, const uint32_t *__restrict__ tabs, size_t m, const uint8_t *z, int zlen) {
  typedef typename G::el el;
  const size_t tw = gt_pp_table_words<G>(zlen);
  el acc, t;
  G::from_words(acc, tabs + (size_t) z[zlen - 1] * G::WORDS_EL);
  for (size_t j = 0; j < m; j++) {
    const uint32_t *tab = tabs + j * tw;
    const uint8_t *zj = z + j * (size_t) zlen;
    for (int row = j ? 0 : 1; row < zlen; row++) {
      G::from_words(t, tab + ((size_t) row * (1 << kPpWin) + zj[zlen - 1 - row]) * G::WORDS_EL);
      G::mul(acc, acc, t);
    }
  }
  G::store(out, acc);
}

}  // namespace pbc
