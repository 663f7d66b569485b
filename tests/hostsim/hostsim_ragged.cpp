// hostsim_ragged.cpp -- TEST INFRASTRUCTURE: the host mirror (hostsim.cpp: the device headers compiled for the CPU, one
// lane per call) plus the lane bodies of the ragged products (pairing_al.cuh fold_lane / ragged_finish_lane on Miller
// records; group_more.cuh term_flag_lane / gt_fold_lane / gt_fold_finish_lane on GT records), driven as the kernels of
// pbc_hip_a.hip and pbc_hip_ragged.hip drive them: the library's own planner (ragged_plan.h), one lane per output record
// of a level, the lane's (product, block) found by the kernels' binary search.  Built by tests/test_ragged_cpu.py into
// a library of its own.  Not part of the product.
#include "hostsim.cpp"
#include "../../pbc_amd/csrc/ragged_plan.h"

static size_t hs_ragged_find(const uint64_t *o, size_t n, uint64_t j) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (o[mid + 1] > j) hi = mid; else lo = mid + 1;
  }
  return lo;
}
#define HS_RAGGED_DISPATCH(P_, ...)                                                                                   \
  do {                                                                                                                \
    if ((P_)->type == 'a' || (P_)->type == '1') {                                                                     \
      if ((P_)->nlimb == 16) { typedef GtA<16> G; typedef FqOps<16> F1; typedef F1 F2; __VA_ARGS__; }                 \
      else { typedef GtA<33> G; typedef FqOps<33> F1; typedef F1 F2; __VA_ARGS__; }                                   \
    } else if ((P_)->type == 'e') {                                                                                   \
      if ((P_)->nlimb == 16) { typedef GtE<16> G; typedef FqOps<16> F1; typedef F1 F2; __VA_ARGS__; }                 \
      else { typedef GtE<33> G; typedef FqOps<33> F1; typedef F1 F2; __VA_ARGS__; }                                   \
    } else if ((P_)->type == 'f') {                                                                                   \
      HS_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; typedef FqOps<N> F1; typedef Fq2Ops<N> F2; __VA_ARGS__; });      \
    } else {                                                                                                          \
      HS_DISPATCH_D(P_, { typedef GtD<N, DEG> G; typedef FqOps<N> F1; typedef FdOps<N, DEG> F2; __VA_ARGS__; });      \
    }                                                                                                                 \
  } while (0)

extern "C" {

// gt[u] = the product of the pairings of terms offsets[u] .. offsets[u + 1]; fold factor F; *levels_out: fold levels taken
int hostsim_ragged(void *h, uint8_t *gt, const uint8_t *g1, const uint8_t *g2, const uint64_t *offsets, size_t n, int F, int *levels_out) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  std::vector<std::vector<uint64_t>> lv;
  pbc_host::ragged_plan(offsets, n, (unsigned) F, lv);
  const size_t T = (size_t) lv[0][n], lt = (size_t) P->lenT;
  if (levels_out) *levels_out = (int) lv.size() - 1;
  if (P->type == 'a' && !P->a_generic) {                   // the record route
    activate(P, true);
    constexpr int M = AL<16>::MREC;
    std::vector<uint4> cur((T ? T : 1) * M, uint4{0, 0, 0, 0}), nxt;
    for (size_t t = 0; t < T; t++) {
      AL<16>::miller_record_lane(cur.data() + t * M, g1 + t * P->len1, g2 + t * P->len2);
      AL<16>::ragged_mask_lane(cur.data() + t * M, g2 + t * P->len2);
    }
    for (size_t l = 0; l + 1 < lv.size(); l++) {
      const uint64_t *oin = lv[l].data(), *oout = lv[l + 1].data();
      const size_t nout = (size_t) oout[n];
      nxt.assign(nout * M, uint4{0, 0, 0, 0});
      for (size_t j = 0; j < nout; j++) {
        const size_t u = hs_ragged_find(oout, n, j);
        const uint64_t start = oin[u] + (j - oout[u]) * (uint64_t) F, left = oin[u + 1] - start;
        AL<16>::fold_lane(nxt.data() + j * M, cur.data() + start * M, (int) (left < (uint64_t) F ? left : (uint64_t) F));
      }
      cur.swap(nxt);
    }
    const uint64_t *off = lv.back().data();
    const size_t nrec = off[n] ? (size_t) off[n] : 1;
    for (size_t u = 0; u < n; u++) {
      const size_t at = off[u] < nrec ? (size_t) off[u] : nrec - 1;
      AL<16>::ragged_finish_lane(gt + u * lt, cur.data() + at * M, (int) (off[u + 1] - off[u]));
    }
    activate(P);
    return 0;
  }
  // the GT route: single pairings (the lane kernels' bodies), a flag byte per term, folds over GT records
  std::vector<uint8_t> cur((T ? T : 1) * lt), nxt, fcur(T ? T : 1), fnxt;
  if (T && hostsim_prod_pairing(h, cur.data(), g1, g2, T, 1)) return 1;
  activate(P);
  for (size_t t = 0; t < T; t++) HS_RAGGED_DISPATCH(P, (fcur[t] = term_flag_lane<F1, F2>(g1 + t * P->len1, g2 + t * P->len2)));
  for (size_t l = 0; l + 1 < lv.size(); l++) {
    const uint64_t *oin = lv[l].data(), *oout = lv[l + 1].data();
    const size_t nout = (size_t) oout[n];
    nxt.assign(nout * lt, 0);
    fnxt.assign(nout, 0xee);
    for (size_t j = 0; j < nout; j++) {
      const size_t u = hs_ragged_find(oout, n, j);
      const uint64_t start = oin[u] + (j - oout[u]) * (uint64_t) F, left = oin[u + 1] - start;
      const int cnt = (int) (left < (uint64_t) F ? left : (uint64_t) F);
      HS_RAGGED_DISPATCH(P, (fnxt[j] = gt_fold_lane<G>(nxt.data() + j * lt, cur.data() + start * lt, fcur.data() + start, cnt)));
    }
    cur.swap(nxt);
    fcur.swap(fnxt);
  }
  const uint64_t *off = lv.back().data();
  for (size_t u = 0; u < n; u++)
    HS_RAGGED_DISPATCH(P, gt_fold_finish_lane<G>(gt + u * lt, cur.data() + off[u] * lt, fcur.data() + off[u], (int) (off[u + 1] - off[u])));
  return 0;
}

}
