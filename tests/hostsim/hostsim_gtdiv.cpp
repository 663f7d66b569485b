// hostsim_gtdiv.cpp -- TEST INFRASTRUCTURE: the host mirror (hostsim.cpp: the device headers compiled for the CPU, one lane
// per call) plus the lane bodies of element_invert / element_div on GT and of element_cmp (group_gtdiv.cuh) and the host
// derivation of the compared integer (cmp_plan.h), with the dispatch of pbc_hip_gtdiv.hip.  Built by
// tests/test_gtdiv_cpu.py / tests/test_cmp_cpu.py into a library of its own.  Not part of the product.
#include "hostsim.cpp"
#include "../../pbc_amd/csrc/group_gtdiv.cuh"
#include "../../pbc_amd/csrc/mpz_plan.h"
#include "../../pbc_amd/csrc/cmp_plan.h"

#include <vector>

#define HS_DISPATCH_GTDIV(P_, ...)                                                                                \
  do {                                                                                                            \
    const int t_ = (P_)->type;                                                                                    \
    if (t_ == 'a' || t_ == '1') { if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if (t_ == 'e') { if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if (t_ == 'f') { HS_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); }                        \
    else { HS_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                                          \
  } while (0)

extern "C" {

// b == null: out[i] = a[i]^-1, else a[i] / b[i].  generic: "hip_group_slow 1".  lanes[i]: 1 where the lane ran the
// inversion in the subfield, 0 where it stored the conjugate (the product with it)
int hostsim_gtdiv(void *h, int generic, uint8_t *out, uint8_t *lanes, const uint8_t *a, const uint8_t *b, size_t n) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  activate(P);
  const size_t L = (size_t) P->lenT;
  for (size_t i = 0; i < n; i++) {
    bool slow = false;
    if (b) HS_DISPATCH_GTDIV(P, (slow = gt_div_lane<G>(out + i * L, a + i * L, b + i * L, generic != 0)));
    else HS_DISPATCH_GTDIV(P, (slow = gt_invert_lane<G>(out + i * L, a + i * L, generic != 0)));
    lanes[i] = slow ? 1 : 0;
  }
  return 0;
}
// element_cmp.  mode 0: as the library -- on a twist the fast lane, and the complete lane where it raised its flag; 1: the
// complete lane alone ("hip_group_slow 1"); 2: the fast lane alone.  flags[i]: the fast lane's flag (0 off the twists and
// in mode 1).  text: the parameter text the integer is derived from (the twists)
int hostsim_cmp(void *h, int group, int mode, uint8_t *res, uint8_t *flags, const uint8_t *a, const uint8_t *b, size_t n, const char *text, size_t tlen) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (group < 0 || group > 3) return 1;
  const bool sym = P->type == 'a' || P->type == '1' || P->type == 'e';
  for (size_t i = 0; i < n; i++) flags[i] = 0;
  if (group == 0) {
    if (!P->zr_nlimb) return 1;
    int rc = 0;
    HS_DISPATCH(P->zr_nlimb, {
      KArgs<N> K;
      rc = zr_kargs<N>(P, K);
      memcpy(hostsim_kargs + sizeof hostsim_kargs - sizeof K, &K, sizeof K);
      const size_t L = (size_t) P->len_zr;
      for (size_t i = 0; i < n && !rc; i++) res[i] = zr_cmp_lane<N>(a + i * L, b + i * L);
    });
    activate(P);
    return rc;
  }
  activate(P);
  if (group == 3) {
    const size_t L = (size_t) P->lenT;
    for (size_t i = 0; i < n; i++) HS_DISPATCH_GTDIV(P, (res[i] = gt_cmp_lane<G>(a + i * L, b + i * L)));
    return 0;
  }
  if (group == 1 || sym) {
    const size_t L = (size_t) P->len1;
    for (size_t i = 0; i < n; i++) HS_DISPATCH(P->nlimb, (res[i] = ec_cmp_plain_lane<FqOps<N>>(a + i * L, b + i * L)));
    return 0;
  }
  std::vector<uint8_t> c;
  if (!pbc_host::cmp_quotient(text, tlen, 1, c) || c.empty()) return 2;
  for (size_t i = c.size(); i-- > 0;) if (c[i]--) break;         // c - 1
  std::vector<int8_t> d;
  const int w = pbc_host::mpz_recode(false, c.data(), c.size(), d);
  const int nd = (int) d.size();
  std::vector<uint32_t> words(d.size() / 4 + 1, 0);
  if (!d.empty()) memcpy(words.data(), d.data(), d.size());
  const uint32_t *dig = words.data();
  const size_t L = (size_t) P->len2;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *ra = a + i * L, *rb = b + i * L;
    bool flag = false;
    uint8_t v = 0xff;
    if (mode != 1) HS_DISPATCH_TWIST(P, (v = w == 2 ? ec_cmp_fast_lane<F, 2>(ra, rb, dig, nd, flag) : ec_cmp_fast_lane<F, 4>(ra, rb, dig, nd, flag)));
    if (mode == 1 || (mode == 0 && flag)) HS_DISPATCH_TWIST(P, (v = ec_cmp_complete_lane<F>(ra, rb, dig, nd, w)));
    flags[i] = flag ? 1 : 0;
    res[i] = v;
  }
  return 0;
}

}
