// hostsim_mpz.cpp -- TEST INFRASTRUCTURE: the host mirror (hostsim.cpp: the device headers compiled for the CPU, one lane
// per call) plus the lane bodies of element_mul_mpz / element_pow_mpz (group_mpz.cuh) and the host recoding
// (mpz_plan.h), with the dispatch of pbc_hip_mpz.hip.  Built by tests/test_mpz_cpu.py into a library of its own.  Not
// part of the product.
#include "hostsim.cpp"
#include "../../pbc_amd/csrc/group_mpz.cuh"
#include "../../pbc_amd/csrc/mpz_plan.h"

#include <vector>

// the digits as the device buffer holds them: int8, padded to whole words.  w = 0: the library's choice for points
// (mpz_plan.h mpz_recode), else the width asked for; `w` returns the width taken
static std::vector<uint32_t> mpz_words(const uint8_t *k, size_t klen, int &w, int &nd) {
  std::vector<int8_t> d;
  if (w) pbc_host::mpz_digits(k, klen, w, d);
  else w = pbc_host::mpz_recode(false, k, klen, d);
  nd = (int) d.size();
  std::vector<uint32_t> words(d.size() / 4 + 1, 0);
  if (!d.empty()) memcpy(words.data(), d.data(), d.size());
  return words;
}

extern "C" {

// G1 / G2 (group 1 / 2).  mode 0: as the library -- the fast lane, and the complete lane where it raised its flag; 1: the
// complete lane alone ("hip_group_slow 1"); 2: the fast lane alone (a flagged unit's record is left as it was).
// flags[i]: the fast lane's flag (0 in mode 1).  The 512-bit type a field and G1 of the five-word fields take their
// limb-form fast lanes, bound trackers armed.  w: 0 = the width the library takes for this k, or 2 / 4 to force one.
// Returns the width taken, negative on an error.
int hostsim_mpz_points(void *h, int group, int mode, int w, uint8_t *out, uint8_t *flags, const uint8_t *in, size_t n, const uint8_t *k, size_t klen) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if ((group != 1 && group != 2) || (w != 0 && w != 2 && w != 4)) return -1;
  activate(P);
  const size_t L = (size_t) (group == 2 ? P->len2 : P->len1);
  const bool fast_a = P->type == 'a' && !P->a_generic;
  const bool fast_l5 = group == 1 && P->nlimb == 5 && ((P->type == 'd' && P->deg == 3 && P->dconst.limb_ok) || (P->type == 'f' && P->fconst.pl_ok));
  int nd;
  const std::vector<uint32_t> words = mpz_words(k, klen, w, nd);
  const uint32_t *dig = words.data();
  for (size_t i = 0; i < n; i++) {
    const uint8_t *rec = in + i * L;
    uint8_t *o = out + i * L;
    bool ok = false;
    if (mode != 1) {
      if (fast_a) ok = w == 2 ? MpzAL<16>::fast_lane<2>(o, rec, dig, nd) : MpzAL<16>::fast_lane<4>(o, rec, dig, nd);
      else if (fast_l5 && P->type == 'd') ok = w == 2 ? MpzL5<KPd>::fast_lane<2>(o, rec, dig, nd) : MpzL5<KPd>::fast_lane<4>(o, rec, dig, nd);
      else if (fast_l5) ok = w == 2 ? MpzL5<KPf>::fast_lane<2>(o, rec, dig, nd) : MpzL5<KPf>::fast_lane<4>(o, rec, dig, nd);
      else HS_DISPATCH_G(P, group, (ok = w == 2 ? ec_mpz_fast_lane<F, 2>(o, rec, dig, nd) : ec_mpz_fast_lane<F, 4>(o, rec, dig, nd)));
    }
    if (mode == 1 || (mode == 0 && !ok)) HS_DISPATCH_G(P, group, (ec_mpz_complete_lane<F>(o, rec, dig, nd, w)));
    flags[i] = (mode != 1 && !ok) ? 1 : 0;
  }
  return w;
}
// GT.  mode 0: as the library (the 512-bit type a field: the Lucas lane, the generic lane where it raised its flag; type f
// on the five-word field: the cyclotomic lane of element_pow_zn on k as a Z_r record where mpz_gt_wants_record says so,
// the generic lane where it raised its flag; otherwise the generic lane); 1: the generic lane alone; 2: the Lucas lane
// alone (type a fast path only)
#define HS_DISPATCH_MPZ_GT(P_, ...)                                                                               \
  do {                                                                                                            \
    const int t_ = (P_)->type;                                                                                    \
    if (t_ == 'a' || t_ == '1') { if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if (t_ == 'e') { if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if (t_ == 'f') { HS_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); }                        \
    else { HS_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                                          \
  } while (0)
int hostsim_mpz_gt(void *h, int mode, uint8_t *out, uint8_t *flags, const uint8_t *in, size_t n, const uint8_t *k, size_t klen) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  activate(P);
  const size_t L = (size_t) P->lenT;
  const bool fast_a = P->type == 'a' && !P->a_generic;
  if (mode == 2 && !fast_a) return 1;
  int nd, w = 1;
  const std::vector<uint32_t> words = mpz_words(k, klen, w, nd);
  const uint32_t *dig = words.data();
  std::vector<int8_t> bits;
  pbc_host::mpz_digits(k, klen, 1, bits);
  const bool cyc_f = mode == 0 && P->type == 'f' && P->nlimb == 5 && pbc_host::mpz_gt_wants_record(bits, (size_t) P->len_zr);
  std::vector<uint8_t> zr((size_t) P->len_zr, 0);
  if (cyc_f)
    for (size_t b = 0; b < bits.size(); b++) if (bits[b]) zr[zr.size() - 1 - (b >> 3)] |= (uint8_t) (1u << (b & 7));
  for (size_t i = 0; i < n; i++) {
    const uint8_t *rec = in + i * L;
    uint8_t *o = out + i * L;
    bool ok = false;
    if (mode != 1 && fast_a) ok = MpzAL<16>::gt_fast_lane(o, rec, dig, nd);
    if (cyc_f) {
      activate(P, true);               // the pairing kernels' constant block, as the library passes it to this lane
      if (P->f_bm1 && P->fconst_i.xs_ok) ok = f_gt_pow_cyc_lane<TypeF<5, true, true>>(o, rec, zr.data(), P->len_zr);
      else if (P->f_bm1) ok = f_gt_pow_cyc_lane<TypeF<5, true, false>>(o, rec, zr.data(), P->len_zr);
      else ok = f_gt_pow_cyc_lane<TypeF<5, false, false>>(o, rec, zr.data(), P->len_zr);
      activate(P);
    }
    if (mode == 1 || (mode == 0 && !ok)) HS_DISPATCH_MPZ_GT(P, (gt_mpz_lane<G>(o, rec, dig, nd)));
    flags[i] = (mode != 1 && (fast_a || cyc_f) && !ok) ? 1 : 0;
  }
  return 0;
}
// the recoding itself (what pbc_hip_diag_mpz_digits returns, without the library)
size_t hostsim_mpz_digits(const uint8_t *k, size_t klen, int w, int8_t *out, size_t cap) {
  std::vector<int8_t> d;
  if (w) pbc_host::mpz_digits(k, klen, w, d);
  else (void) pbc_host::mpz_recode(false, k, klen, d);
  for (size_t i = 0; i < d.size() && i < cap; i++) out[i] = d[i];
  return d.size();
}

}
