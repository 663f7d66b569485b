// hostsim_eppset.cpp -- TEST INFRASTRUCTURE: the host mirror (hostsim.cpp: the device headers compiled for the CPU, one lane
// per call) plus the lane bodies of the fixed-base table sets (group_ppset.cuh) with the routing of pbc_hip_eppset.hip.
// Built by tests/test_eppset_cpu.py into a library of its own.  Not part of the product.
#include "hostsim.cpp"
#include "../../pbc_amd/csrc/group_ppset.cuh"

#include <vector>

#define HS_DISPATCH_EPP_GT(P_, ...)                                                                               \
  do {                                                                                                            \
    const int t_ = (P_)->type;                                                                                    \
    if (t_ == 'a' || t_ == '1') { if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if (t_ == 'e') { if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if (t_ == 'f') { HS_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); }                        \
    else { HS_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                                          \
  } while (0)

static size_t epp_len(const pbc_hip_pairing_s *P, int group) { return (size_t) (group == 3 ? P->lenT : group == 2 ? P->len2 : P->len1); }

extern "C" {

// entries of one table / 32-bit words of one table
size_t hostsim_eppset_entries(void *h, int group) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  return group == 3 ? (size_t) P->len_zr << kPpWin : (size_t) P->len_zr * kPpRowLen;
}
size_t hostsim_eppset_table_words(void *h, int group) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  size_t w = 0;
  if (group == 3) HS_DISPATCH_EPP_GT(P, w = gt_pp_table_words<G>(P->len_zr));
  else HS_DISPATCH_G(P, group, w = ec_pp_table_words<F>(P->len_zr));
  return w;
}
// the set's tables, one entry per call of the set's entry lane: every unit (units == null) or the listed ones; eflags
// (groups 1, 2): one byte per entry, written for the units built
int hostsim_eppset_tables(void *h, int group, uint32_t *tabs, uint8_t *eflags, const uint8_t *bases, size_t m, const uint64_t *units, size_t nunits) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (group < 1 || group > 3) return 1;
  activate(P);
  const size_t all = m * hostsim_eppset_entries(h, group);
  const size_t cnt = units ? nunits : all;
  for (size_t i = 0; i < cnt; i++) {
    const size_t u = units ? (size_t) units[i] : i;
    if (u >= all) return 2;
    if (group == 3) HS_DISPATCH_EPP_GT(P, gt_pp_set_entry_lane<G>(tabs, bases, P->len_zr, u));
    else HS_DISPATCH_G(P, group, ec_pp_set_entry_lane<F>(tabs, eflags, bases, P->len_zr, u));
  }
  return 0;
}
// the table of a single-base object (pbc_hip_element_pp_init: ec_pp_entry_lane / gt_pp_entry_lane on the base itself):
// every entry (units == null) or the listed ones
int hostsim_eppset_single_table(void *h, int group, uint32_t *tab, uint8_t *eflags, const uint8_t *base, const uint64_t *units, size_t nunits) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (group < 1 || group > 3) return 1;
  activate(P);
  const size_t per = hostsim_eppset_entries(h, group);
  for (size_t i = 0; i < (units ? nunits : per); i++) {
    const size_t u = units ? (size_t) units[i] : i;
    if (u >= per) return 2;
    if (group == 3) HS_DISPATCH_EPP_GT(P, gt_pp_entry_lane<G>(tab, base, u));
    else HS_DISPATCH_G(P, group, ec_pp_entry_lane<F>(tab, eflags, base, P->len_zr, u));
  }
  return 0;
}
// multi-base powers of n units (m scalars each).  mode 0: as the library -- complete_only (some table of the set is
// "complete only") sends every unit to the complete lane, otherwise the fast lane and the complete lane where it raised
// its flag; 1: the complete lane alone ("hip_group_slow 1"); 2: the fast lane alone (a flagged unit's record is left as
// it was).  flags[i]: the fast lane's flag (0 where it did not run).  GT has one lane and no flags.
int hostsim_eppset_prod(void *h, int group, int mode, int complete_only, uint8_t *out, uint8_t *flags, const uint32_t *tabs, const uint8_t *bases, size_t m,
                        const uint8_t *zr, size_t n) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (group < 1 || group > 3) return 1;
  activate(P);
  const size_t L = epp_len(P, group), zl = (size_t) P->len_zr;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *z = zr + i * m * zl;
    uint8_t *o = out + i * L;
    flags[i] = 0;
    if (group == 3) { HS_DISPATCH_EPP_GT(P, gt_pp_set_prod_lane<G>(o, tabs, m, z, P->len_zr)); continue; }
    bool ok = false;
    const bool fast = mode == 2 || (mode == 0 && !complete_only);
    if (fast) {
      HS_DISPATCH_G(P, group, ok = ec_pp_set_prod_lane<F>(o, tabs, m, z, P->len_zr));
      flags[i] = ok ? 0 : 1;
    }
    if (mode == 1 || (mode == 0 && !ok)) HS_DISPATCH_G(P, group, ec_pp_set_prod_complete_lane<F>(o, bases, m, z, P->len_zr));
  }
  return 0;
}
// segmented powers: unit u takes the table pp_set_table_of finds in offsets (m + 1 values); tflags: one "complete only"
// byte per table.  mode as above (the complete lane: ec_mul_lane on the unit's own base)
int hostsim_eppset_pow(void *h, int group, int mode, uint8_t *out, uint8_t *flags, const uint32_t *tabs, const uint8_t *tflags, const uint8_t *bases, size_t m,
                       const uint8_t *zr, const uint64_t *offsets) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (group < 1 || group > 3) return 1;
  activate(P);
  const size_t L = epp_len(P, group), zl = (size_t) P->len_zr, n = (size_t) offsets[m];
  for (size_t i = 0; i < n; i++) {
    const size_t t = pp_set_table_of(offsets, m, i);
    if (t >= m || offsets[t] > i || i >= offsets[t + 1]) return 2;
    const uint8_t *z = zr + i * zl;
    uint8_t *o = out + i * L;
    flags[i] = 0;
    if (group == 3) { HS_DISPATCH_EPP_GT(P, gt_pp_pow_lane<G>(o, tabs + t * gt_pp_table_words<G>(P->len_zr), z, P->len_zr)); continue; }
    bool ok = false;
    if (mode != 1) {
      if (!tflags[t]) HS_DISPATCH_G(P, group, ok = ec_pp_pow_lane<F>(o, tabs + t * ec_pp_table_words<F>(P->len_zr), z, P->len_zr));
      flags[i] = ok ? 0 : 1;
    }
    if (mode == 1 || (mode == 0 && !ok)) HS_DISPATCH_G(P, group, ec_mul_lane<F>(o, bases + t * L, z, P->len_zr));
  }
  return 0;
}

}
