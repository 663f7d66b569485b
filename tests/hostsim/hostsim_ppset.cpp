// hostsim_ppset.cpp -- TEST INFRASTRUCTURE: the host mirror (hostsim.cpp: the device headers compiled for the CPU, one
// lane per call) plus the lane bodies of the table sets (include/pbc_hip.h pbc_hip_pairing_pp_set_*), driven as the
// kernels of pbc_hip_a.hip drive them on the 512-bit type a: the set-init lane (a_pp_init_lane per first argument, table
// after table), then per product one pp_miller_record_lane per term, on the wave slots of the library's own planner
// (pp_set_plan.h, term-major), and prod_finish_lane over the m records.  Built by tests/test_ppset_cpu.py into a library
// of its own.  Not part of the product.
#include "hostsim.cpp"
#include "../../pbc_amd/csrc/pp_set_plan.h"

extern "C" {

// words of one table of a set on this object (0: not the 512-bit type a)
size_t hostsim_ppset_table_words(void *h) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (P->type != 'a' || P->a_generic) return 0;
  return (size_t) (P->a.exp2 + 1) * 3 * 16;
}
// a_pp_set_init_kernel lane by lane: tabs [m][table_words], flags [m]
int hostsim_ppset_init(void *h, uint32_t *tabs, uint32_t *flags, const uint8_t *g1, size_t m) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  const size_t tw = hostsim_ppset_table_words(h);
  if (!tw) return 1;
  activate(P);
  for (size_t idx = 0; idx < m; idx++) flags[idx] = a_pp_init_lane<16>(tabs + idx * tw, g1 + idx * P->len1) ? 1u : 0u;
  return 0;
}
// the single table pbc_hip_pairing_pp_init's kernel derives from one record
int hostsim_ppset_single_table(void *h, uint32_t *tab, uint32_t *flag, const uint8_t *g1) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (!hostsim_ppset_table_words(h)) return 1;
  activate(P);
  *flag = a_pp_init_lane<16>(tab, g1) ? 1u : 0u;
  return 0;
}
// gt[u] = prod_{j<m} e(g1[j], g2[u m + j]) for u < n on the record route: al_pp_set_miller_kernel's lanes over the slots
// of pp_set_prod_plan, then al_prod_finish_kernel's
int hostsim_ppset_prod(void *h, uint8_t *gt, const uint32_t *tabs, const uint32_t *flags, const uint8_t *g2, size_t m, size_t n) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  const size_t tw = hostsim_ppset_table_words(h);
  if (!tw) return 1;
  activate(P);
  constexpr int M = AL<16>::MREC;
  std::vector<uint4> recs(n * m * M, uint4{0, 0, 0, 0});
  std::vector<uint64_t> plan;
  pbc_host::pp_set_prod_plan(m, n, plan);
  for (size_t s = 0; s < plan.size(); s += pbc_host::kPpSetSlotWords) {
    const size_t table = (size_t) plan[s], first = (size_t) plan[s + 1], count = (size_t) plan[s + 2];
    for (size_t lane = 0; lane < count; lane++) {
      const size_t rec = (first + lane) * m + table;
      AL<16>::pp_miller_record_lane(recs.data() + rec * M, tabs + table * tw, flags[table] != 0, g2 + rec * P->len2);
    }
  }
  for (size_t u = 0; u < n; u++) AL<16>::prod_finish_lane(gt + u * P->lenT, recs.data() + u * m * M, (int) m);
  return 0;
}

}
