// ragged_plan.h -- the host-side plan of a ragged product of pairings (include/pbc_hip.h
// pbc_hip_element_prod_pairing_ragged_batch): pure host code, shared by the library (pbc_hip_ragged.hip), its planner
// diagnostic (pbc_hip_diag_ragged_plan) and the host mirror of the tests.
// A product of c records is folded level by level: at every level a lane multiplies up to F consecutive records of ONE
// product into one, so a product of c records has ceil(c / F) at the next level; this repeats until no product holds
// more than F records, which a finish lane multiplies.  Level 0 is the caller's offsets array; level i + 1 is the prefix
// sum of ceil(c_i(u) / F).  An empty product stays empty at every level.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pbc_host {

constexpr uint64_t kRaggedMaxTerms = (uint64_t) 1 << 22;   // terms of one product, and of one launch group (the workspace bound of include/pbc_hip.h)
constexpr int kRaggedFoldDefault = 16;                     // "hip_ragged_fold N", 2 <= N <= 64 (profiles/ragged_notes.md)

// 0: fine; 1: offsets[0] != 0; 2: a decreasing pair (*at = its first index); 3: a product above kRaggedMaxTerms (*at = the product)
static inline int ragged_check(const uint64_t *offsets, size_t n, size_t *at) {
  if (offsets[0] != 0) return 1;
  for (size_t u = 0; u < n; u++) {
    if (offsets[u + 1] < offsets[u]) { *at = u; return 2; }
    if (offsets[u + 1] - offsets[u] > kRaggedMaxTerms) { *at = u; return 3; }
  }
  return 0;
}

// levels[0] = offsets rebased to offsets[0] (n + 1 values), then one array per fold level; the last one has every count <= F
static inline void ragged_plan(const uint64_t *offsets, size_t n, unsigned F, std::vector<std::vector<uint64_t>> &levels) {
  levels.clear();
  levels.emplace_back(n + 1);
  uint64_t longest = 0;
  for (size_t u = 0; u <= n; u++) levels[0][u] = offsets[u] - offsets[0];
  for (size_t u = 0; u < n; u++) if (levels[0][u + 1] - levels[0][u] > longest) longest = levels[0][u + 1] - levels[0][u];
  while (longest > F) {
    const std::vector<uint64_t> &in = levels.back();
    std::vector<uint64_t> out(n + 1);
    out[0] = 0;
    for (size_t u = 0; u < n; u++) out[u + 1] = out[u] + (in[u + 1] - in[u] + F - 1) / F;
    longest = (longest + F - 1) / F;
    levels.push_back(std::move(out));
  }
}

}  // namespace pbc_host
