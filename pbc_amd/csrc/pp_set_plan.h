// pp_set_plan.h -- the host-side wave plan of a call on a set of preprocessed first arguments (include/pbc_hip.h
// pbc_hip_pairing_pp_set_apply_batch / pbc_hip_pairing_pp_set_prod_batch): pure host code, shared by the library
// (pbc_hip_ppset.hip), its planner diagnostic (pbc_hip_diag_pp_set_plan) and the host mirror of the tests.
// The apply lanes read their table as wave-uniform data (AL::to_el_uniform keeps the word-to-limb conversion on the
// scalar unit), so a wavefront must never hold units of two tables.  The plan deals the units out to WAVE SLOTS: one
// descriptor (table, first unit, count) per slot, 1 <= count <= 64, ceil(c / 64) slots for a table of c units, none for
// a table without units.  Slot s is run by the s-th wavefront of the launch (the resident kernels: by whichever
// wavefront reaches block s of their unit range 64 x slots).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pbc_host {

constexpr uint64_t kPpSetWave = 64;        // units of one slot: the lanes of a wavefront
constexpr int kPpSetSlotWords = 3;         // uint64_t per descriptor: table, first unit, count

// offsets: m + 1 values.  0: fine; 1: offsets[0] != 0; 2: a decreasing pair (*at = its first index)
static inline int pp_set_check(const uint64_t *offsets, size_t m, size_t *at) {
  if (offsets[0] != 0) return 1;
  for (size_t t = 0; t < m; t++)
    if (offsets[t + 1] < offsets[t]) { *at = t; return 2; }
  return 0;
}

// Segmented apply: table t serves the units offsets[t] <= i < offsets[t + 1].  The slots of the units c0 <= i < c1 (a
// chunk of the host-buffer form; the whole call: 0, offsets[m]) are appended to `slots`, `first` relative to c0.
static inline void pp_set_plan_range(const uint64_t *offsets, size_t m, uint64_t c0, uint64_t c1, std::vector<uint64_t> &slots) {
  for (size_t t = 0; t < m; t++) {
    const uint64_t a = offsets[t] > c0 ? offsets[t] : c0, b = offsets[t + 1] < c1 ? offsets[t + 1] : c1;
    for (uint64_t i = a; i < b; i += kPpSetWave) {
      slots.push_back(t);
      slots.push_back(i - c0);
      slots.push_back(b - i < kPpSetWave ? b - i : kPpSetWave);
    }
  }
}
static inline void pp_set_plan(const uint64_t *offsets, size_t m, std::vector<uint64_t> &slots) {
  pp_set_plan_range(offsets, m, 0, offsets[m], slots);
}

// Products over the set, term-major: the slots of table j cover the products u = 0 .. n - 1; the lane of unit u works
// on term record u m + j (the kernels' index stride), so the m terms of a product lie next to each other for the
// kernel that multiplies them.
static inline void pp_set_prod_plan(size_t m, size_t n, std::vector<uint64_t> &slots) {
  for (size_t j = 0; j < m; j++)
    for (uint64_t u = 0; u < n; u += kPpSetWave) {
      slots.push_back(j);
      slots.push_back(u);
      slots.push_back(n - u < kPpSetWave ? n - u : kPpSetWave);
    }
}

}  // namespace pbc_host
