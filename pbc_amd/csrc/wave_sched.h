// wave_sched.h -- the SCHEDULE ENTRY of the wavefront level machine (wave_vm.cuh), shared by the host, which packs it, and
// the device, which unpacks it; and the host's straight-line builder.  A pairing on the machine is a run of 64-bit entries:
//   row a [0:12) | lanes a [12:17) | row b [17:29) | lanes b [29:34) | terms [34:38) | op [38:42) | table line [42:54) | line flag [55]
//   OP_LEVEL: a level (track a on the first lanes, track b -- type d only -- on the last);  OP_BZERO / OP_INV: lane code of the
//   family (the B = 0 test of cc_tatepower; the one inversion);  OP_END: the end;  OP_LOADLINE: table line -> coefficient slots
//   (pairing_pp_apply, before the first level);  OP_MARK: ends a run that the kernel repeats (type g's product with a term)
//   line flag on a level: that line of the pairing_pp table arrives in its coefficient slots when the level is over
// Which level of which program runs when depends on the curve's constants only, so the host writes the schedules once per
// object ({dw,fw,gw}_sched.h) and the kernel is a plain interpreter.  tools/{dw,fw,gw}_gen.py hold the same sequences on Python
// integers (flat_schedule); tests compare the two entry by entry.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace pbc { namespace wave {

enum { OP_LEVEL = 0, OP_BZERO = 1, OP_INV = 2, OP_END = 3, OP_LOADLINE = 4, OP_MARK = 5 };
// the schedules of an object, one after the other in one buffer (host_params.h WaveSched: off[] -- where each begins): the
// pairing; the Miller value alone (a TERM of a product); the product with a term's value + the final exponentiation;
// pairing_pp_apply (types d and g)
enum { SCHED_PAIRING = 0, SCHED_MILLER = 1, SCHED_FINISH = 2, SCHED_PP = 3 };
struct LevelRef { uint16_t row; uint8_t T, lanes; };              // a level of a family's tables: first row, terms per sum, working lanes
struct ProgRef { const char *name; uint16_t first, count; };      // a program: a run of levels, found by name

constexpr int kRowA = 0, kLanesA = 12, kRowB = 17, kLanesB = 29, kTerms = 34, kOp = 38, kLine = 42, kLineFlag = 55;   // first bits
constexpr unsigned kRowMask = 4095, kLanesMask = 31, kTermsMask = 15, kOpMask = 15, kLineMask = 4095;
constexpr int kMaxLines = (int) kLineMask + 1;

constexpr uint64_t with_line(uint64_t e, int line) { return line >= 0 ? e | (uint64_t) line << kLine | 1ull << kLineFlag : e; }
constexpr uint64_t pack_level(LevelRef a, LevelRef b, unsigned terms, int line = -1) {
  return with_line((uint64_t) a.row << kRowA | (uint64_t) a.lanes << kLanesA | (uint64_t) b.row << kRowB | (uint64_t) b.lanes << kLanesB |
                   (uint64_t) terms << kTerms | (uint64_t) OP_LEVEL << kOp, line);
}
constexpr uint64_t pack_op(int op, int line = -1) { return with_line((uint64_t) op << kOp, line); }
// (constexpr: the device unpacks with the same functions)
constexpr int ent_op(uint64_t e) { return (int) ((e >> kOp) & kOpMask); }
constexpr int ent_terms(uint64_t e) { return (int) ((e >> kTerms) & kTermsMask); }
constexpr bool ent_has_line(uint64_t e) { return ((e >> kLineFlag) & 1u) != 0; }
constexpr int ent_line(uint64_t e) { return (int) ((e >> kLine) & kLineMask); }
constexpr int ent_row_a(uint64_t e) { return (int) ((e >> kRowA) & kRowMask); }
constexpr int ent_lanes_a(uint64_t e) { return (int) ((e >> kLanesA) & kLanesMask); }
constexpr int ent_row_b(uint64_t e) { return (int) ((e >> kRowB) & kRowMask); }
constexpr int ent_lanes_b(uint64_t e) { return (int) ((e >> kLanesB) & kLanesMask); }

// lines of a pairing_pp table: one per doubling, one more per set digit (digit(m): the signed digit of the Miller loop at position m)
template <class Digit>
inline int table_lines(int rbits, const Digit &digit) {
  int n = 0;
  for (int m = rbits - 2; m >= 0; m--) n += 1 + ((m > 0 && digit(m)) ? 1 : 0);
  return n;
}

// One track, programs by name (types f and g): the builder appends every level of a program of the family's tables.
struct Builder {
  std::vector<uint64_t> &out;
  const ProgRef *prog;
  const int progs;
  const LevelRef *level;
  bool ok = true;                                                   // false: a program the generator did not emit
  template <int NP>
  Builder(std::vector<uint64_t> &o, const ProgRef (&p)[NP], const LevelRef *l) : out(o), prog(p), progs(NP), level(l) {}
  void run(const std::string &name) {
    for (int i = 0; i < progs; i++)
      if (name == prog[i].name) {
        for (int l = 0; l < prog[i].count; l++) {
          const LevelRef &A = level[prog[i].first + l];
          out.push_back(pack_level(A, LevelRef{0, 0, 0}, A.T));
        }
        return;
      }
    ok = false;
  }
  void op(int o, int line = -1) { out.push_back(pack_op(o, line)); }
  void run_with_line(const std::string &name, int line) {          // ... whose first level also takes table line `line` (-1: none)
    const size_t at = out.size();
    run(name);
    if (out.size() > at) out[at] = with_line(out[at], line);
  }
};
// the Miller loop of types f and g (cc_miller_no_denom, ecc/f_param.c:216-233; the loop of ecc/d_param.c:321-422 that
// ecc/g_param.c shares).  A square and the doubling of the step after it share nothing: ONE program, "sqrdbl", holds both.
template <class Digit>
inline void build_miller(Builder &B, int rbits, const Digit &digit) {
  for (int m = rbits - 2; m >= 0; m--) {
    if (m == rbits - 2) B.run("pt_dbl");
    B.run("line_mul");
    if (m > 0 && digit(m)) { B.run(digit(m) < 0 ? "pt_addm" : "pt_addp"); B.run("line_mul"); }
    if (m > 0) B.run("sqrdbl");
  }
}

} }  // namespace pbc::wave
