// wave_vm.cuh -- the WAVEFRONT LEVEL MACHINE: one pairing per wavefront, and nothing of any one pairing (round 6; small batches).
//
// A throughput kernel runs a pairing as one lane's serial instruction stream, milliseconds whatever the batch size.  Every
// tower operation, though, is a set of INDEPENDENT lazily reduced sums of F_q products.  Here a wavefront owns one pairing:
//   * every F_q element is a slot of L 29-bit limbs in an LDS slot file (TB::kSlots slots per wavefront);
//   * a LEVEL is "lane l computes out[l] = sum_t x[l][t] y[l][t] / R" -- the library's sop_limbs on operands gathered from
//     the slot file by the lane's ROW of the family's table (TB::rows_src(): {dw,fw,gw}_tables.h, generated and checked against
//     the reference's vectors on Python integers by tools/{dw,fw,gw}_gen.py) -- "and writes its slot"; a level's lanes read
//     before any lane writes;
//   * sums, differences and small multiples are products with the constant slots 1, -1, 2, ...: nothing but sums of
//     products exists, so ONE routine (2 / 4 terms per lane; eight-term sums on four lanes each) is the whole arithmetic;
//   * a level has two TRACKS, a on lanes 0-31 and b on lanes 32-63 (type d runs the accumulator beside the point; types f and g
//     use one).
// Which level runs when depends on the curve's constants only: the HOST flattens a pairing into a schedule of 64-bit entries
// (wave_sched.h) and interpret() runs it.  What is not a level -- the set-up from the wire bytes, the B = 0 test, the one
// inversion -- is ordinary lane code of a FAMILY (pairing_dw.cuh, pairing_fw.cuh, pairing_gw.cuh), a struct with
//   VM                          this machine on its tables (TB: kSlots, kRows, rows_src(); kLines -- whether pairing_pp tables exist --
//                               and, where they do, line_slot(line): where a line's three coefficients go)
//   kCoef, kF                   coefficients of a GT element; the first slot of the accumulator f (kCoef consecutive slots, wire order)
//   kG1, kG2, kGT               F_q elements of a G1, G2, GT record on the wire
//   setup_consts()              lane 0: the constant slots
//   setup_inputs(g1, g2)        lane 0: bytes -> slots, curve checks; false: an argument not on its curve.  g1 == nullptr:
//                               pairing_pp_apply, the table stands for the first argument
//   lane_op(op)                 an entry that is no level: the family's lane code for op; false: not an op of the family's (the
//                               machine then takes it for OP_LOADLINE)
//   kHasMark                    whether the family's schedules hold OP_MARK (it then ends a run of interpret() as OP_END does)
//   kOperand, kProdEntries, kFinishPrefetch     the finish step of a product, see finish()
// The drivers -- pairing, miller_term, finish, pp_apply -- are at the end.
#pragma once
#include "fp.cuh"
#include "wave_sched.h"

#ifndef PBC_DW_WHATIF
#define PBC_DW_WHATIF 0               // timing what-ifs (wrong results): bit 1 no Miller loop, bit 2 no final exponentiation
#endif
#ifndef PBC_DW_SPLIT
#define PBC_DW_SPLIT 1                // eight-term levels on four lanes per sum (exec_split8)
#endif
namespace pbc {

template <int ND, class TB> __shared__ __attribute__((aligned(16))) uint32_t g_lds_wv[TB::kSlots * Limbs29<ND>::L + TB::kRows * 5];

// the slots of the constants 0, 1, -1, 2, -2, 3, 4, -8 (16 and 1/2: where the family has them) and of the point track's state
// (V = (X, Y, Z) in Jacobian coordinates with Z^2, Z^3 and -Z; P and -Py), as a family's tables number them
struct WaveSmallSlots { int zero, one, m1, two, m2, three, four, m8, sixteen = -1, half = -1; };
struct WavePointSlots { int X, Y, Z, nZ, ZZ, ZZZ, Px, Py, nPy; };

template <int ND, class TB>
struct WaveVM {
  typedef fp<ND> fq;
  static constexpr int L = Limbs29<ND>::L;
  // (the row tables hold sums of up to eight terms.  Six and seven limbs: eight products of every limb pair and the reduction's
  // fit a 64-bit column, fp.cuh sop_limbs.  Eight limbs: the eight terms alone do -- 64 products below 2^58 --, and the four
  // lanes' joined columns are relieved exactly, wide_squeeze, before the reduction adds its own: exec_split8.)
  static constexpr bool kSqueeze = 8 * L + L > 63;
  static_assert(4 * L + L <= 63 && 8 * L <= 64, "sums of four terms on a lane, of eight on four lanes");

  static PBC_DEV uint32_t *slot(int s) { return g_lds_wv<ND, TB> + s * L; }
  static PBC_DEV const uint32_t *rows() { return g_lds_wv<ND, TB> + TB::kSlots * L; }
  static PBC_DEV void put(int s, const fl<ND> &a) {
#pragma unroll
    for (int i = 0; i < L; i++) slot(s)[i] = a.l[i];
  }
  static PBC_DEV fl<ND> get(int s) {
    fl<ND> r;
#pragma unroll
    for (int i = 0; i < L; i++) r.l[i] = slot(s)[i];
    return r;
  }
  static PBC_DEV void put_fq(int s, const fq &a) { fl<ND> t; to_limbs<ND>(t, a); put(s, t); }
  static PBC_DEV fq get_fq(int s) { fq r; from_limbs<ND>(r, get(s)); return r; }     // the canonical residue (Montgomery form)

  struct Lev { int row, T, lanes; };
  static PBC_DEV Lev ent_a(uint64_t e) { return Lev{wave::ent_row_a(e), wave::ent_terms(e), wave::ent_lanes_a(e)}; }
  static PBC_DEV Lev ent_b(uint64_t e) { return Lev{wave::ent_row_b(e), wave::ent_terms(e), wave::ent_lanes_b(e)}; }

  // One level of the machine: track a on lanes 0-31, track b on lanes 32-63 (lanes = 0: the track idles).  A lane's ROW
  // (the slot it writes, eight x and eight y operand slots) does not depend on data: the rows of level k + 1 are read while
  // level k multiplies (one LDS round trip less on every level's critical path).
  struct Rows { uint32_t w[5]; bool active; };
  static PBC_DEV Rows load_rows(const Lev a, const Lev b) {
    const int lane = (int) threadIdx.x, r = lane & 31;
    const bool second = lane >= 32;
    const int first = second ? b.row : a.row, lanes = second ? b.lanes : a.lanes;
    Rows R;
    R.active = r < lanes;
    const uint32_t *p = rows() + (first + (R.active ? r : 0)) * 5;
#pragma unroll
    for (int i = 0; i < 5; i++) R.w[i] = R.active ? p[i] : 0u;           // (slot 0 is ZERO: an idle lane multiplies zeros)
    return R;
  }
  template <int T>
  static PBC_DEV void exec_T(const Rows &R) {
    fl<ND> x[T], y[T], res;
#pragma unroll
    for (int t = 0; t < T; t++) {
      const int kx = 1 + t, ky = 9 + t;
      const uint32_t *px = slot((int) ((R.w[kx >> 2] >> (8 * (kx & 3))) & 255u));
      const uint32_t *py = slot((int) ((R.w[ky >> 2] >> (8 * (ky & 3))) & 255u));
#pragma unroll
      for (int i = 0; i < L; i++) { x[t].l[i] = px[i]; y[t].l[i] = py[i]; }
    }
    sop_limbs<ND, T>(res, x, y);
    __builtin_amdgcn_wave_barrier();                                      // every lane has read: now the writes
    if (R.active) put((int) (R.w[0] & 255u), res);
    __builtin_amdgcn_wave_barrier();
  }
  // Eight-term levels, FOUR lanes per sum (PBC_DW_SPLIT): a lone wavefront gets one v_mad_u64_u32 through every ~9 cycles, so
  // a level's time is its multiply-adds per LANE.  Lane s of a group of four accumulates terms s and s + 4 unreduced (wide
  // columns), two DPP exchanges (quad_perm 1032 / 2301) add the four partial columns, every lane reduces, lane 0 of the
  // group writes: 72 + 36 multiply-adds per lane instead of 288 + 36.
  static PBC_DEV Rows load_rows4(const Lev a, const Lev b) {
    const int g = (int) threadIdx.x >> 2;
    const bool second = g >= a.lanes;               // track a's sums take the first groups, track b's the next (at most 16 in all: dw_gen.py)
    const int r = second ? g - a.lanes : g, first = second ? b.row : a.row, lanes = second ? b.lanes : a.lanes;
    Rows R;
    R.active = r < lanes;
    const uint32_t *p = rows() + (first + (R.active ? r : 0)) * 5;
#pragma unroll
    for (int i = 0; i < 5; i++) R.w[i] = R.active ? p[i] : 0u;
    return R;
  }
  static PBC_DEV uint32_t row_byte(const Rows &R, int k) {                // k wave-uniform or per lane
    uint32_t w = R.w[0];
#pragma unroll
    for (int i = 1; i < 5; i++) w = (k >> 2) == i ? R.w[i] : w;
    return (w >> (8 * (k & 3))) & 255u;
  }
  static PBC_DEV void exec_split8(const Rows &R) {
    const int s = (int) threadIdx.x & 3;
    wide<ND> W;
    wide_zero<ND>(W);
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int t = s + 4 * j;
      const uint32_t *px = slot((int) row_byte(R, 1 + t)), *py = slot((int) row_byte(R, 9 + t));
      fl<ND> x, y;
#pragma unroll
      for (int i = 0; i < L; i++) { x.l[i] = px[i]; y.l[i] = py[i]; }
      wide_mac<ND>(W, x, y);
    }
#pragma unroll
    for (int k = 0; k < 2 * L - 1; k++) {
      uint32_t lo = (uint32_t) W.c[k], hi = (uint32_t) (W.c[k] >> 32);
      uint32_t plo = (uint32_t) __builtin_amdgcn_mov_dpp((int) lo, 0xB1, 0xF, 0xF, false), phi = (uint32_t) __builtin_amdgcn_mov_dpp((int) hi, 0xB1, 0xF, 0xF, false);
      W.c[k] += ((uint64_t) phi << 32) | plo;                             // + the neighbour's (lanes 0<->1, 2<->3)
      lo = (uint32_t) W.c[k]; hi = (uint32_t) (W.c[k] >> 32);
      plo = (uint32_t) __builtin_amdgcn_mov_dpp((int) lo, 0x4E, 0xF, 0xF, false); phi = (uint32_t) __builtin_amdgcn_mov_dpp((int) hi, 0x4E, 0xF, 0xF, false);
      W.c[k] += ((uint64_t) phi << 32) | plo;                             // + the other pair's (0<->2, 1<->3)
    }
    fl<ND> res;
    if constexpr (kSqueeze) wide_squeeze<ND>(W);
    wide_reduce<ND>(res, W);
    __builtin_amdgcn_wave_barrier();
    if (R.active && s == 0) put((int) (R.w[0] & 255u), res);
    __builtin_amdgcn_wave_barrier();
  }
  static PBC_DEV void exec(const Rows &R, const Rows &R4, int T) {
    if (T <= 2) exec_T<2>(R);
    else if (T <= 4) exec_T<4>(R);
    else if constexpr (PBC_DW_SPLIT || kSqueeze) exec_split8(R4);
    else exec_T<8>(R);
  }

  // ---- lane 0: the constants and the point state that every family has ----
  static PBC_DEV void put_small_consts(const WaveSmallSlots &S) {
    fq zero, one, t, u;
    fp_set<ND>(one, fpk<ND>().one);
#pragma unroll
    for (int k = 0; k < ND; k++) zero.v[k] = 0;
    put_fq(S.zero, zero);
    put_fq(S.one, one);
    fp_neg<ND>(t, one); put_fq(S.m1, t);
    fp_dbl<ND>(t, one); put_fq(S.two, t);
    fp_neg<ND>(u, t); put_fq(S.m2, u);
    fp_add<ND>(u, t, one); put_fq(S.three, u);
    fp_dbl<ND>(t, t); put_fq(S.four, t);
    fp_dbl<ND>(t, t); fp_neg<ND>(u, t); put_fq(S.m8, u);
    if (S.sixteen >= 0) { fp_dbl<ND>(t, t); put_fq(S.sixteen, t); }
    if (S.half >= 0) { fp_halve<ND>(t, one); put_fq(S.half, t); }
  }
  static PBC_DEV void put_point_state(const WavePointSlots &S, const fq &Px, const fq &Py) {     // V = P
    fq one, t;
    fp_set<ND>(one, fpk<ND>().one);
    put_fq(S.X, Px); put_fq(S.Y, Py); put_fq(S.Z, one); put_fq(S.ZZ, one); put_fq(S.ZZZ, one);
    fp_neg<ND>(t, one); put_fq(S.nZ, t);
    put_fq(S.Px, Px); put_fq(S.Py, Py);
    fp_neg<ND>(t, Py); put_fq(S.nPy, t);
  }

  // ---- lane code between levels (a family's lane_op) ----
  // B = 0 (the value after the easy part of cc_tatepower is +-1) must not poison 1 / (D B): invert D * 1 instead (d_final_exp).
  // B: DEG slots from `from`; B, or 1 in its place, -> DEG slots from `to`
  template <int DEG>
  static PBC_DEV void bzero_test(int from, int to) {
    if (threadIdx.x == 0) {
      fq one, zero;
      fp_set<ND>(one, fpk<ND>().one);
#pragma unroll
      for (int k = 0; k < ND; k++) zero.v[k] = 0;
      fq b[DEG];
      bool b0 = true;
      for (int i = 0; i < DEG; i++) { b[i] = get_fq(from + i); b0 &= fp_is0<ND>(b[i]); }
      for (int i = 0; i < DEG; i++) put_fq(to + i, b0 ? (i ? zero : one) : b[i]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  static PBC_DEV void inversion(int from, int to) {                       // a pairing's only inversion
    if (threadIdx.x == 0) {
      fq n;
      fp_inv<ND>(n, get_fq(from));
      put_fq(to, n);
    }
    __builtin_amdgcn_wave_barrier();
  }

  // ---- the interpreter: entry k + 1 is fetched while entry k runs ----
  // (an entry is the same for every lane: readfirstlane tells the compiler, so that the interpreter's branches are scalar
  // branches and not EXEC-masked regions -- where this compiler's SGPR spills into VGPR lanes go wrong, tools/gpu_faults.md)
  static PBC_DEV uint64_t uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) v), hi = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) (v >> 32));
    return ((uint64_t) hi << 32) | lo;
  }
  template <class T> static PBC_DEV const T *uniform_ptr(const T *p) { return reinterpret_cast<const T *>(uniform64(reinterpret_cast<uint64_t>(p))); }
  // A line of a pairing_pp table ([steps][3][ND] words, pairing_d.cuh d_pp_init_lane): lanes 0-2 fetch a', b', c' when a level
  // starts and put them into the slots TB::line_slot(line) names when it is over -- the fetch hides under the level's multiplications.
  struct Line { uint32_t w[ND]; };
  static PBC_DEV Line line_fetch(const uint32_t *tab, int line) {
    Line r;
    const uint32_t *p = tab + ((size_t) line * 3 + (threadIdx.x < 3 ? threadIdx.x : 0)) * ND;
#pragma unroll
    for (int k = 0; k < ND; k++) r.w[k] = p[k];
    return r;
  }
  static PBC_DEV void line_put(const Line &ln, int line) {
    if constexpr (TB::kLines) {                       // (tables without lines name no slot for one)
      if (threadIdx.x < 3) {
        fq v;
#pragma unroll
        for (int k = 0; k < ND; k++) v.v[k] = ln.w[k];
        put_fq(TB::line_slot(line) + (int) threadIdx.x, v);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  // one LEVEL entry.  LINES: the schedule may flag table lines (tab: the table); false: it has none, and none is looked for
  template <bool LINES>
  static PBC_DEV void run_entry(uint64_t e, const uint32_t *tab) {
    const int T = wave::ent_terms(e);
    const Lev a = ent_a(e), b = ent_b(e);
    const Rows R = T > 4 && (PBC_DW_SPLIT || kSqueeze) ? load_rows4(a, b) : load_rows(a, b);
    if (LINES && wave::ent_has_line(e)) {
      const int line = wave::ent_line(e);
      const Line ln = line_fetch(tab, line);
      exec(R, R, T);
      line_put(ln, line);
    } else {
      exec(R, R, T);
    }
  }
  // runs entries up to OP_END or OP_MARK; returns how many it consumed (the terminator included).  tab: the pairing_pp table
  // the schedule's lines come from (nullptr: a schedule without lines).  What a family lacks is not in its loop: no table
  // (TB::kLines false: type f) -- no table pointer, no line flag on a level, no OP_LOADLINE; no mark in its schedules
  // (Fam::kHasMark false: types d and f) -- OP_END alone ends a run.
  template <class Fam>
  static __device__ __noinline__ int interpret(const uint64_t *sched_, const uint32_t *tab_) {
    const uint64_t *sched = uniform_ptr(sched_);
    constexpr bool kMark = Fam::kHasMark;
    const uint32_t *tab = TB::kLines ? uniform_ptr(tab_) : nullptr;
    uint64_t e = uniform64(sched[0]);
    int k = 1;
    for (;; k++) {
      const int op = wave::ent_op(e);
      const bool last = op == wave::OP_END || (kMark && op == wave::OP_MARK);
#if PBC_DW_WHATIF & 1
      if (!last) { e = uniform64(sched[k]); continue; }
#endif
      if (last) break;
      const uint64_t nxt = uniform64(sched[k]);       // (a scalar load that completes under this entry's work)
      if (op == wave::OP_LEVEL) run_entry<TB::kLines>(e, tab);
      // (an op that lane_op declines is taken for OP_LOADLINE unchecked: the host's builders write no other)
      else if (!Fam::lane_op(op) && TB::kLines) { const int line = wave::ent_line(e); line_put(line_fetch(tab, line), line); }
      e = nxt;
    }
    return __builtin_amdgcn_readfirstlane(k);
  }

  static PBC_DEV void begin() {
    const uint32_t *src = TB::rows_src();
    for (int i = (int) threadIdx.x; i < TB::kRows * 5; i += 64) g_lds_wv<ND, TB>[TB::kSlots * L + i] = src[i];
    for (int i = (int) threadIdx.x; i < TB::kSlots * L; i += 64) g_lds_wv<ND, TB>[i] = 0;
    __builtin_amdgcn_wave_barrier();
  }
  // begin(), then lane 0 sets the slots up; whether the arguments were on their curves waits in LDS for the store: ONE word
  // per workgroup (= wavefront), written by lane 0 before the barrier in start(), read by every lane after the interpreter
  // (no register is held across that call)
  static PBC_DEV int &valid_flag() { __shared__ int valid_s; return valid_s; }
  template <class Fam>
  static PBC_DEV void start(const uint8_t *g1, const uint8_t *g2) {
    begin();
    if (threadIdx.x == 0) { Fam::setup_consts(); valid_flag() = Fam::setup_inputs(g1, g2) ? 1 : 0; }
    __builtin_amdgcn_wave_barrier();
  }
  template <class Fam>
  static PBC_DEV void store_gt(uint8_t *gt, bool valid) {
    if (threadIdx.x < Fam::kCoef) {
      fq o = get_fq(Fam::kF + (int) threadIdx.x);     // the coefficients of f are consecutive slots in GT's wire order
      if (!valid) {                                   // an input that deserialises to O: the identity of GT
        fq one;
        fp_set<ND>(one, fpk<ND>().one);
#pragma unroll
        for (int k = 0; k < ND; k++) o.v[k] = threadIdx.x == 0 ? one.v[k] : 0u;
      }
      fp_store_be<ND>(gt + (size_t) threadIdx.x * fpk<ND>().fbytes, o);
    }
  }
  // A RECORD of a product's workspace: the Miller value of one term -- the kCoef slots of f as they are -- then the validity flag
  static constexpr int rec_words(int coef) { return (coef * L + 1 + 7) & ~7; }
  template <class Fam> struct Rec { static constexpr int kPerLane = (Fam::kCoef * L + 63) / 64; uint32_t w[kPerLane]; };      // a lane's words of a record's value
  template <class Fam>
  static PBC_DEV void rec_write(uint32_t *rec, int valid) {
    for (int i = (int) threadIdx.x; i < Fam::kCoef * L; i += 64) rec[i] = slot(Fam::kF)[i];
    if (threadIdx.x == 0) rec[Fam::kCoef * L] = (uint32_t) valid;
  }
  template <class Fam>
  static PBC_DEV Rec<Fam> rec_read(const uint32_t *rec) {
    Rec<Fam> r;
#pragma unroll
    for (int j = 0; j < Rec<Fam>::kPerLane; j++) { const int i = (int) threadIdx.x + 64 * j; r.w[j] = rec[i < Fam::kCoef * L ? i : 0]; }
    return r;
  }
  template <class Fam>
  static PBC_DEV void rec_put(int s, const Rec<Fam> &r) {
#pragma unroll
    for (int j = 0; j < Rec<Fam>::kPerLane; j++) { const int i = (int) threadIdx.x + 64 * j; if (i < Fam::kCoef * L) slot(s)[i] = r.w[j]; }
  }

  // entries J .. NP - 1 of pe, one copy of the level's code each (a loop this large is not unrolled on request)
  template <int J, int NP>
  static PBC_DEV void run_held(const uint64_t *pe) {
    if constexpr (J < NP) { run_entry<false>(pe[J], nullptr); run_held<J + 1, NP>(pe); }
  }

  // ---- the drivers ----
  // element_pairing
  template <class Fam>
  static __device__ void pairing(uint8_t *gt, const uint8_t *g1, const uint8_t *g2, const uint64_t *sched) {
    start<Fam>(g1, g2);
    interpret<Fam>(sched, nullptr);
    store_gt<Fam>(gt, valid_flag() != 0);
  }
  // element_prod_pairing, first kernel: the Miller value of ONE TERM -> its record of the workspace.  (The reference squares
  // one accumulator for all terms, or multiplies reduced pairings; the product of the terms' own Miller values is the same
  // element up to factors the final exponentiation removes.)
  template <class Fam>
  static __device__ void miller_term(uint32_t *rec, const uint8_t *g1, const uint8_t *g2, const uint64_t *sched) {
    start<Fam>(g1, g2);
    interpret<Fam>(sched, nullptr);
    rec_write<Fam>(rec, valid_flag());
  }
  // second kernel: f <- the product of the k records, then the final exponentiation; any invalid term: the identity.  Each
  // further record goes to the slots Fam::kOperand and the schedule's first entries multiply it in: Fam::kProdEntries of them,
  // held in registers, or, where that is 0, the entries up to the schedule's OP_MARK, interpreted again for every term.
  // Fam::kFinishPrefetch: record t + 1 is in flight while record t is multiplied in.
  template <class Fam>
  static __device__ void finish(uint8_t *gt, const uint32_t *recs, int k, const uint64_t *sched_) {
    constexpr int NP = Fam::kProdEntries, W = Fam::kCoef * L, kRec = rec_words(Fam::kCoef);
    static_assert(NP > 0 || Fam::kHasMark, "the product's entries: held in registers, or ended by a mark");
    const uint64_t *sched = uniform_ptr(sched_);
    begin();
    if (threadIdx.x == 0) Fam::setup_consts();
    __builtin_amdgcn_wave_barrier();
    bool valid = recs[W] != 0;
    rec_put<Fam>(Fam::kF, rec_read<Fam>(recs));
    uint64_t pe[NP > 0 ? NP : 1];                      // types d (2) and f (3): the product's entries, read once, wave-uniform (SGPRs)
#pragma unroll
    for (int j = 0; j < NP; j++) pe[j] = uniform64(sched[j]);
    int used = NP;
    Rec<Fam> nxt;
    if constexpr (Fam::kFinishPrefetch) nxt = rec_read<Fam>(recs + (k > 1 ? kRec : 0));      // type d: record 1 (k = 1: record 0 again, unused)
    for (int t = 1; t < k; t++) {
      const uint32_t *r = recs + (size_t) t * kRec;
      valid &= r[W] != 0;
      if constexpr (!Fam::kFinishPrefetch) nxt = rec_read<Fam>(r);                           // types f and g: record t, now
      rec_put<Fam>(Fam::kOperand, nxt);
      __builtin_amdgcn_wave_barrier();
      if constexpr (Fam::kFinishPrefetch) { if (t + 1 < k) nxt = rec_read<Fam>(r + kRec); }  // type d: record t + 1 in flight during the levels
      if constexpr (NP > 0) run_held<0, NP>(pe);                                             // types d and f
      else used = interpret<Fam>(sched, nullptr);                                            // type g: up to the mark
    }
    if constexpr (NP == 0) {                           // type g: where the final exponentiation begins
      if (k < 2) {                                     // (never routed here; skip the product's entries)
        for (used = 0; wave::ent_op(uniform64(sched[used])) != wave::OP_MARK; used++) {}
        used++;
      }
    }
    __builtin_amdgcn_wave_barrier();
    interpret<Fam>(sched + used, nullptr);
    store_gt<Fam>(gt, valid);
  }
  // pairing_pp_apply: the lines' coefficients come from the table of pairing_pp_init (pairing_d.cuh d_pp_init_lane), no
  // arithmetic on E(F_q)
  template <class Fam>
  static __device__ void pp_apply(uint8_t *gt, const uint32_t *tab, bool p_valid, const uint8_t *g2, const uint64_t *sched) {
    start<Fam>(nullptr, g2);
    interpret<Fam>(sched, tab);
    store_gt<Fam>(gt, p_valid && valid_flag() != 0);
  }
};

}  // namespace pbc
