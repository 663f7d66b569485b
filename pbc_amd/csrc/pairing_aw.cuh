// pairing_aw.cuh -- element_pairing, type a (512-bit q), ONE PAIRING PER WAVEFRONT: the low-latency path for small
// batches (include/pbc_hip.h "batch sizes").  The throughput kernels (pairing_al.cuh) give every lane a whole pairing:
// 2.1 M dependent multiply-adds, 6.4 ms however small the batch.  Here an F_q element is ONE register: lane j of the
// wave holds limb j (29 bits, 18 lanes in use), sums and differences are single instructions, and the Montgomery
// product runs across the lanes:
//     for i in 0..17:   acc_j += a_i b_j          a_i: v_readlane -> SGPR operand of v_mad_u64_u32
//                       m = acc_0 (-1/q) mod 2^29  v_readfirstlane
//                       acc_j += m q_j
//                       acc_j = (acc_j >> 29) + (acc_{j+1} mod 2^29)      one DPP wave shift
// Lane j holds column i + j in step i: its own carry is already where it belongs after the shift, only the low 29
// bits travel, and what a lane keeps between steps fits 32 bits.  After 18 steps lane j holds limb j of
// a b / R + (multiple of q); carry passes (DPP, wave-uniform loop on a ballot) bring the limbs below 2^29.  Seven
// vector instructions per step; about 1 300 cycles per product against 5 900 for the 648 multiply-adds of a lane-local
// product at one wave per SIMD.
// The final exponentiation is AL<N>'s, operation for operation (same sums, same borrowed constants, same
// normalisations, hence the same bounds -- in the host mirror an element IS an AL<N>::el and carries AL's worst-case
// tracker through these routines).  The Miller steps (double_step, add_step below) are the JACOBIAN ones AL<N> had
// before it moved to weight-(1, 2) coordinates (pairing_al.cuh): the two paths' Miller values now differ by factors
// in F_q^*, which the final exponentiation removes, so they still agree bit for bit on every input, the invalid
// ones included; the one inversion runs AL's divsteps routine on lane 0 (a Fermat ladder on the wave's products,
// `invert`, is kept for reference: 0.32 against 0.14 ms).
// Boundaries (bytes <-> limbs, validity, the final halvings) run the word-form routines on lane 0 through LDS.
#pragma once
#ifndef PBC_AW_INV_LANE0
#define PBC_AW_INV_LANE0 0          // 1: invert_lane0 calls fp_inv under a lane-0-only EXEC mask (faulted in round 4; tools/gpu_faults.md)
#endif
#include "pairing_al.cuh"

namespace pbc {

constexpr int AW_SLOTS = 24;                 // LDS words per workgroup: AW_SLOTS x 64 (5 inputs / 2 outputs, the inversion, 2 x 4 -- NW = 8: 2 x 8 -- products of a round); a slot holds all 64 lanes, so no access is predicated
#ifndef PBC_HOSTSIM
template <int N> __shared__ uint32_t g_lds_aw_t[AW_SLOTS * 64];
#define g_lds_aw g_lds_aw_t<N>
#endif

// Round 6: the same routines for type a1 and for type a parameters outside the 512-bit Solinas fast path (AG<N> below in place
// of AL<N>): the Miller loop walks the signed digits of the group order (pairing_a.cuh a1_miller_lane), the limbs are W = 29 or 28
// bits wide (fp.cuh Limbs29: 38 limbs of 28 bits on the 33-word fields, one lane each), the subtraction constants and the
// number of limbs q really fills (LEFF: a 1033-bit p leaves the 38th limb empty, so the borrow is taken from the 37th) come
// from a table the host builds per object (host_params.h ag_aux_build), and the records are fq_bytes long.  The host mirror
// runs these instantiations too (AG<N>'s mirror below: AL's bound tracker with the object's own limb width, filled limbs,
// top-limb fill and radix slack), so the bounds are checked per object, not carried over; the host admits a q that fills twelve
// bits of its top limb and leaves ten bits of the radix free, and keeps the lane kernels otherwise.
template <int N>
struct AG {
  static constexpr int L = Limbs29<N>::L;
  static constexpr int WB = Limbs29<N>::W;
  static constexpr uint32_t MASK = Limbs29<N>::MASK;
  static constexpr bool kDigits = true;
  typedef fl<N> el;
  enum { K2 = 0, K4 = 1, K8 = 2, K12 = 3, K16 = 4 };
#ifndef PBC_HOSTSIM
  static PBC_DEV void to_el(el &r, const fp<N> &a) { to_limbs<N>(r, a); }
  static PBC_DEV void to_words(fp<N> &r, const el &a) { from_limbs<N>(r, a); }
#else
  // ---- host mirror: AL<N>'s additive layer and worst-case bound tracker (pairing_al.cuh) for ANY field the table admits: W-bit
  // limbs, LEFF of them filled, the borrowed constants from the object's table, the two assumptions about q as numbers -- q fills
  // `top` bits of limb LEFF - 1 (hs_topf = 2^(top - 1): what a multiple of q is worth in units of that limb) and leaves `slack`
  // bits of the radix (hs_slackf = 2^slack: what a product's value shrinks by).  tests/hostsim sets them from the object.
  static inline const uint32_t *hs_tab = nullptr;
  static inline int hs_leff = L;
  static inline double hs_topf = 2048.0, hs_slackf = 1024.0;
  static constexpr double UNIT = (double) (1u << WB), OVF = 4294967296.0 / UNIT;          // limbs are tracked in units of 2^W; 32-bit limbs hold OVF units
  static constexpr double U_STRICT = 1.0 - 1.0 / UNIT, U_ALMOST = 1.0 + 7.0 / UNIT;
  static constexpr double KC[5] = {2, 4, 8, 12, 16}, KD[5] = {1, 2, 4, 2, 2};
  static int leff_() { return hs_leff; }
  static double hs_slack() { return hs_slackf; }
  static void hs_fail(const char *what, double v) { fprintf(stderr, "hostsim: wave kernels of type a1 / e: %s (%g)\n", what, v); abort(); }
  static void hs_limbs(const el &a) {
    for (int i = 0; i < L; i++)
      if ((double) a.l[i] > a.hs_u * UNIT) hs_fail("limb above its tracked bound", a.hs_u);
    for (int i = hs_leff; i < L; i++)
      if (a.l[i]) hs_fail("limb above the ones q fills", (double) i);
  }
  static void hs_set(el &r, double u, double B) { r.hs_u = u; r.hs_B = B; hs_limbs(r); }
  static void hs_dom(const el &b, int k) {
    hs_limbs(b);
    if (b.hs_u > KD[k] * U_STRICT + 1e-12) hs_fail("subtrahend limbs not dominated", b.hs_u);
    if ((KC[k] - b.hs_B) * hs_topf < KD[k] + 1) hs_fail("subtrahend value not dominated", b.hs_B);
  }
  static void hs_cols(double s) { if (s > 2.55) hs_fail("column capacity", s); }
  static void add(el &r, const el &a, const el &b) {
    for (int i = 0; i < L; i++) r.l[i] = a.l[i] + b.l[i];
    if (a.hs_u + b.hs_u >= OVF) hs_fail("sum overflows 32 bits", a.hs_u + b.hs_u);
    hs_set(r, a.hs_u + b.hs_u, a.hs_B + b.hs_B);
  }
  template <int S> static void shl(el &r, const el &a) {
    for (int i = 0; i < L; i++) r.l[i] = a.l[i] << S;
    if (a.hs_u * (1 << S) >= OVF) hs_fail("shift overflows 32 bits", a.hs_u);
    hs_set(r, a.hs_u * (1 << S), a.hs_B * (1 << S));
  }
  static void subk(el &r, const el &a, const el &b, int k) {
    const uint32_t *K = hs_tab + AW_AUX_HEAD + k * L;
    hs_dom(b, k);
    const double u = a.hs_u + KD[k] + 1, B = a.hs_B + KC[k];
    if (u >= OVF) hs_fail("difference overflows 32 bits", u);
    for (int i = 0; i < L; i++) {
      if (K[i] < b.l[i]) hs_fail("negative limb in a difference", (double) i);
      r.l[i] = a.l[i] - b.l[i] + K[i];
    }
    hs_set(r, u, B);
  }
  static void negk(el &r, const el &b, int k) {
    const uint32_t *K = hs_tab + AW_AUX_HEAD + k * L;
    hs_dom(b, k);
    for (int i = 0; i < L; i++) {
      if (K[i] < b.l[i]) hs_fail("negative limb in a negation", (double) i);
      r.l[i] = K[i] - b.l[i];
    }
    hs_set(r, KD[k] + 1, KC[k]);
  }
  static void norm(el &r, const el &a) {                       // AW::norm_m with init()'s masks: one parallel carry pass
    hs_limbs(a);
    const double B = a.hs_B;
    if (a.hs_u >= OVF) hs_fail("normalising limbs above 32 bits", a.hs_u);
    uint32_t c = 0;
    for (int i = 0; i < L; i++) {
      const uint32_t t = a.l[i];
      r.l[i] = (i < hs_leff - 1 ? (t & MASK) : (i == hs_leff - 1 ? t : 0u)) + c;
      c = i < hs_leff - 1 ? t >> WB : 0u;
    }
    hs_set(r, U_ALMOST, B);
  }
  static void to_el(el &r, const fp<N> &a) { to_limbs<N>(r, a); hs_set(r, U_STRICT, 1.0); }
  static void to_words(fp<N> &r, const el &a) {
    hs_limbs(a);
    if (a.hs_u > U_STRICT || a.hs_B >= 2) hs_fail("from_limbs needs a P-class value", a.hs_B);
    from_limbs<N>(r, a);
  }
  static void to_el_uniform(el &r, const uint32_t *w) {
    for (int i = 0; i < L; i++) {
      const int bit = WB * i, j = bit >> 5, sh = bit & 31;
      const uint64_t pair = ((uint64_t) (j + 1 < N ? w[j + 1] : 0u) << 32) | w[j];
      r.l[i] = (uint32_t) (pair >> sh) & MASK;
    }
    hs_set(r, U_STRICT, 1.0);
  }
#endif
};

template <int N, int NW = 1, class A_ = AL<N>>   // NW: wavefronts that work on ONE pairing (1, 2 or 4 = a 128- / 256-lane workgroup: see round_nw)
struct AW {
  typedef A_ A;
  typedef typename A::el el;
  static constexpr int L = A::L;
  static constexpr int WB = Limbs29<N>::W;     // bits of a limb
  static constexpr uint32_t MASK = A::MASK;
  static constexpr bool kDigits = A::kDigits;  // the Miller loop over signed digits (type a1 / generic type a) instead of the Solinas loop
  enum { K2 = A::K2, K4 = A::K4, K8 = A::K8, K12 = A::K12, K16 = A::K16 };
  static PBC_DEV int fq_len() { if constexpr (kDigits) return (int) fpk<N>().fbytes; else return 4 * N; }   // bytes of a coordinate record

#ifdef PBC_HOSTSIM
  // ---- host mirror: an element is all L limbs (AL's el with its tracker); the lanes run in a loop ------------------
  typedef el W;
  void init() {}
  static W add(const W &a, const W &b) { W r; A::add(r, a, b); return r; }
  template <int S> static W shl(const W &a) { W r; A::template shl<S>(r, a); return r; }
  static W subk(const W &a, const W &b, int k) { W r; A::subk(r, a, b, k); return r; }
  static W negk(const W &b, int k) { W r; A::negk(r, b, k); return r; }
  static W norm(const W &a) { W r; A::norm(r, a); return r; }
  // the lane recurrence of the device product, lanes 0 .. L (lane L: the zero lane above the top limb)
  static void lanes_sop(W &r, const W *a, const W *b, int terms) {
    const FpK<N> &K = fpk<N>();
    uint64_t acc[L + 1] = {0};
    PBC_COUNT_MACS((terms + 1) * L * L);
    for (int i = 0; i < L; i++) {
      for (int t = 0; t < terms; t++)
        for (int j = 0; j < L; j++) {
          const uint64_t p = (uint64_t) a[t].l[i] * b[t].l[j];
          if (acc[j] + p < p) A::hs_fail("wave product: accumulator overflow", (double) i);
          acc[j] += p;
        }
      const uint32_t m = ((uint32_t) acc[0] * K.ninv29) & MASK;
      for (int j = 0; j < L; j++) acc[j] += (uint64_t) m * K.p29[j];
      uint32_t lo[L + 1];
      for (int j = 0; j <= L; j++) lo[j] = (uint32_t) acc[j] & MASK;
      if (lo[0]) A::hs_fail("wave product: column not cleared", (double) i);
      for (int j = 0; j < L; j++) {
        if (acc[j] >> 60) A::hs_fail("wave product: accumulator above 2^60", (double) i);
        acc[j] = (acc[j] >> WB) + lo[j + 1];                   // 32 bits on the device
        if (acc[j] >> 32) A::hs_fail("wave product: carried limb above 32 bits", (double) j);
      }
    }
    for (int j = 0; j < L; j++) {
      if (acc[j] >> 32) A::hs_fail("wave product: limb above 32 bits", (double) j);
      r.l[j] = (uint32_t) acc[j];
    }
    strict_limbs(r);
  }
  static void strict_limbs(W &r) {            // carry passes until every limb below the top is under 2^W (the device's masks: AW::init)
    const int le = A::leff_();
    for (;;) {
      bool any = false;
      uint32_t c = 0;
      for (int j = 0; j < L; j++) {
        const uint32_t t = r.l[j];
        r.l[j] = (j < le - 1 ? (t & MASK) : (j == le - 1 ? t : 0u)) + c;
        c = j < le - 1 ? t >> WB : 0;
      }
      for (int j = 0; j < le - 1; j++) any |= r.l[j] > MASK;
      if (!any) break;
    }
  }
  static W mul(const W &a, const W &b) {
    W r;
    A::hs_limbs(a); A::hs_limbs(b); A::hs_cols(a.hs_u * b.hs_u);
    const double B = 1 + a.hs_B * b.hs_B / A::hs_slack();
    lanes_sop(r, &a, &b, 1);
    A::hs_set(r, A::U_STRICT, B);
    return r;
  }
  static W sqr(const W &a) { return mul(a, a); }
  static W sop2(const W &a0, const W &b0, const W &a1, const W &b1) {
    W r;
    const W x[2] = {a0, a1}, y[2] = {b0, b1};
    A::hs_limbs(a0); A::hs_limbs(b0); A::hs_limbs(a1); A::hs_limbs(b1); A::hs_cols(a0.hs_u * b0.hs_u + a1.hs_u * b1.hs_u);
    const double B = 1 + (a0.hs_B * b0.hs_B + a1.hs_B * b1.hs_B) / A::hs_slack();
    lanes_sop(r, x, y, 2);
    A::hs_set(r, A::U_STRICT, B);
    return r;
  }
  static void mul2(W &r0, W &r1, const W &a, const W &b, const W &c, const W &d) { const W x = mul(a, b), y = mul(c, d); r0 = x; r1 = y; }
  static void sop2x2(W &r0, W &r1, const W &a0, const W &b0, const W &a1, const W &b1, const W &c0, const W &d0, const W &c1, const W &d1) {
    const W x = sop2(a0, b0, a1, b1), y = sop2(c0, d0, c1, d1);
    r0 = x; r1 = y;
  }
  // x >= q ?  and  x - q  (x: strict limbs, value < 2q)
  static bool geq_q(const W &x) {
    const FpK<N> &K = fpk<N>();
    for (int j = L - 1; j >= 0; j--) if (x.l[j] != K.p29[j]) return x.l[j] > K.p29[j];
    return true;
  }
  static W sub_q(const W &x) {
    const FpK<N> &K = fpk<N>();
    W r;
    const int le = A::leff_();
    for (int j = 0; j < L; j++) r.l[j] = x.l[j] - K.p29[j] + (j < le - 1 ? (1u << WB) : 0) - (j > 0 && j < le ? 1 : 0);
    strict_limbs(r);
    A::hs_set(r, A::U_STRICT, 1.0);
    return r;
  }
  static bool is_zero(const W &x) { for (int j = 0; j < L; j++) if (x.l[j]) return false; return true; }
  static void mul4(W &r0, W &r1, W &r2, W &r3, const W &a0, const W &b0, const W &a1, const W &b1, const W &a2, const W &b2,
                   const W &a3, const W &b3, int count) {
    const W x = mul(a0, b0), y = mul(a1, b1), z = count > 2 ? mul(a2, b2) : a2, t = count > 3 ? mul(a3, b3) : a3;
    r0 = x; r1 = y;
    if (count > 2) r2 = z;
    if (count > 3) r3 = t;
  }
  static void round8(W *r, const W *a0, const W *b0, const W *a1, const W *b1, int count, unsigned sums) {
    W t[8];
    for (int k = 0; k < count; k++) t[k] = ((sums >> k) & 1) ? sop2(a0[k], b0[k], a1[k], b1[k]) : mul(a0[k], b0[k]);
    for (int k = 0; k < count; k++) r[k] = t[k];
  }
  static bool lane0() { return true; }
  static void sync() {}
  static W load_uniform(const uint32_t *w) { W r; A::to_el_uniform(r, w); return r; }
#else
  // ---- device: one limb per lane ----------------------------------------------------------------------------------
  typedef uint32_t W;
  // lane masks of the carry pass: mr = what a lane keeps (2^29 - 1 below the top limb, everything in the top limb,
  // nothing above it), cm = whose carry travels (all ones below the top limb)
  struct masks { uint32_t mr, cm; };
  W kk[5], qq;                                                 // this lane's limb of the five borrowed constants and of q
  uint32_t nv;                                                 // -1/q mod 2^29
  masks mk;
  int par = 0;                                                 // which set of round slots is written next (NW > 1)
  const uint32_t *aux = nullptr;                               // AG: the object's table (LEFF, five constants of L limbs)
  int leff = L;                                                // limbs q fills (the top one takes the borrows and keeps the carries)
  PBC_DEV void init() {
    const int j = lane();
    if constexpr (kDigits) {
      leff = __builtin_amdgcn_readfirstlane((int) aux[0]);
#pragma unroll
      for (int k = 0; k < 5; k++) kk[k] = j < L ? aux[AW_AUX_HEAD + k * L + j] : 0u;
    } else {
#pragma unroll
      for (int k = 0; k < 5; k++) kk[k] = j < L ? c_a.ksub[k][j] : 0u;
    }
    qq = j < L ? fpk<N>().p29[j] : 0u;
    nv = fpk<N>().ninv29;
    mk.mr = j < leff - 1 ? MASK : (j == leff - 1 ? 0xffffffffu : 0u);
    mk.cm = j < leff - 1 ? 0xffffffffu : 0u;
  }
  static PBC_DEV int lane() { return (int) (threadIdx.x & 63); }
  static PBC_DEV W from_above(W x) { return (W) __builtin_amdgcn_update_dpp(0, (int) x, 0x130, 0xf, 0xf, true); }   // wave_shl:1 : lane j <- lane j + 1
  static PBC_DEV W from_below(W x) { return (W) __builtin_amdgcn_update_dpp(0, (int) x, 0x138, 0xf, 0xf, true); }   // wave_shr:1 : lane j <- lane j - 1
  static PBC_DEV W add(W a, W b) { return a + b; }
  template <int S> static PBC_DEV W shl(W a) { return a << S; }
  PBC_DEV W subk(W a, W b, int k) const { return a - b + kk[k]; }
  PBC_DEV W negk(W b, int k) const { return kk[k] - b; }
  static PBC_DEV W norm_m(W a, masks k) { return (a & k.mr) + from_below((a >> WB) & k.cm); }
  static PBC_DEV W strict_limbs(W x, masks k) {
    for (;;) {
      x = norm_m(x, k);
      if (__ballot((x & ~k.mr & k.cm) != 0) == 0) break;
    }
    return x;
  }
  PBC_DEV W norm(W a) const { return norm_m(a, mk); }
  // One step of the recurrence for accumulator `acc` (see the head of the file).  Accumulators stay below 2^61 (column
  // sums <= 2.55 2^58 + m q: AL's hs_cols), so acc >> 29 is one v_alignbit.  (Forming m on the scalar unit from acc_0's
  // low word and b_0 (-1/q) -- so that the two multiply-adds issue back to back -- measured 9 % SLOWER: 2.75 against
  // 2.52 ms per pairing; the scalar multiplies sit on the same dependency chain.)
  template <int TERMS>
  static PBC_DEV void lanes_step(uint32_t &nxt, uint32_t x0, W b0, uint32_t x1, W b1, W q, uint32_t ninv) {
    uint64_t acc = (uint64_t) x0 * b0 + nxt;
    if (TERMS == 2) acc += (uint64_t) x1 * b1;
    const uint32_t m = ((uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) acc) * ninv) & MASK;   // scalar unit
    acc += (uint64_t) m * q;
    const uint32_t c = __builtin_amdgcn_alignbit((uint32_t) (acc >> 32), (uint32_t) acc, WB);   // < 2^31: acc < 2^60
    nxt = c + from_above((uint32_t) acc & MASK);
  }
  template <int TERMS>
  static PBC_DEV W lanes_sop(W a0, W b0, W a1, W b1, W q, uint32_t nv, masks k) {
    const uint32_t ninv = (uint32_t) __builtin_amdgcn_readfirstlane((int) nv);   // handed down in a register: a scalar load here stalls every product
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < L; i++)
      lanes_step<TERMS>(acc, (uint32_t) __builtin_amdgcn_readlane((int) a0, i), b0, TERMS == 2 ? (uint32_t) __builtin_amdgcn_readlane((int) a1, i) : 0u, b1, q, ninv);
    return strict_limbs(acc, k);
  }
  // two independent sums of products in one instruction stream: the dependency chain of a step (multiply-add, m,
  // multiply-add, shift: eight instructions of ~9 cycles each at one wave per SIMD) leaves the pipe half empty
  struct W2 { W r0, r1; };
  template <int TERMS>
  static PBC_DEV W2 lanes_sop_x2(W a0, W b0, W a1, W b1, W c0, W d0, W c1, W d1, W q, uint32_t nv, masks k) {
    const uint32_t ninv = (uint32_t) __builtin_amdgcn_readfirstlane((int) nv);
    uint32_t acc = 0, bcc = 0;
#pragma unroll
    for (int i = 0; i < L; i++) {
      lanes_step<TERMS>(acc, (uint32_t) __builtin_amdgcn_readlane((int) a0, i), b0, TERMS == 2 ? (uint32_t) __builtin_amdgcn_readlane((int) a1, i) : 0u, b1, q, ninv);
      lanes_step<TERMS>(bcc, (uint32_t) __builtin_amdgcn_readlane((int) c0, i), d0, TERMS == 2 ? (uint32_t) __builtin_amdgcn_readlane((int) c1, i) : 0u, d1, q, ninv);
    }
    W x = acc, y = bcc;
    for (;;) {
      x = norm_m(x, k);
      y = norm_m(y, k);
      if (__ballot(((x | y) & ~k.mr & k.cm) != 0) == 0) break;
    }
    return W2{x, y};
  }
  static __device__ __noinline__ W2 mul2_fn(W a, W b, W c, W d, W q, uint32_t nv, masks k) { return lanes_sop_x2<1>(a, b, 0, 0, c, d, 0, 0, q, nv, k); }
  static __device__ __noinline__ W2 sop2x2_fn(W a0, W b0, W a1, W b1, W c0, W d0, W c1, W d1, W q, uint32_t nv, masks k) { return lanes_sop_x2<2>(a0, b0, a1, b1, c0, d0, c1, d1, q, nv, k); }
  // ---- a ROUND: up to four independent products ------------------------------------------------------------------
  // NW = 1: two at a time in one instruction stream.  NW = 4 (one pairing per 256-lane workgroup, a wave on each SIMD of
  // the CU; every wave carries the whole state and repeats the additions): wave w forms product w, writes it to its
  // LDS slot, ONE barrier, every wave reads all of them.  The slots alternate between two sets, so a wave that is a
  // round ahead writes where nobody reads.
  static PBC_DEV int wave() { return NW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)); }
  template <int TERMS>
  PBC_DEV void round_nw(W *r, const W *a0, const W *b0, const W *a1, const W *b1, int count) {
    const int w = wave();
    const int base = 6 + 4 * par;
    if constexpr (NW == 2) {
      // two wavefronts per pairing (round 5): wave w forms products w and w + 2 -- both in ONE instruction stream when it
      // has two (lanes_sop_x2: the dependency chain of a step leaves the pipe half empty) -- so a round of four costs each
      // wave one double product instead of four waves one single product each and a barrier with two of them idle
      const bool two = w + 2 < count;                          // wave-uniform
      if (w < count) {
        const W x0 = w ? a0[1] : a0[0], y0 = w ? b0[1] : b0[0], x2 = w ? a0[3] : a0[2], y2 = w ? b0[3] : b0[2];
        if (TERMS == 1) {
          if (two) {
            const W2 t = mul2_fn(x0, y0, x2, y2, qq, nv, mk);
            put_slot(t.r0, base + w);
            put_slot(t.r1, base + w + 2);
          } else {
            put_slot(mul_fn(x0, y0, qq, nv, mk), base + w);
          }
        } else {                                               // (sums of two products come in pairs: count == 2)
          const W x1 = w ? a1[1] : a1[0], y1 = w ? b1[1] : b1[0];
          put_slot(sop2_fn(x0, y0, x1, y1, qq, nv, mk), base + w);
        }
      }
    } else if (w < count) {
      W x0, y0, x1 = 0u, y1 = 0u;                                 // w is wave-uniform: a scalar branch, no per-lane selects
      switch (w) {
        case 0: x0 = a0[0]; y0 = b0[0]; if (TERMS == 2) { x1 = a1[0]; y1 = b1[0]; } break;
        case 1: x0 = a0[1]; y0 = b0[1]; if (TERMS == 2) { x1 = a1[1]; y1 = b1[1]; } break;
        case 2: x0 = a0[2]; y0 = b0[2]; if (TERMS == 2) { x1 = a1[2]; y1 = b1[2]; } break;
        default: x0 = a0[3]; y0 = b0[3]; if (TERMS == 2) { x1 = a1[3]; y1 = b1[3]; } break;
      }
      const W res = TERMS == 1 ? mul_fn(x0, y0, qq, nv, mk) : sop2_fn(x0, y0, x1, y1, qq, nv, mk);
      put_slot(res, base + w);
    }
    sync();
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < count) r[k] = get_slot(base + k);
    par ^= 1;
  }
  // NW = 8 (round 6: a 512-lane workgroup, two wavefronts on every SIMD of the CU -- a lone wave's dependency chain leaves the pipe
  // half empty, so the second one rides along): up to EIGHT items a round, each a product or -- bit k of `sums` -- a sum of two
  PBC_DEV void round8(W *r, const W *a0, const W *b0, const W *a1, const W *b1, int count, unsigned sums) {
    if constexpr (NW == 8) {
      const int w = wave();
      const int base = 6 + 8 * par;
      if (w < count) {
        W x0, y0, x1, y1;
        switch (w) {                                           // (w is wave-uniform: scalar branches, no indexed register file)
          case 0: x0 = a0[0]; y0 = b0[0]; x1 = a1[0]; y1 = b1[0]; break;
          case 1: x0 = a0[1]; y0 = b0[1]; x1 = a1[1]; y1 = b1[1]; break;
          case 2: x0 = a0[2]; y0 = b0[2]; x1 = a1[2]; y1 = b1[2]; break;
          case 3: x0 = a0[3]; y0 = b0[3]; x1 = a1[3]; y1 = b1[3]; break;
          case 4: x0 = a0[4]; y0 = b0[4]; x1 = a1[4]; y1 = b1[4]; break;
          case 5: x0 = a0[5]; y0 = b0[5]; x1 = a1[5]; y1 = b1[5]; break;
          case 6: x0 = a0[6]; y0 = b0[6]; x1 = a1[6]; y1 = b1[6]; break;
          default: x0 = a0[7]; y0 = b0[7]; x1 = a1[7]; y1 = b1[7]; break;
        }
        const bool sum = ((sums >> w) & 1u) != 0;                // wave-uniform
        const W res = sum ? sop2_fn(x0, y0, x1, y1, qq, nv, mk) : mul_fn(x0, y0, qq, nv, mk);
        put_slot(res, base + w);
      }
      sync();
#pragma unroll
      for (int k = 0; k < 8; k++) if (k < count) r[k] = get_slot(base + k);
      par ^= 1;
    } else {                                                   // (fewer waves: one after the other, every wave for itself)
      for (int k = 0; k < count; k++) r[k] = ((sums >> k) & 1u) ? sop2(a0[k], b0[k], a1[k], b1[k]) : mul(a0[k], b0[k]);
    }
  }
  PBC_DEV void mul4(W &r0, W &r1, W &r2, W &r3, W a0, W b0, W a1, W b1, W a2, W b2, W a3, W b3, int count) {
    if constexpr (NW == 1) {
      const W2 t = mul2_fn(a0, b0, a1, b1, qq, nv, mk);
      r0 = t.r0; r1 = t.r1;
      if (count == 3) r2 = mul_fn(a2, b2, qq, nv, mk);
      if (count == 4) { const W2 u = mul2_fn(a2, b2, a3, b3, qq, nv, mk); r2 = u.r0; r3 = u.r1; }
    } else {
      W r[4];
      const W a[4] = {a0, a1, a2, a3}, b[4] = {b0, b1, b2, b3};
      round_nw<1>(r, a, b, a, b, count);
      r0 = r[0]; r1 = r[1];
      if (count > 2) r2 = r[2];
      if (count > 3) r3 = r[3];
    }
  }
  PBC_DEV void mul2(W &r0, W &r1, W a, W b, W c, W d) {
    if constexpr (NW == 1) { const W2 t = mul2_fn(a, b, c, d, qq, nv, mk); r0 = t.r0; r1 = t.r1; }
    else { W r2, r3; mul4(r0, r1, r2, r3, a, b, c, d, 0u, 0u, 0u, 0u, 2); }
  }
  PBC_DEV void sop2x2(W &r0, W &r1, W a0, W b0, W a1, W b1, W c0, W d0, W c1, W d1) {
    if constexpr (NW == 1) { const W2 t = sop2x2_fn(a0, b0, a1, b1, c0, d0, c1, d1, qq, nv, mk); r0 = t.r0; r1 = t.r1; }
    else {
      W r[4];
      const W x0[4] = {a0, c0, 0u, 0u}, y0[4] = {b0, d0, 0u, 0u}, x1[4] = {a1, c1, 0u, 0u}, y1[4] = {b1, d1, 0u, 0u};
      round_nw<2>(r, x0, y0, x1, y1, 2);
      r0 = r[0]; r1 = r[1];
    }
  }
  static __device__ __noinline__ W mul_fn(W a, W b, W q, uint32_t nv, masks k) { return lanes_sop<1>(a, b, 0, 0, q, nv, k); }
  static __device__ __noinline__ W sop2_fn(W a0, W b0, W a1, W b1, W q, uint32_t nv, masks k) { return lanes_sop<2>(a0, b0, a1, b1, q, nv, k); }
  PBC_DEV W mul(W a, W b) const { return mul_fn(a, b, qq, nv, mk); }
  PBC_DEV W sqr(W a) const { return mul_fn(a, a, qq, nv, mk); }
  PBC_DEV W sop2(W a0, W b0, W a1, W b1) const { return sop2_fn(a0, b0, a1, b1, qq, nv, mk); }
  PBC_DEV bool geq_q(W x) const {
    const uint32_t q = qq;
    const uint64_t gt = __ballot(x > q), lt = __ballot(x < q);
    return gt >= lt;                                           // the highest differing limb decides; equal: x = q
  }
  PBC_DEV W sub_q(W x) const {
    const int j = lane();
    W r = x - qq + (j < leff - 1 ? (1u << WB) : 0u) - (j > 0 && j < leff ? 1u : 0u);
    return strict_limbs(r, mk);
  }
  static PBC_DEV bool is_zero(W x) { return __ballot(x != 0) == 0; }
  static PBC_DEV void sync() { __syncthreads(); }
  static PBC_DEV bool lane0() { return threadIdx.x == 0; }
  // N canonical / Montgomery words in memory (the same for every lane: a table entry, a constant) -> this lane's limb
  // (AL::to_el_uniform lane by lane: limb j = bits 29 j .. 29 j + 28)
  static PBC_DEV W load_uniform(const uint32_t *w) {
    const int j = lane(), bit = WB * (j < L ? j : 0), i = bit >> 5, sh = bit & 31;
    const uint64_t pair = ((uint64_t) (i + 1 < N ? w[i + 1] : 0u) << 32) | w[i];
    return j < L ? (uint32_t) (pair >> sh) & MASK : 0u;
  }
  // every lane's limb -> LDS slot; lane 0 (after sync) reads the whole element
  static PBC_DEV void put_slot(W x, int slot) { g_lds_aw[slot * 64 + lane()] = x; }
  static PBC_DEV void slot_to_el(el &r, int slot) {
#pragma unroll
    for (int i = 0; i < L; i++) r.l[i] = g_lds_aw[slot * 64 + i];
  }
  static PBC_DEV void el_to_slot(const el &x, int slot) {
#pragma unroll
    for (int i = 0; i < L; i++) g_lds_aw[slot * 64 + i] = x.l[i];
#pragma unroll
    for (int i = L; i < 64; i++) g_lds_aw[slot * 64 + i] = 0;
  }
  static PBC_DEV W get_slot(int slot) { return g_lds_aw[slot * 64 + lane()]; }
#endif

  // value < 2q, any limbs the product accepts -> the canonical residue, strict limbs (what to_fp + to_el give AL)
  PBC_DEV W canon(const W &x, const W &oneR) {
    W t = mul(x, oneR);
    if (geq_q(t)) t = sub_q(t);
    return t;
  }
  // 1/x by the lane-local divsteps routine (fp_inv, fp.cuh: 58 product-equivalents of ONE lane = 0.14 ms at one wave
  // per SIMD; a Fermat ladder x^(q-2) on the wave's products -- 654 of them -- took 0.32 ms), through LDS: AL's own
  // sequence to_words, fp_inv, to_el.  x: a product's output (strict limbs, value below 2q).  Every lane runs the same
  // inversion: with the call under a lane-0-only EXEC mask the kernel faulted (profiles/r04_notes.md).
  PBC_DEV W invert_lane0(const W &x) {
#ifdef PBC_HOSTSIM
    fp<N> tw;
    el r;
    A::to_words(tw, x);
    fp_inv<N>(tw, tw);
    A::to_el(r, tw);
    return r;
#else
    put_slot(x, 5);
    sync();
#if PBC_AW_INV_LANE0
    if (lane0()) {                                             // experiment switch (tools/gpu_faults.md): the call under a lane-0-only EXEC mask
      el e;
      fp<N> tw;
      slot_to_el(e, 5);
      A::to_words(tw, e);
      fp_inv<N>(tw, tw);
      A::to_el(e, tw);
      el_to_slot(e, 5);
    }
#else
    {                                                          // every lane runs the same inversion (no call under a partial EXEC mask)
      el e;
      fp<N> tw;
      slot_to_el(e, 5);
      A::to_words(tw, e);
      fp_inv<N>(tw, tw);
      A::to_el(e, tw);
      sync();
      if (lane0()) el_to_slot(e, 5);
    }
#endif
    sync();
    const W r = get_slot(5);
    sync();
    return r;
#endif
  }

  struct state {
    W fx, fy, X, Y, Z, ZZ, Qx, Qy;
  };
  PBC_DEV void fmul(state &s, const W &lx, const W &ly) {    // AL::fmul: two lazy sums of two products
    const W nfy = norm(negk(s.fy, K2));
    sop2x2(s.fx, s.fy, s.fx, lx, nfy, ly, s.fx, ly, s.fy, lx);
  }
  // The Jacobian doubling step (pairing_a.cuh a_double_step in limb form), its 19 products in four rounds of up to four independent ones and the two two-term sums of f l
  PBC_DEV void double_step(state &s) {
    W XX, Z4, YY, t0, t1, lx, ly, Z3, S1, MM, Y4, nfx, nfy, ZZn, u;
    {
      const W e0 = add(s.fx, s.fy);
      const W e1 = norm(subk(s.fx, s.fy, K2));
      mul4(nfx, nfy, XX, Z4, e0, e1, shl<1>(s.fx), s.fy, s.X, s.X, s.ZZ, s.ZZ, 4);     // f^2 (AL::fsqr), X^2, Z^4
    }
    s.fx = nfx;
    s.fy = nfy;
    W M = add(add(shl<1>(XX), XX), Z4);
    M = norm(M);
    mul4(YY, t0, Z3, MM, s.Y, s.Y, s.Qx, s.ZZ, shl<1>(s.Y), s.Z, M, M, 4);
    t0 = add(t0, s.X);
    mul4(lx, t1, S1, ZZn, M, t0, Z3, s.ZZ, YY, shl<1>(s.X), Z3, Z3, 4);
    u = shl<1>(YY);
    lx = norm(subk(lx, u, K4));
    s.Z = Z3;
    s.ZZ = ZZn;
    u = shl<2>(S1);
    s.X = norm(subk(MM, u, K8));
    u = shl<1>(S1);
    const W Wd = norm(subk(u, s.X, K12));
    mul4(ly, Y4, t0, u, t1, s.Qy, YY, YY, M, Wd, M, Wd, 3);
    fmul(s, lx, ly);
    t1 = norm(shl<3>(Y4));
    s.Y = norm(subk(t0, t1, K12));
  }
  PBC_DEV void add_step(state &s, const W &x2, const W &y2) {   // the Jacobian mixed addition step (a_add_step in limb form)
    if constexpr (kDigits) {
      // (an order with hundreds of non-zero digits: the same products -- the same operand classes, the same borrowed constants --
      // in five rounds of up to four independent ones instead of one after the other)
      W a, b, c, Z3, HH, lx, HHH, XHH, RR, t0, ly, ZZn, YH, unused;
      mul2(a, b, x2, s.ZZ, s.Z, s.ZZ);
      const W H = norm(subk(a, s.X, K16));
      mul4(c, Z3, HH, unused, y2, b, H, s.Z, H, H, H, H, 3);
      const W R = norm(subk(c, s.Y, K16));
      mul4(lx, HHH, XHH, RR, R, add(s.Qx, x2), HH, H, s.X, HH, R, R, 4);
      mul4(t0, ly, ZZn, YH, Z3, y2, Z3, s.Qy, Z3, Z3, s.Y, HHH, 4);
      lx = norm(subk(lx, t0, K2));
      W t1 = norm(subk(RR, HHH, K2));
      t1 = norm(subk(t1, shl<1>(XHH), K4));
      const W d = norm(subk(XHH, t1, K16));
      const W e = mul(R, d);
      s.Y = norm(subk(e, YH, K2));
      s.X = t1;
      s.Z = Z3;
      s.ZZ = ZZn;
      fmul(s, lx, ly);
      return;
    }
    W t0 = mul(x2, s.ZZ);
    const W H = norm(subk(t0, s.X, K16));
    t0 = mul(s.Z, s.ZZ);
    t0 = mul(y2, t0);
    const W R = norm(subk(t0, s.Y, K16));
    W Z3 = mul(H, s.Z);
    t0 = add(s.Qx, x2);
    W lx = mul(R, t0);
    t0 = mul(Z3, y2);
    lx = norm(subk(lx, t0, K2));
    const W ly = mul(Z3, s.Qy);
    W HH = sqr(H);
    W HHH = mul(HH, H);
    t0 = mul(s.X, HH);
    W t1 = sqr(R);
    t1 = norm(subk(t1, HHH, K2));
    HH = shl<1>(t0);
    t1 = norm(subk(t1, HH, K4));
    t0 = norm(subk(t0, t1, K16));
    t0 = mul(R, t0);
    HHH = mul(s.Y, HHH);
    s.Y = norm(subk(t0, HHH, K2));
    s.X = t1;
    s.Z = Z3;
    s.ZZ = sqr(Z3);
    fmul(s, lx, ly);
  }

  // The Miller loop: a.param's Solinas order (a_pairing_proj, ecc/a_param.c:1101-1210: exp2 doublings, one addition after bit
  // exp1), or -- type a1 and type a parameters of other shapes -- the signed digits of the order (pairing_a.cuh a1_miller_lane:
  // a1_pairing_proj, a_param.c:1840-2015, with the digits of hostbn.h naf_of_half)
  // NW = 8: the same products, operand classes and borrowed constants as double_step / add_step in THREE rounds a doubling step --
  // the point's chain is three products deep (X^2 -> M^2 -> M Wd), and the accumulator's two (f <- f l of step i - 1, then f^2) fit
  // beside it once the line of a step is multiplied in at the start of the next:
  //     1  X^2, Z^4, Y^2, 2Y Z, Qx ZZ  |  f l_(i-1) (two sums)        2  M^2, Y^2 2X, Y^4, M (Qx ZZ + X), Z3 ZZ, Z3^2  |  f^2 (two)
  //     3  M Wd, (Z3 ZZ) Qy                                          -> l_i waits for round 1 of the next step (or of the addition)
  // an addition in five: the waiting line beside its first two products, its own line beside its last one.
  PBC_DEV void miller_loop_p(state &s, const W &Px, const W &Py) {
    const W nPy = norm(negk(Py, K2));
    W plx = s.fx, ply = s.fx;                                  // the line that waits (values: none yet)
    bool pending = false;
    W r[8];
    for (int i = c_a.rbits - 2; i >= 0; i--) {
      W XX, Z4, YY, Z3, t0;
      {
        const W nfy = norm(negk(s.fy, K2));
        const W a0[8] = {s.X, s.ZZ, s.Y, shl<1>(s.Y), s.Qx, s.fx, s.fx, s.fx}, b0[8] = {s.X, s.ZZ, s.Y, s.Z, s.ZZ, plx, ply, ply};
        const W a1[8] = {s.X, s.X, s.X, s.X, s.X, nfy, s.fy, s.X}, b1[8] = {s.X, s.X, s.X, s.X, s.X, ply, plx, s.X};
        round8(r, a0, b0, a1, b1, pending ? 7 : 5, 0x60u);
        XX = r[0]; Z4 = r[1]; YY = r[2]; Z3 = r[3]; t0 = r[4];
        if (pending) { s.fx = r[5]; s.fy = r[6]; }
      }
      const W M = norm(add(add(shl<1>(XX), XX), Z4));
      t0 = add(t0, s.X);
      W MM, S1, Y4, lx, t1, ZZn;
      {
        const W e0 = add(s.fx, s.fy);
        const W e1 = norm(subk(s.fx, s.fy, K2));
        const W a0[8] = {M, YY, YY, M, Z3, Z3, e0, shl<1>(s.fx)}, b0[8] = {M, shl<1>(s.X), YY, t0, s.ZZ, Z3, e1, s.fy};
        round8(r, a0, b0, a0, b0, 8, 0u);
        MM = r[0]; S1 = r[1]; Y4 = r[2]; lx = r[3]; t1 = r[4]; ZZn = r[5]; s.fx = r[6]; s.fy = r[7];
      }
      lx = norm(subk(lx, shl<1>(YY), K4));
      const W X3 = norm(subk(MM, shl<2>(S1), K8));
      const W Wd = norm(subk(shl<1>(S1), X3, K12));
      {
        const W a0[8] = {M, t1, M, M, M, M, M, M}, b0[8] = {Wd, s.Qy, M, M, M, M, M, M};
        round8(r, a0, b0, a0, b0, 2, 0u);
      }
      const W Y48 = norm(shl<3>(Y4));
      s.Y = norm(subk(r[0], Y48, K12));
      s.X = X3; s.Z = Z3; s.ZZ = ZZn;
      plx = lx; ply = r[1]; pending = true;
      const int dig = i > 0 ? a1_digit(i) : 0;
      if (dig) {                                               // the Jacobian addition step; its first round takes the waiting line along
        const W x2 = Px, y2 = dig < 0 ? nPy : Py;
        W a, b;
        {
          const W nfy = norm(negk(s.fy, K2));
          const W a0[8] = {x2, s.Z, s.fx, s.fx, x2, x2, x2, x2}, b0[8] = {s.ZZ, s.ZZ, plx, ply, x2, x2, x2, x2};
          const W a1[8] = {x2, x2, nfy, s.fy, x2, x2, x2, x2}, b1[8] = {x2, x2, ply, plx, x2, x2, x2, x2};
          round8(r, a0, b0, a1, b1, 4, 0xcu);
          a = r[0]; b = r[1]; s.fx = r[2]; s.fy = r[3];
          pending = false;
        }
        const W H = norm(subk(a, s.X, K16));
        W c, Z3a, HH;
        {
          const W a0[8] = {y2, H, H, H, H, H, H, H}, b0[8] = {b, s.Z, H, H, H, H, H, H};
          round8(r, a0, b0, a0, b0, 3, 0u);
          c = r[0]; Z3a = r[1]; HH = r[2];
        }
        const W R = norm(subk(c, s.Y, K16));
        W alx, HHH, XHH, RR;
        {
          const W a0[8] = {R, HH, s.X, R, R, R, R, R}, b0[8] = {add(s.Qx, x2), H, HH, R, R, R, R, R};
          round8(r, a0, b0, a0, b0, 4, 0u);
          alx = r[0]; HHH = r[1]; XHH = r[2]; RR = r[3];
        }
        W at0, aly, ZZa, YH;
        {
          const W a0[8] = {Z3a, Z3a, Z3a, s.Y, R, R, R, R}, b0[8] = {y2, s.Qy, Z3a, HHH, R, R, R, R};
          round8(r, a0, b0, a0, b0, 4, 0u);
          at0 = r[0]; aly = r[1]; ZZa = r[2]; YH = r[3];
        }
        alx = norm(subk(alx, at0, K2));
        W t1a = norm(subk(RR, HHH, K2));
        t1a = norm(subk(t1a, shl<1>(XHH), K4));
        const W d = norm(subk(XHH, t1a, K16));
        {
          const W nfy = norm(negk(s.fy, K2));
          const W a0[8] = {R, s.fx, s.fx, R, R, R, R, R}, b0[8] = {d, alx, aly, R, R, R, R, R};
          const W a1[8] = {R, nfy, s.fy, R, R, R, R, R}, b1[8] = {R, aly, alx, R, R, R, R, R};
          round8(r, a0, b0, a1, b1, 3, 0x6u);
          s.Y = norm(subk(r[0], YH, K2));
          s.fx = r[1]; s.fy = r[2];
        }
        s.X = t1a; s.Z = Z3a; s.ZZ = ZZa;
      }
    }
    if (pending) fmul(s, plx, ply);
  }
  PBC_DEV void miller_loop(state &s, const W &Px, const W &Py) {
    if constexpr (kDigits && NW == 8) {
      miller_loop_p(s, Px, Py);
    } else if constexpr (kDigits) {
      W nPy = norm(negk(Py, K2));
      for (int i = c_a.rbits - 2; i >= 0; i--) {
        double_step(s);
        const int dig = i > 0 ? a1_digit(i) : 0;
        if (dig) add_step(s, Px, dig < 0 ? nPy : Py);
      }
    } else {
      for (int i = c_a.exp2 - 1; i >= 0; i--) {
        double_step(s);
        if (i == c_a.exp1) {
          W y2 = Py;
          if (c_a.sign1 < 0) y2 = norm(negk(y2, K2));
          add_step(s, Px, y2);
        }
      }
    }
  }

  // f^((q^2-1)/r): AL::final_exp with the inversion on the wave.  Leaves (v0 R-scaled, y) for the word-form tail:
  //     out.x = v0 / 2,   out.y = -y / 4
  PBC_DEV void final_exp(W &ox, W &oy, const state &s, const W &oneR) {
    W a2, b2, B, unused;
    mul4(a2, b2, B, unused, s.fx, s.fx, s.fy, s.fy, shl<1>(s.fx), s.fy, s.fx, s.fx, 3);
    const W Nn = norm(add(a2, b2));
    const W Av = norm(subk(a2, b2, K2));
    B = norm(negk(B, K2));
    B = canon(B, oneR);
    if (is_zero(B)) B = oneR;                                  // f^(q-1) = +-1: invert N * 1 instead (a_final_exp)
    W t = mul(Nn, B);
    t = invert_lane0(t);                                       // 1/(N B), canonical
    W w, g0;
    mul2(w, t, t, B, t, Nn);                                   // 1/N, 1/B
    mul2(g0, w, Av, w, t, Nn);                                 // Re f^(q-1), N/B
    const W P = norm(shl<1>(g0));
    W two = strict2(add(oneR, oneR));
    if (geq_q(two)) two = sub_q(two);
#ifdef PBC_HOSTSIM
    else A::hs_set(two, A::U_STRICT, 1.0);                     // (below q: the comparison has just said so)
#endif
    W v0 = two, v1 = P;
    for (int j = c_a.hbits - 1; j >= 0; j--) {
      const bool bit = j ? ((c_a.h[j >> 5] >> (j & 31)) & 1) : false;
      const W v = bit ? v1 : v0;
      W m, sq;
      mul2(m, sq, v0, v1, v, v);
      m = norm(subk(m, P, K4));
      sq = norm(subk(sq, two, K2));
      if (bit) {
        v1 = sq;
        v0 = m;
      } else {
        v0 = sq;
        v1 = m;
      }
    }
    mul2(t, ox, v0, P, v0, oneR);
    v1 = shl<1>(v1);
    v1 = norm(subk(v1, t, K2));
    oy = mul(v1, w);
  }
  // 2 R mod q from R + R: strict limbs of a value < 2q (the sum's limbs are below 2^30)
#ifdef PBC_HOSTSIM
  static W strict2(const W &x) { W r = x; strict_limbs(r); A::hs_set(r, A::U_STRICT, 2.0); return r; }
#else
  PBC_DEV W strict2(W x) const { return strict_limbs(x, mk); }
#endif

  // ---- pairing_pp_apply and few-term products on the wave (round 5; VERDICT r4 "missing" 1) ------------------------
  // The word-form tail of pairing_wave: (ox, oy) -> out.x = ox / 2, out.y = -oy / 4, stored by lane 0
  PBC_DEV void store_result(uint8_t *gt, const W &ox, const W &oy, bool valid) {
#ifndef PBC_HOSTSIM
    put_slot(ox, 0);
    put_slot(oy, 1);
    sync();
#endif
    if (lane0()) {
      el ex, ey;
#ifdef PBC_HOSTSIM
      ex = ox; ey = oy;
#else
      slot_to_el(ex, 0);
      slot_to_el(ey, 1);
#endif
      fp2<N> out;
      fp<N> x, y;
      A::to_words(y, ey);
      fp_halve<N>(y, y);
      fp_halve<N>(y, y);
      fp_neg<N>(out.y, y);
      A::to_words(x, ex);
      fp_halve<N>(out.x, x);
      a_store_gt<N>(gt, out, valid);
    }
  }
  // Q = (Qx, Qy) and R mod q into the wave's registers through lane 0 and the LDS slots; returns a_on_curve(Q) (lane 0's
  // answer, broadcast)
  PBC_DEV bool load_second(state &s, W &oneR, const uint8_t *g2) {
    const int NB = fq_len();
    bool ok = false;
    el e[3];
    if (lane0()) {
      fp<N> qx, qy, one;
      fp_load_be<N>(qx, g2);
      fp_load_be<N>(qy, g2 + NB);
      ok = a_on_curve<N>(qx, qy);
      fp_set<N>(one, fpk<N>().one);
      A::to_el(e[0], qx);
      A::to_el(e[1], qy);
      A::to_el(e[2], one);
#ifndef PBC_HOSTSIM
      for (int i = 0; i < 3; i++) el_to_slot(e[i], 2 + i);
#endif
    }
#ifdef PBC_HOSTSIM
    s.Qx = e[0]; s.Qy = e[1]; oneR = e[2];
#else
    sync();
    s.Qx = get_slot(2); s.Qy = get_slot(3); oneR = get_slot(4);
    sync();
#endif
    return ok;
  }
  // pairing_pp_apply (a_pairing_pp_apply, ecc/a_param.c:317-360) for one second argument on the wave: AL::pp_apply_lane's
  // operations -- per step f <- f^2, then f <- f ((cA Qx + cC) + i cB Qy) with (cA, cB, cC) from the table of the fixed
  // first argument (a_pp_init_lane: [exp2 + 1][3][N] Montgomery words, wave-uniform) -- with the two products of f^2 and
  // the two of the line in ONE round of four (they are independent: the line does not involve f).  8 products per step
  // against the 19 + 4 of a full Miller step; no point arithmetic.
  PBC_DEV void pp_apply_wave(uint8_t *gt, const uint32_t *tab, bool p_valid, const uint8_t *g2) {
    state s;
    init();
    W oneR;
    bool valid = load_second(s, oneR, g2);
    valid = valid && p_valid;                                  // (lane 0's value is the one that is used)
    s.fx = oneR;
#ifdef PBC_HOSTSIM
    { el z; for (int i = 0; i < L; i++) z.l[i] = 0; A::hs_set(z, A::U_STRICT, 1.0); s.fy = z; }
#else
    s.fy = 0;
#endif
    int slot = 0;
    if constexpr (kDigits) {
      // (a1_pp_apply_lane: one table entry per doubling and per addition, in loop order)
      for (int i = c_a.rbits - 2; i >= 0; i--) {
        W nfx, nfy, lx, ly;
        {
          const W e0 = add(s.fx, s.fy);
          const W e1 = norm(subk(s.fx, s.fy, K2));
          const W cA = load_uniform(tab + ((size_t) slot * 3 + 0) * N), cB = load_uniform(tab + ((size_t) slot * 3 + 1) * N);
          mul4(nfx, nfy, lx, ly, e0, e1, shl<1>(s.fx), s.fy, s.Qx, cA, s.Qy, cB, 4);
        }
        s.fx = nfx;
        s.fy = nfy;
        lx = norm(add(lx, load_uniform(tab + ((size_t) slot * 3 + 2) * N)));
        fmul(s, lx, ly);
        slot++;
        if (i > 0 && a1_digit(i)) {
          const W cA = load_uniform(tab + ((size_t) slot * 3 + 0) * N), cB = load_uniform(tab + ((size_t) slot * 3 + 1) * N);
          mul2(lx, ly, s.Qx, cA, s.Qy, cB);
          lx = norm(add(lx, load_uniform(tab + ((size_t) slot * 3 + 2) * N)));
          fmul(s, lx, ly);
          slot++;
        }
      }
    } else
    for (int i = c_a.exp2 - 1; i >= 0; i--, slot++) {
      W nfx, nfy, lx, ly;
      {
        const W e0 = add(s.fx, s.fy);
        const W e1 = norm(subk(s.fx, s.fy, K2));
        const W cA = load_uniform(tab + (slot * 3 + 0) * N), cB = load_uniform(tab + (slot * 3 + 1) * N);
        mul4(nfx, nfy, lx, ly, e0, e1, shl<1>(s.fx), s.fy, s.Qx, cA, s.Qy, cB, 4);     // f^2 (AL::fsqr) and the line's two products
      }
      s.fx = nfx;
      s.fy = nfy;
      lx = norm(add(lx, load_uniform(tab + (slot * 3 + 2) * N)));
      fmul(s, lx, ly);
      if (i == c_a.exp1) {                                     // the addition step's line: table entry exp2
        const W cA = load_uniform(tab + (c_a.exp2 * 3 + 0) * N), cB = load_uniform(tab + (c_a.exp2 * 3 + 1) * N);
        mul2(lx, ly, s.Qx, cA, s.Qy, cB);
        lx = norm(add(lx, load_uniform(tab + (c_a.exp2 * 3 + 2) * N)));
        fmul(s, lx, ly);
      }
    }
    W ox, oy;
    final_exp(ox, oy, s, oneR);
    store_result(gt, ox, oy, valid);
  }
  // The Miller loop of pairing_wave alone (f_(r, P)(Q) before the final exponentiation); validity as pairing_wave's
  PBC_DEV bool miller_wave(state &s, W &oneR, const uint8_t *g1, const uint8_t *g2) {
    const int NB = fq_len();
    bool valid = false;
    W Px, Py;
    {
      el e[2];
      if (lane0()) {
        fp<N> px, py;
        fp_load_be<N>(px, g1);
        fp_load_be<N>(py, g1 + NB);
        valid = a_first_arg_ok<N>(px, py);
        A::to_el(e[0], px);
        A::to_el(e[1], py);
#ifndef PBC_HOSTSIM
        for (int i = 0; i < 2; i++) el_to_slot(e[i], i);
#endif
      }
#ifdef PBC_HOSTSIM
      Px = e[0]; Py = e[1];
#else
      sync();
      Px = get_slot(0); Py = get_slot(1);
      sync();
#endif
    }
    const bool qok = load_second(s, oneR, g2);
    valid = valid && qok;
    s.X = Px; s.Y = Py; s.Z = oneR; s.ZZ = oneR; s.fx = oneR;
#ifdef PBC_HOSTSIM
    { el z; for (int i = 0; i < L; i++) z.l[i] = 0; A::hs_set(z, A::U_STRICT, 1.0); s.fy = z; }
#else
    s.fy = 0;
#endif
    miller_loop(s, Px, Py);
    return valid;
  }
  // Products of a few terms with small batches (element_prod_pairing, benchmark/multipairing.c's shape): every TERM gets a
  // wave (or four), writes its Miller value as a record of 2 L limbs + a validity word (WREC words); a second launch
  // gives every PRODUCT a wave that multiplies its k values and runs ONE final exponentiation.  The same value as
  // a_pairings_affine (ecc/a_param.c:1283-1383): the product of the Miller values is taken before the exponentiation.
  static constexpr int WREC = 2 * L + 4;                       // words per record (16-byte multiple)
#ifdef PBC_HOSTSIM
  struct wrec { W fx, fy; bool valid; };
  void miller_record_wave(wrec &r, const uint8_t *g1, const uint8_t *g2) {
    state s;
    W oneR;
    init();
    r.valid = miller_wave(s, oneR, g1, g2);
    r.fx = s.fx; r.fy = s.fy;
  }
  void prod_finish_wave(uint8_t *gt, const wrec *rec, int k) {
    state s;
    init();
    fp<N> one;
    fp_set<N>(one, fpk<N>().one);
    W oneR;
    A::to_el(oneR, one);
    bool valid = rec[0].valid;
    s.fx = rec[0].fx; s.fy = rec[0].fy;
    for (int t = 1; t < k; t++) {
      valid = valid && rec[t].valid;
      fmul(s, rec[t].fx, rec[t].fy);
    }
    W ox, oy;
    final_exp(ox, oy, s, oneR);
    store_result(gt, ox, oy, valid);
  }
#else
  PBC_DEV void miller_record_wave(uint32_t *rec, const uint8_t *g1, const uint8_t *g2) {
    state s;
    W oneR;
    init();
    const bool valid = miller_wave(s, oneR, g1, g2);
    const int j = lane();
    if (NW == 1 || wave() == 0) {                              // (four waves per term: every wave holds the whole state, wave 0 writes)
      if (j < L) { rec[j] = s.fx; rec[L + j] = s.fy; }
      if (threadIdx.x == 0) rec[2 * L] = valid ? 1u : 0u;
    }
  }
  PBC_DEV void prod_finish_wave(uint8_t *gt, const uint32_t *rec, int k) {
    state s;
    init();
    const int j = lane();
    const W oneR = load_uniform(fpk<N>().one);
    uint32_t ok = rec[2 * L];
    s.fx = j < L ? rec[j] : 0u;
    s.fy = j < L ? rec[L + j] : 0u;
    for (int t = 1; t < k; t++) {
      const uint32_t *r = rec + (size_t) t * WREC;
      ok &= r[2 * L];
      const W lx = j < L ? r[j] : 0u, ly = j < L ? r[L + j] : 0u;
      fmul(s, lx, ly);
    }
    W ox, oy;
    final_exp(ox, oy, s, oneR);
    store_result(gt, ox, oy, ok != 0);
  }
#endif

  // element_pairing, one wave: gt <- e(g1, g2)
  PBC_DEV void pairing_wave(uint8_t *gt, const uint8_t *g1, const uint8_t *g2) {
    const int NB = fq_len();
    bool valid = false;
    state s;
    init();
    W Px, Py, oneR;
    {
      el e[5];
      if (lane0()) {
        fp<N> px, py, qx, qy, one;
        fp_load_be<N>(px, g1);
        fp_load_be<N>(py, g1 + NB);
        fp_load_be<N>(qx, g2);
        fp_load_be<N>(qy, g2 + NB);
        valid = a_first_arg_ok<N>(px, py) & a_on_curve<N>(qx, qy);
        fp_set<N>(one, fpk<N>().one);
        A::to_el(e[0], px);
        A::to_el(e[1], py);
        A::to_el(e[2], qx);
        A::to_el(e[3], qy);
        A::to_el(e[4], one);
#ifndef PBC_HOSTSIM
        for (int i = 0; i < 5; i++) el_to_slot(e[i], i);
#endif
      }
#ifdef PBC_HOSTSIM
      Px = e[0]; Py = e[1]; s.Qx = e[2]; s.Qy = e[3]; oneR = e[4];
#else
      sync();
      Px = get_slot(0); Py = get_slot(1); s.Qx = get_slot(2); s.Qy = get_slot(3); oneR = get_slot(4);
      sync();
#endif
    }
    s.X = Px; s.Y = Py; s.Z = oneR; s.ZZ = oneR; s.fx = oneR;
#ifdef PBC_HOSTSIM
    { el z; for (int i = 0; i < L; i++) z.l[i] = 0; A::hs_set(z, A::U_STRICT, 1.0); s.fy = z; }
#else
    s.fy = 0;
#endif
    miller_loop(s, Px, Py);
    W ox, oy;
    final_exp(ox, oy, s, oneR);
#ifndef PBC_HOSTSIM
    put_slot(ox, 0);
    put_slot(oy, 1);
    sync();
#endif
    if (lane0()) {
      el ex, ey;
#ifdef PBC_HOSTSIM
      ex = ox; ey = oy;
#else
      slot_to_el(ex, 0);
      slot_to_el(ey, 1);
#endif
      fp2<N> out;
      fp<N> x, y;
      A::to_words(y, ey);
      fp_halve<N>(y, y);
      fp_halve<N>(y, y);
      fp_neg<N>(out.y, y);
      A::to_words(x, ex);
      fp_halve<N>(out.x, x);
      a_store_gt<N>(gt, out, valid);
    }
  }
};

}  // namespace pbc
