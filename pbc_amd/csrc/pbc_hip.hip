// pbc_hip.hip -- kernels + C-ABI of libpbc_hip.so (see include/pbc_hip.h).
//
// gfx950 only.  Host side: parameter parsing and constant derivation (hostbn.h), device
// buffer management, launches.  Device side: one pairing per lane (pairing_a.cuh).
#include "host_common.h"
#include "host_text.h"

extern "C" const char *pbc_hip_last_error(void) { return g_err; }

// Batched F_q operations on wire bytes (differential check of the limb arithmetic).
template <int N>
__global__ void __launch_bounds__(kBlock) fq_op_kernel(int op, uint8_t *c, const uint8_t *a,
                                                        const uint8_t *b, size_t n, KArgs<N> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const int L = (int) fpk<N>().fbytes;
  fp<N> x, y, z;
  fp_load_be<N>(x, a + idx * L);
  if (b) fp_load_be<N>(y, b + idx * L); else y = x;
  switch (op) {
    case 0: fp_mul<N>(z, x, y); break;
    case 1: fp_add<N>(z, x, y); break;
    case 2: fp_sub<N>(z, x, y); break;
    case 3: fp_inv<N>(z, x); break;
    case 4: fp_neg<N>(z, x); break;
    case 5: fp_halve<N>(z, x); break;
    default: fp_dbl<N>(z, x); break;
  }
  fp_store_be<N>(c + idx * L, z);
}

// ---- register-only instruction-throughput probes (the measured integer roofline) --------
#define REP8(x) x x x x x x x x
template <int V>
__global__ void __launch_bounds__(256) probe_kernel(uint32_t *sink, int iters, uint32_t seed) {
  uint32_t t = threadIdx.x + seed;
  uint64_t a0 = t, a1 = t + 1, a2 = t + 2, a3 = t + 3, a4 = t + 4, a5 = t + 5, a6 = t + 6, a7 = t + 7;
  uint32_t x = t * 2654435761u + 12345u, y = t ^ 0x9e3779b9u, c0 = 0, c1 = 0;
  double d0 = t, d1 = t + 1.5, d2 = t + 2.5, d3 = t + 3.5, dx = 1.0000001, dy = 0.9999999;
  for (int i = 0; i < iters; i++) {
    if constexpr (V == 0) {            // 8 independent v_mad_u64_u32 chains
      REP8(asm volatile("v_mad_u64_u32 %0, vcc, %8, %9, %0\n\tv_mad_u64_u32 %1, vcc, %8, %9, %1\n\t"
                        "v_mad_u64_u32 %2, vcc, %8, %9, %2\n\tv_mad_u64_u32 %3, vcc, %8, %9, %3\n\t"
                        "v_mad_u64_u32 %4, vcc, %8, %9, %4\n\tv_mad_u64_u32 %5, vcc, %8, %9, %5\n\t"
                        "v_mad_u64_u32 %6, vcc, %8, %9, %6\n\tv_mad_u64_u32 %7, vcc, %8, %9, %7"
                        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                        : "v"(x), "v"(y) : "vcc");)
    } else if constexpr (V == 1) {     // the engine's MAC: mad + addc, one dependent chain
      REP8(asm volatile("v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc"
                        : "+v"(a0), "+v"(c0), "+v"(c1) : "v"(x), "v"(y) : "vcc");)
    } else if constexpr (V == 2) {     // v_mul_lo_u32
      REP8(asm volatile("v_mul_lo_u32 %0, %0, %8\n\tv_mul_lo_u32 %1, %1, %8\n\tv_mul_lo_u32 %2, %2, %8\n\t"
                        "v_mul_lo_u32 %3, %3, %8\n\tv_mul_lo_u32 %4, %4, %8\n\tv_mul_lo_u32 %5, %5, %8\n\t"
                        "v_mul_lo_u32 %6, %6, %8\n\tv_mul_lo_u32 %7, %7, %8"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x));)
    } else if constexpr (V == 3) {     // v_mul_hi_u32
      REP8(asm volatile("v_mul_hi_u32 %0, %0, %8\n\tv_mul_hi_u32 %1, %1, %8\n\tv_mul_hi_u32 %2, %2, %8\n\t"
                        "v_mul_hi_u32 %3, %3, %8\n\tv_mul_hi_u32 %4, %4, %8\n\tv_mul_hi_u32 %5, %5, %8\n\t"
                        "v_mul_hi_u32 %6, %6, %8\n\tv_mul_hi_u32 %7, %7, %8"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x));)
    } else if constexpr (V == 4) {     // v_dot2_u32_u16
      REP8(asm volatile("v_dot2_u32_u16 %0, %8, %9, %0\n\tv_dot2_u32_u16 %1, %8, %9, %1\n\t"
                        "v_dot2_u32_u16 %2, %8, %9, %2\n\tv_dot2_u32_u16 %3, %8, %9, %3\n\t"
                        "v_dot2_u32_u16 %4, %8, %9, %4\n\tv_dot2_u32_u16 %5, %8, %9, %5\n\t"
                        "v_dot2_u32_u16 %6, %8, %9, %6\n\tv_dot2_u32_u16 %7, %8, %9, %7"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x), "v"(y));)
    } else if constexpr (V == 5) {     // v_fma_f64, 4 chains x 2
      REP8(asm volatile("v_fma_f64 %0, %4, %5, %0\n\tv_fma_f64 %1, %4, %5, %1\n\tv_fma_f64 %2, %4, %5, %2\n\t"
                        "v_fma_f64 %3, %4, %5, %3\n\tv_fma_f64 %0, %4, %5, %0\n\tv_fma_f64 %1, %4, %5, %1\n\t"
                        "v_fma_f64 %2, %4, %5, %2\n\tv_fma_f64 %3, %4, %5, %3"
                        : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(dx), "v"(dy));)
    } else if constexpr (V == 6) {     // v_addc_co_u32 chain
      REP8(asm volatile("v_add_co_u32 %0, vcc, %0, %8\n\tv_addc_co_u32 %1, vcc, %1, %8, vcc\n\t"
                        "v_addc_co_u32 %2, vcc, %2, %8, vcc\n\tv_addc_co_u32 %3, vcc, %3, %8, vcc\n\t"
                        "v_addc_co_u32 %4, vcc, %4, %8, vcc\n\tv_addc_co_u32 %5, vcc, %5, %8, vcc\n\t"
                        "v_addc_co_u32 %6, vcc, %6, %8, vcc\n\tv_addc_co_u32 %7, vcc, %7, %8, vcc"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x) : "vcc");)
    } else if constexpr (V == 7) {     // v_mad_u32_u24
      REP8(asm volatile("v_mad_u32_u24 %0, %8, %9, %0\n\tv_mad_u32_u24 %1, %8, %9, %1\n\t"
                        "v_mad_u32_u24 %2, %8, %9, %2\n\tv_mad_u32_u24 %3, %8, %9, %3\n\t"
                        "v_mad_u32_u24 %4, %8, %9, %4\n\tv_mad_u32_u24 %5, %8, %9, %5\n\t"
                        "v_mad_u32_u24 %6, %8, %9, %6\n\tv_mad_u32_u24 %7, %8, %9, %7"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x), "v"(y));)
    } else if constexpr (V == 8) {     // v_lshl_add_u64 (64-bit add)
      REP8(asm volatile("v_lshl_add_u64 %0, %0, 0, %8\n\tv_lshl_add_u64 %1, %1, 0, %8\n\t"
                        "v_lshl_add_u64 %2, %2, 0, %8\n\tv_lshl_add_u64 %3, %3, 0, %8\n\t"
                        "v_lshl_add_u64 %4, %4, 0, %8\n\tv_lshl_add_u64 %5, %5, 0, %8\n\t"
                        "v_lshl_add_u64 %6, %6, 0, %8\n\tv_lshl_add_u64 %7, %7, 0, %8"
                        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                        : "v"(a0 ^ 0x12345));)
    } else if constexpr (V == 9) {     // v_dot4_u32_u8
      REP8(asm volatile("v_dot4_u32_u8 %0, %8, %9, %0\n\tv_dot4_u32_u8 %1, %8, %9, %1\n\t"
                        "v_dot4_u32_u8 %2, %8, %9, %2\n\tv_dot4_u32_u8 %3, %8, %9, %3\n\t"
                        "v_dot4_u32_u8 %4, %8, %9, %4\n\tv_dot4_u32_u8 %5, %8, %9, %5\n\t"
                        "v_dot4_u32_u8 %6, %8, %9, %6\n\tv_dot4_u32_u8 %7, %8, %9, %7"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x), "v"(y));)
    } else if constexpr (V == 10) {    // mad + addc with an s_nop 0 after each pair (compiler's asm pad)
      REP8(asm volatile("v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0\n\t"
                        "v_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc\n\ts_nop 0"
                        : "+v"(a0), "+v"(c0), "+v"(c1) : "v"(x), "v"(y) : "vcc");)
    } else if constexpr (V == 11) {    // v_mad_u32_u16
      REP8(asm volatile("v_mad_u32_u16 %0, %8, %9, %0\n\tv_mad_u32_u16 %1, %8, %9, %1\n\t"
                        "v_mad_u32_u16 %2, %8, %9, %2\n\tv_mad_u32_u16 %3, %8, %9, %3\n\t"
                        "v_mad_u32_u16 %4, %8, %9, %4\n\tv_mad_u32_u16 %5, %8, %9, %5\n\t"
                        "v_mad_u32_u16 %6, %8, %9, %6\n\tv_mad_u32_u16 %7, %8, %9, %7"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x), "v"(y));)
    } else if constexpr (V == 12) {    // v_add_u32 (full-rate reference)
      REP8(asm volatile("v_add_u32 %0, %0, %8\n\tv_add_u32 %1, %1, %8\n\tv_add_u32 %2, %2, %8\n\t"
                        "v_add_u32 %3, %3, %8\n\tv_add_u32 %4, %4, %8\n\tv_add_u32 %5, %5, %8\n\t"
                        "v_add_u32 %6, %6, %8\n\tv_add_u32 %7, %7, %8"
                        : "+v"(*(uint32_t *) &a0), "+v"(*(uint32_t *) &a1), "+v"(*(uint32_t *) &a2),
                          "+v"(*(uint32_t *) &a3), "+v"(*(uint32_t *) &a4), "+v"(*(uint32_t *) &a5),
                          "+v"(*(uint32_t *) &a6), "+v"(*(uint32_t *) &a7) : "v"(x));)
    } else if constexpr (V == 13) {    // v_mad_u64_u32 with an SGPR factor (modulus limb form)
      REP8(asm volatile("v_mad_u64_u32 %0, vcc, %8, %9, %0\n\tv_mad_u64_u32 %1, vcc, %8, %9, %1\n\t"
                        "v_mad_u64_u32 %2, vcc, %8, %9, %2\n\tv_mad_u64_u32 %3, vcc, %8, %9, %3\n\t"
                        "v_mad_u64_u32 %4, vcc, %8, %9, %4\n\tv_mad_u64_u32 %5, vcc, %8, %9, %5\n\t"
                        "v_mad_u64_u32 %6, vcc, %8, %9, %6\n\tv_mad_u64_u32 %7, vcc, %8, %9, %7"
                        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                        : "v"(x), "s"(seed) : "vcc");)
    } else if constexpr (V == 14) {    // same, the carry-outs spread over four SGPR pairs (is the vcc write the limiter?)
      REP8(asm volatile("v_mad_u64_u32 %0, vcc, %8, %9, %0\n\tv_mad_u64_u32 %1, s[36:37], %8, %9, %1\n\t"
                        "v_mad_u64_u32 %2, s[38:39], %8, %9, %2\n\tv_mad_u64_u32 %3, s[40:41], %8, %9, %3\n\t"
                        "v_mad_u64_u32 %4, vcc, %8, %9, %4\n\tv_mad_u64_u32 %5, s[36:37], %8, %9, %5\n\t"
                        "v_mad_u64_u32 %6, s[38:39], %8, %9, %6\n\tv_mad_u64_u32 %7, s[40:41], %8, %9, %7"
                        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                        : "v"(x), "s"(seed) : "vcc", "s36", "s37", "s38", "s39", "s40", "s41");)
    } else if constexpr (V == 15) {    // the signed form, v_mad_i64_i32 (what a signed-limb representation would issue)
      REP8(asm volatile("v_mad_i64_i32 %0, vcc, %8, %9, %0\n\tv_mad_i64_i32 %1, vcc, %8, %9, %1\n\t"
                        "v_mad_i64_i32 %2, vcc, %8, %9, %2\n\tv_mad_i64_i32 %3, vcc, %8, %9, %3\n\t"
                        "v_mad_i64_i32 %4, vcc, %8, %9, %4\n\tv_mad_i64_i32 %5, vcc, %8, %9, %5\n\t"
                        "v_mad_i64_i32 %6, vcc, %8, %9, %6\n\tv_mad_i64_i32 %7, vcc, %8, %9, %7"
                        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                        : "v"(x), "s"(seed) : "vcc");)
    } else if constexpr (V == 16 || V == 17 || V == 18) {
      // VGPR bank placement of the all-VGPR multiply-add (4 banks, bank = register number mod 4; the 64-bit accumulator
      // takes two).  16: factors in the two banks the accumulator leaves free; 17: both factors in the accumulator's
      // banks; 18: both factors in ONE free bank.  Explicit registers, eight chains.
#define PBC_PROBE_MAD8(X_, Y_)                                                                                  \
      "v_mad_u64_u32 v[100:101], vcc, " X_ ", " Y_ ", v[100:101]\n\tv_mad_u64_u32 v[104:105], vcc, " X_ ", " Y_ ", v[104:105]\n\t" \
      "v_mad_u64_u32 v[108:109], vcc, " X_ ", " Y_ ", v[108:109]\n\tv_mad_u64_u32 v[112:113], vcc, " X_ ", " Y_ ", v[112:113]\n\t" \
      "v_mad_u64_u32 v[116:117], vcc, " X_ ", " Y_ ", v[116:117]\n\tv_mad_u64_u32 v[120:121], vcc, " X_ ", " Y_ ", v[120:121]\n\t" \
      "v_mad_u64_u32 v[124:125], vcc, " X_ ", " Y_ ", v[124:125]\n\tv_mad_u64_u32 v[128:129], vcc, " X_ ", " Y_ ", v[128:129]\n\t"
#define PBC_PROBE_CLOB "vcc", "v100", "v101", "v104", "v105", "v108", "v109", "v112", "v113", "v116", "v117", "v120", "v121", \
                       "v124", "v125", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135"
      if (i == 0) asm volatile("v_mov_b32 v130, %0\n\tv_mov_b32 v131, %1\n\tv_mov_b32 v132, %0\n\tv_mov_b32 v133, %1\n\t"
                               "v_mov_b32 v134, %0\n\tv_mov_b32 v135, %1\n\t"
                               "v_mov_b32 v100, %0\n\tv_mov_b32 v101, 0\n\tv_mov_b32 v104, %1\n\tv_mov_b32 v105, 0\n\t"
                               "v_mov_b32 v108, %0\n\tv_mov_b32 v109, 0\n\tv_mov_b32 v112, %1\n\tv_mov_b32 v113, 0\n\t"
                               "v_mov_b32 v116, %0\n\tv_mov_b32 v117, 0\n\tv_mov_b32 v120, %1\n\tv_mov_b32 v121, 0\n\t"
                               "v_mov_b32 v124, %0\n\tv_mov_b32 v125, 0\n\tv_mov_b32 v128, %1\n\tv_mov_b32 v129, 0"
                               : : "v"(x), "v"(y) : PBC_PROBE_CLOB);
      // accumulators sit in banks 0, 1 (v100 = 4 * 25); v130 / v134: bank 2, v131 / v135: bank 3, v132: bank 0, v133: bank 1
      if constexpr (V == 16) { REP8(asm volatile(PBC_PROBE_MAD8("v130", "v131") "" : : : PBC_PROBE_CLOB);) }
      else if constexpr (V == 17) { REP8(asm volatile(PBC_PROBE_MAD8("v132", "v133") "" : : : PBC_PROBE_CLOB);) }
      else { REP8(asm volatile(PBC_PROBE_MAD8("v130", "v134") "" : : : PBC_PROBE_CLOB);) }
      if (i == iters - 1) asm volatile("v_xor_b32 %0, v100, v104\n\tv_xor_b32 %0, %0, v108\n\tv_xor_b32 %0, %0, v129" : "=v"(c0) : : PBC_PROBE_CLOB);
#undef PBC_PROBE_MAD8
#undef PBC_PROBE_CLOB
    }
  }
  uint64_t r = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7 ^ c0 ^ c1;
  r ^= (uint64_t) (d0 + d1 + d2 + d3);
  if (r == 0x1234567887654321ull) sink[0] = (uint32_t) r;   // never true in practice: keeps the chains live
}

// limb-form out-of-line product / square (experiment: elements kept as 18 x 29-bit limbs between calls)
typedef uint32_t v18 __attribute__((ext_vector_type(18)));
static __device__ __noinline__ v18 fz_mul_fn(v18 va, v18 vb) {
  fl<16> a[1], b[1], r;
#pragma unroll
  for (int i = 0; i < 18; i++) { a[0].l[i] = va[i]; b[0].l[i] = vb[i]; }
  sop_limbs<16, 1>(r, a, b);
  v18 o;
#pragma unroll
  for (int i = 0; i < 18; i++) o[i] = r.l[i];
  return o;
}
static __device__ __noinline__ v18 fz_sqr_fn(v18 va) {
  uint32_t x[18], t[18];
#pragma unroll
  for (int i = 0; i < 18; i++) x[i] = va[i];
  sqr_limbs<16>(t, x);
  v18 o;
#pragma unroll
  for (int i = 0; i < 18; i++) o[i] = t[i];
  return o;
}
// ---- multiplier micro-benchmark: iters dependent F_q products per lane, nothing else ------
template <int N, int V>
__global__ void __launch_bounds__(256) mul_bench_kernel(uint32_t *out, const uint32_t *in, int iters, KArgs<N> ka) {
  int tid = blockIdx.x * 256 + threadIdx.x;
  int n = gridDim.x * 256;
  fp<N> x, y;
#pragma unroll
  for (int i = 0; i < N; i++) { x.v[i] = in[i * n + tid]; y.v[i] = in[(N + i) * n + tid] | 1; }
#pragma nounroll
  for (int it = 0; it < iters; it++) {
    if constexpr (V == 1) fp_mul29_inl<N, false>(x, x, y);
    else if constexpr (V == 2) fp_mul29_inl<N, true>(x, x, y);
    else if constexpr (V == 3) fp_sqr29_inl<N, false>(x, x);
    else if constexpr (V == 4) fp_sqr29_inl<N, true>(x, x);
    else if constexpr (V == 5) { fp_inv<N>(x, x); fp_add<N>(x, x, y); }          // safegcd inversion
    else if constexpr (V == 6) fp_mul<N>(x, x, y);                                 // out-of-line product
    else if constexpr (V == 7) fp_sqr<N>(x, x);                                    // out-of-line square
    else if constexpr (N == 16 && (V == 8 || V == 9 || V == 10)) {
      // limb-form chain: x, y reinterpreted as 18 limbs (values are garbage but the work is the same)
      v18 a, b;
#pragma unroll
      for (int i = 0; i < 18; i++) { a[i] = x.v[i & 15] & 0x1fffffffu; b[i] = y.v[i & 15] & 0x1fffffffu; }
      for (int rep = 0; rep < 8; rep++) {
        if constexpr (V == 8) a = fz_mul_fn(a, b);
        else if constexpr (V == 9) a = fz_sqr_fn(a);
        else {                                               // product + lazy subtraction + parallel carry
          v18 c = fz_mul_fn(a, b);
          uint32_t cy[18];
#pragma unroll
          for (int i = 0; i < 18; i++) { uint32_t t = c[i] + 0x3ffffff8u - b[i]; cy[i] = t >> 29; c[i] = t & 0x1fffffffu; }
#pragma unroll
          for (int i = 1; i < 18; i++) c[i] += cy[i - 1];
          a = c;
        }
      }
#pragma unroll
      for (int i = 0; i < 16; i++) x.v[i] = a[i];
      it += 7;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) out[i * n + tid] = x.v[i];
}

extern "C" int pbc_hip_pairing_init_set_buf(pbc_hip_pairing_t **out, const char *param, size_t len) {
  if (!out || !param) return fail("null argument");
  if (!len) len = strlen(param);
  std::string type;
  if (!pbc_host::param_lookup(param, len, "type", type)) return fail("unknown pairing type (no 'type' key)");
  pbc_hip_pairing_s *P = new pbc_hip_pairing_s();
  int rc;
  if (type == "a") {
    P->type = 'a';
    rc = init_type_a(P, param, len);
  } else if (type == "a1") {
    P->type = '1';
    rc = init_type_a1(P, param, len);
  } else if (type == "e") {
    P->type = 'e';
    rc = init_type_e(P, param, len);
  } else if (type == "d") {
    P->type = 'd';
    rc = init_type_d(P, param, len, 3);
  } else if (type == "g") {
    P->type = 'g';
    rc = init_type_d(P, param, len, 5);
  } else if (type == "f") {
    P->type = 'f';
    rc = init_type_f(P, param, len);
  } else {
    rc = fail("pairing type '%s' is not built into libpbc_hip yet", type.c_str());
  }
  if (!rc) {
    P->param_text.assign(param, len);
    int hc = 0;                        // "hip_host_chunk N": units per chunk of the host-buffer entry points (measurements)
    pbc_host::param_int(param, len, "hip_host_chunk", hc);
    P->host_chunk = hc > 0 ? (size_t) hc : 0;
    int zc = PBC_HIP_ZERO_COPY_DEFAULT;   // "hip_zero_copy 0/1": kernels of the host-buffer entry points read / write pinned caller buffers in place
    pbc_host::param_int(param, len, "hip_zero_copy", zc);
    P->zero_copy = zc != 0;
    int rs = 0;                        // "hip_resident_slots N": workgroups of a resident launch (tests: forces several units per lane on small batches)
    pbc_host::param_int(param, len, "hip_resident_slots", rs);
    P->resident_slots = rs > 0 ? rs : 0;
    int dy = 0, nf = 0;                // "hip_dynamic 1": resident launches fetch units from a counter; "hip_no_fair 1": no time-sliced priorities
    pbc_host::param_int(param, len, "hip_dynamic", dy);
    pbc_host::param_int(param, len, "hip_no_fair", nf);
    P->dynamic = dy != 0;
    P->no_fair = nf != 0;
    int gs = 0;                        // "hip_group_slow 1": element_mul_zn / GT pow_zn on the complete bit-by-bit ladders only
    pbc_host::param_int(param, len, "hip_group_slow", gs);
    P->group_slow = gs != 0;
    int rf = pbc_host::kRaggedFoldDefault;   // "hip_ragged_fold N": records per fold lane of the ragged products (every value: the same bytes)
    pbc_host::param_int(param, len, "hip_ragged_fold", rf);
    if (rf < 2 || rf > 64) rc = fail("hip_ragged_fold must be 2..64 (got %d)", rf);
    P->ragged_fold = rf;
    int mc = 0;                        // "hip_multi_compose 1": type a pow2 / pow3 as single-base ladders + additions (A/B with the joint ladder)
    pbc_host::param_int(param, len, "hip_multi_compose", mc);
    P->a_multi_compose = mc != 0;
    // bind to the caller's current device; without one the object still parses/validates
    // parameters (host logic), and every batch call fails loudly -- there is no CPU path.
    if (hipGetDevice(&P->device) != hipSuccess) P->device = -1;
  }
  if (rc) {
    delete P;
    return 1;
  }
  *out = P;
  return 0;
}
static void hostctx_free(pbc_hip_pairing_s *P);
extern "C" void pbc_hip_pairing_clear(pbc_hip_pairing_t *p) {
  if (!p) return;
  hostctx_free(p);
  delete p;
}
extern "C" int pbc_hip_pairing_type(const pbc_hip_pairing_t *p) { return p->type; }
extern "C" int pbc_hip_device_count(void) {
  int count = 0;
  return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}
extern "C" int pbc_hip_pairing_use_devices(pbc_hip_pairing_t *P, const int *devices, int n) {
  if (!P) return fail("null pairing");
  if (n < 0 || n > 16 || (n > 0 && !devices)) return fail("use_devices: 0..16 devices");
  int count = 0;
  if (n > 0 && hipGetDeviceCount(&count) != hipSuccess) return fail("no HIP device: libpbc_hip has no CPU fallback");
  for (int i = 0; i < n; i++)
    if (devices[i] < 0 || devices[i] >= count) return fail("use_devices: device %d is not visible (%d devices)", devices[i], count);
  for (int i = 0; i < n; i++) P->devs[i] = devices[i];
  P->ndev = n;
  return 0;
}
extern "C" int pbc_hip_pairing_length_in_bytes_G1(const pbc_hip_pairing_t *p) { return p->len1; }
extern "C" int pbc_hip_pairing_length_in_bytes_G2(const pbc_hip_pairing_t *p) { return p->len2; }
extern "C" int pbc_hip_pairing_length_in_bytes_GT(const pbc_hip_pairing_t *p) { return p->lenT; }
extern "C" int pbc_hip_length_in_bytes_Fq(const pbc_hip_pairing_t *p) { return p->len_fq; }

extern "C" double pbc_hip_algorithmic_macs_per_unit(const pbc_hip_pairing_t *p, int k) {
  double n = p->nlimb;
  double per_mul = 2 * n * n + n;
  if (k < 0) return p->fq_muls_pp * per_mul;
  if (k > 1) return (p->fq_muls_prod_a * k + p->fq_muls_prod_b) * per_mul;
  return p->fq_muls_single * per_mul;
}


// Self-test of the constant block's addressing (fp.cuh: every device routine finds the block at a fixed negative offset
// from the implicit-argument pointer -- an assumption about the code object ABI that only static_asserts on sizes would
// otherwise protect).  On the first use of an object a single lane reads the block back THROUGH the device-side accessors,
// inside a non-inlined callee as the arithmetic routines do, and the host compares it with what it passed: a toolchain
// that pads or reorders the hidden arguments fails here, loudly, instead of computing with garbage constants.
template <int N>
static __device__ __noinline__ void kargs_probe_fn(uint32_t *out) {
  const FpK<N> &K = fpk<N>();
  const uint32_t *kw = reinterpret_cast<const uint32_t *>(&K);
  uint32_t sum = 0;
  for (int i = 0; i < (int) (sizeof(FpK<N>) / 4); i++) sum = sum * 31u + kw[i];
  out[0] = sum;
  const uint32_t *hw = reinterpret_cast<const uint32_t *>(&kconst<uint8_t, 0>());
  sum = 0;
  for (int i = 0; i < KOFF_END / 4; i++) sum = sum * 31u + hw[i];
  out[1] = sum;
  out[2] = K.p[0];
  out[3] = K.fbytes;
  out[4] = hw[0];
  out[5] = hw[KOFF_END / 4 - 1];
}
template <int N>
__global__ void kargs_selftest_kernel(uint32_t *out, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  kargs_probe_fn<N>(out);
}
template <int N>
static int kargs_selftest(pbc_hip_pairing_s *P, hipStream_t s) {
  KArgs<N> K = kargs<N>(P);
  // sentinels at both ends of the head: a shifted block cannot pass by reading zeros against zeros
  uint32_t first = 0x5eed0001u, last = 0x5eed0002u;
  memcpy(K.head, &first, 4);
  memcpy(K.head + KOFF_END - 4, &last, 4);
  uint32_t want[6], got[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t *kw = reinterpret_cast<const uint32_t *>(&K.fp);
  uint32_t sum = 0;
  for (size_t i = 0; i < sizeof(FpK<N>) / 4; i++) sum = sum * 31u + kw[i];
  want[0] = sum;
  const uint32_t *hw = reinterpret_cast<const uint32_t *>(K.head);
  sum = 0;
  for (int i = 0; i < KOFF_END / 4; i++) sum = sum * 31u + hw[i];
  want[1] = sum;
  want[2] = K.fp.p[0];
  want[3] = K.fp.fbytes;
  want[4] = first;
  want[5] = last;
  DevBuf buf;
  HIP_TRY(buf.alloc(sizeof got));
  HIP_TRY(hipMemsetAsync(buf.p, 0, sizeof got, s));
  hipLaunchKernelGGL(kargs_selftest_kernel<N>, dim3(1), dim3(64), 0, s, buf.as<uint32_t>(), K);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(got, buf.p, sizeof got, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (memcmp(want, got, sizeof got) != 0)
    return fail("self-test of the kernel-argument constant block failed for %d-word fields (device read %08x %08x %08x %u %08x %08x, host passed "
                "%08x %08x %08x %u %08x %08x): this build of libpbc_hip does not match the toolchain's hidden-argument layout", N,
                got[0], got[1], got[2], got[3], got[4], got[5], want[0], want[1], want[2], want[3], want[4], want[5]);
  return 0;
}

// First use of an object on a device: constants that are derived ON the device (the library carries no host-side copy of
// the tower arithmetic) are computed by single-lane kernels of the family's translation unit and kept in the object;
// every later launch passes them in its argument block.  Nothing is uploaded per call.
int ensure_derived(pbc_hip_pairing_s *P, hipStream_t s) {
  if (!P->kargs_checked) {
    PBC_DISPATCH_N(P->nlimb, { if (kargs_selftest<N>(P, s)) return 1; });
    P->kargs_checked = true;
  }
  if (P->dev_ready || (P->type != 'd' && P->type != 'g' && P->type != 'e' && P->type != 'f')) return 0;
  if (P->type == 'd' || P->type == 'g') { if (derive_d(P, s)) return 1; }
  else if (P->type == 'e') { if (derive_e(P, s)) return 1; }
  else if (derive_f(P, s)) return 1;
  P->dev_ready = true;
  return 0;
}

// Grid of a resident-workgroup launch (PBC_RESIDENT_LOOP): the workgroups the current device holds at once for this
// kernel (occupancy query, cached per kernel and device), or one per 128 units when the batch is smaller than that.
// PBC_HIP_RESIDENT=0 restores one workgroup per 128 units (A/B measurements).
unsigned resident_grid(const pbc_hip_pairing_s *P, const void *kernel, size_t n) {
  const size_t nvb = (n + kBlock - 1) / kBlock;
  if (P->resident_slots > 0) return (unsigned) (nvb < (size_t) P->resident_slots ? nvb : (size_t) P->resident_slots);   // "hip_resident_slots N" (tests)
  static const bool off = [] { const char *e = getenv("PBC_HIP_RESIDENT"); return e && e[0] == '0'; }();
  if (off) return (unsigned) nvb;
  static std::mutex mu;
  static std::vector<std::pair<std::pair<const void *, int>, size_t>> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return (unsigned) nvb;
  size_t slots = 0;
  {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : cache) if (e.first.first == kernel && e.first.second == dev) slots = e.second;
    if (!slots) {
      int per_cu = 0, cus = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0) != hipSuccess || per_cu < 1 ||
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
        (void) hipGetLastError();
        return (unsigned) nvb;
      }
      slots = (size_t) per_cu * (size_t) cus;
      cache.push_back({{kernel, dev}, slots});
    }
  }
  return (unsigned) (nvb < slots ? nvb : slots);
}

// "hip_dynamic 1": the counter a resident launch fetches its 64-unit blocks from -- one of a small ring of device words
// per (object, device), zeroed on the launch's stream right before the kernel (a ring, so that launches in flight on
// different streams do not share one)
constexpr int kCounters = 64;
struct CounterRing { int dev; unsigned *p; unsigned next; };
static std::mutex g_ctr_mu;
unsigned *unit_counter(pbc_hip_pairing_s *P, hipStream_t s) {
  if (!P->dynamic) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_ctr_mu);
  if (!P->counters) P->counters = new std::vector<CounterRing>();
  auto *rings = static_cast<std::vector<CounterRing> *>(P->counters);
  CounterRing *r = nullptr;
  for (auto &x : *rings) if (x.dev == dev) r = &x;
  if (!r) {
    unsigned *p = nullptr;
    if (hipMalloc(&p, kCounters * sizeof(unsigned)) != hipSuccess) return nullptr;     // (falls back to the fixed stride)
    rings->push_back(CounterRing{dev, p, 0});
    r = &rings->back();
  }
  unsigned *c = r->p + (r->next++ % kCounters);
  if (hipMemsetAsync(c, 0, sizeof(unsigned), s) != hipSuccess) return nullptr;
  return c;
}
static int launch_prod(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k,
                       hipStream_t s, bool upload, const OwnWs *own = nullptr);
static int launch_pairing(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n,
                          hipStream_t s, bool upload) {
  return launch_prod(P, d_gt, d_g1, d_g2, n, 1, s, upload);
}
extern "C" int pbc_hip_element_pairing_batch_dev(pbc_hip_pairing_t *P, void *d_gt, const void *d_g1,
                                                 const void *d_g2, size_t n, void *stream) {
  if (!P) return fail("null pairing");
  return launch_pairing(P, d_gt, d_g1, d_g2, n, (hipStream_t) stream, true);
}

// ---- host-buffer path --------------------------------------------------------------------
// The batch is cut into one chunk per device of the object's device set (more when a share exceeds 2^20 units or 2 GB of
// records: run_host).  Page-locked caller buffers (pbc_hip_host_alloc, hipHostMalloc, torch's pin_memory) are read and
// written by the kernels IN PLACE (pinned_dev_ptr below; "hip_zero_copy 0" in the parameter text turns that off); any
// other memory travels H2D -> kernel -> D2H through chunk buffers on a ring of three streams PER DEVICE (the runtime stages
// pageable memory).  Consecutive chunks go to the devices in turn (pbc_hip_pairing_use_devices: range split, no exchange between devices,
// results land directly in the caller's buffer), each device driven by its own host thread.
// Streams and chunk buffers belong to the object: they are created on first use per device, grow when a larger chunk
// arrives and are released by pbc_hip_pairing_clear -- a call allocates nothing in the steady state.
constexpr int kSlots = 3, kMaxDev = 16;
// Zero-copy: the device address of a page-locked (hipHostMalloc / hipHostRegister) host range the kernels may work on
// in place, or nullptr for any other memory.  `shared`: the range must be visible to every device of a device set
// (allocated with hipHostMallocPortable, as pbc_hip_host_alloc does).
// Why in place: a lane reads its 2 x 128-byte record once (16-byte loads; a few microseconds over PCIe against the ~10 ms
// of a pairing) and writes 128 bytes, while staged copies do not overlap with kernels that hold every register and LDS
// byte of the chip.  Measured (round 3, profiles/r03_notes.md; pinned host -> pinned host, ms per batch, staged / in place):
// type a 2^20 90.1 / 81.6 (kernel alone: 81.7), 16-term type a products 2^18 281.2 / 260.5, type f 2^18 30.8 / 28.5.
void *pinned_dev_ptr(const void *host, size_t bytes, bool shared) {
  if (reinterpret_cast<uintptr_t>(host) % 16) return nullptr;      // the kernels' 16-byte accesses; staged buffers are aligned
  hipPointerAttribute_t at, at_end;
  if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
  if (at.type != hipMemoryTypeHost) return nullptr;
  // the LAST byte must belong to the same page-locked allocation: a buffer that starts inside a registered range and
  // runs past its end would fault in the kernel (staged, it is copied correctly)
  if (bytes > 1) {
    if (hipPointerGetAttributes(&at_end, static_cast<const uint8_t *>(host) + bytes - 1) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
    if (at_end.type != hipMemoryTypeHost) return nullptr;
    // device addresses run in step with host addresses inside one mapping
    if ((static_cast<const uint8_t *>(at_end.devicePointer) - static_cast<const uint8_t *>(at.devicePointer)) != (ptrdiff_t) (bytes - 1)) return nullptr;
  }
  if (shared) {
    unsigned flags = 0;
    if (hipHostGetFlags(&flags, const_cast<void *>(host)) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
    if (!(flags & hipHostMallocPortable)) return nullptr;
  }
  void *d = nullptr;
  if (hipHostGetDevicePointer(&d, const_cast<void *>(host), 0) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
  return d;
}
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}
struct DevCtx {
  int dev = -1;
  hipStream_t st[kSlots] = {nullptr, nullptr, nullptr};
  void *d1[kSlots] = {nullptr, nullptr, nullptr}, *d2[kSlots] = {nullptr, nullptr, nullptr}, *dt[kSlots] = {nullptr, nullptr, nullptr};
  size_t cap1[kSlots] = {0, 0, 0}, cap2[kSlots] = {0, 0, 0}, capt[kSlots] = {0, 0, 0};   // bytes of each slot's chunk buffers (slots are allocated when first used)
  void *ws[kSlots] = {nullptr, nullptr, nullptr};                                          // product workspace of each slot's stream (launch_prod)
  size_t wscap[kSlots] = {0, 0, 0};
  void *ws2[kSlots] = {nullptr, nullptr, nullptr};                                         // ... and its second buffer (ProdWs::get2)
  size_t ws2cap[kSlots] = {0, 0, 0};
  HostStage hs[kSlots];                                                                    // ... and its host staging (ProdWs::stage)
};
// Workspaces of the product kernels (per-term Miller state).  The host-buffer path owns one per stream of its device
// contexts (DevCtx::ws: they live and die with the streams).  Launches of the *_dev entry points on CALLER streams get one
// per (device, stream) from the table below: launches on one stream are ordered, so they may share a buffer; launches on
// different streams get their own.  At most kMaxWs are kept: a caller that launches on ever new streams evicts the least
// recently used entry that is not pinned by a launch in progress (after a device synchronisation -- its stream may no
// longer exist), so the footprint stays bounded and a recycled stream handle cannot alias a stale entry for long.
// `issue` is held from workspace_get to workspace_unpin, i.e. while ONE call enqueues its kernels: two host threads that
// launch on the same (object, stream) pair take turns, so the complete pass of a two-pass operation always reads the flags
// its own fast pass wrote (the stream runs each call's kernels back to back).  Recursive: a call may ask twice.
// p2 / cap2: the entry's second buffer (ProdWs::get2: intermediates a composed call keeps across a launcher's own request).
struct WsEnt { int dev; hipStream_t st; void *p; size_t cap; uint64_t used; int pins; std::recursive_mutex issue; void *p2 = nullptr; size_t cap2 = 0; HostStage hs; };
constexpr size_t kMaxWs = 8;
// Small device buffers that belong to the object and a device, kept until the object is cleared: the schedule of the type d
// wave kernel (read-only, shared by every launch), the wire-format staging area of the limb-image host calls.  Plain
// hipMalloc: the stream-ordered allocator (hipMallocAsync) is NOT used on paths the glue reaches -- under the system HIP
// runtime (a process without torch's bundled one) launches that worked on hipMallocAsync memory faulted or, called from a
// fresh thread per chunk, returned wrong results after a few calls (round 6; the same calls passed under torch's runtime).
struct ScratchEnt { int dev; const void *key; void *p; size_t cap; };
struct HostCtx {
  std::vector<ScratchEnt> scratch;
  DevCtx dc[kMaxDev];
  int n = 0;
  std::vector<std::unique_ptr<WsEnt>> ws;      // (stable addresses: a launch holds its entry while the table changes)
  uint64_t ws_clock = 0;
  std::mutex mu;                               // guards the tables (the per-device entries are used by one worker each)
};
void *stage_acquire(HostStage &st, size_t bytes) {
  if (st.pending) { (void) hipEventSynchronize(st.ev); st.pending = false; }
  if (st.cap < bytes) {
    if (st.h) (void) hipHostFree(st.h);
    st.h = nullptr; st.cap = 0;
    if (hipHostMalloc(&st.h, bytes, hipHostMallocPortable) != hipSuccess) { st.h = nullptr; fail("hipHostMalloc(%zu) failed for a plan's staging", bytes); return nullptr; }
    st.cap = bytes;
  }
  if (!st.ev && hipEventCreateWithFlags(&st.ev, hipEventDisableTiming) != hipSuccess) { st.ev = nullptr; fail("hipEventCreate failed"); return nullptr; }
  return st.h;
}
int stage_copied(HostStage &st, hipStream_t s) {
  HIP_TRY(hipEventRecord(st.ev, s));
  st.pending = true;
  return 0;
}
void stage_free(HostStage &st) {          // (the device the staging was used on is current and idle)
  if (st.ev) (void) hipEventDestroy(st.ev);
  if (st.h) (void) hipHostFree(st.h);
  st = HostStage();
}
static void scratch_free_all(HostCtx *H) {
  for (ScratchEnt &x : H->scratch) {
    DeviceGuard guard(x.dev);
    (void) hipDeviceSynchronize();
    if (x.p) (void) hipFree(x.p);
  }
  H->scratch.clear();
}
static void devctx_free_buffers(DevCtx &c) {   // the calling thread's current device is c.dev
  for (int i = 0; i < kSlots; i++) {
    if (c.st[i]) (void) hipStreamSynchronize(c.st[i]);
    if (c.d1[i]) (void) hipFree(c.d1[i]);
    if (c.d2[i]) (void) hipFree(c.d2[i]);
    if (c.dt[i]) (void) hipFree(c.dt[i]);
    if (c.ws[i]) (void) hipFree(c.ws[i]);
    if (c.ws2[i]) (void) hipFree(c.ws2[i]);
    stage_free(c.hs[i]);
    c.d1[i] = c.d2[i] = c.dt[i] = c.ws[i] = c.ws2[i] = nullptr;
    c.cap1[i] = c.cap2[i] = c.capt[i] = c.wscap[i] = c.ws2cap[i] = 0;
  }
}
static void devctx_release(DevCtx &c) {
  if (c.dev < 0) return;
  DeviceGuard guard(c.dev);
  devctx_free_buffers(c);
  for (int i = 0; i < kSlots; i++) {
    if (c.st[i]) (void) hipStreamDestroy(c.st[i]);
    c.st[i] = nullptr;
  }
  c.dev = -1;
}
static void hostctx_free(pbc_hip_pairing_s *P) {
  if (P->counters) {
    auto *rings = static_cast<std::vector<CounterRing> *>(P->counters);
    for (auto &x : *rings) { DeviceGuard guard(x.dev); (void) hipDeviceSynchronize(); (void) hipFree(x.p); }
    delete rings;
    P->counters = nullptr;
  }
  HostCtx *H = static_cast<HostCtx *>(P->host_ctx);
  if (!H) return;
  for (auto &w : H->ws) {
    DeviceGuard guard(w->dev);
    (void) hipDeviceSynchronize();
    (void) hipFree(w->p);
    (void) hipFree(w->p2);
    stage_free(w->hs);
  }
  scratch_free_all(H);
  for (int i = 0; i < H->n; i++) devctx_release(H->dc[i]);
  delete H;
  P->host_ctx = nullptr;
}
// At least `bytes` of device memory for a kernel about to be launched on stream `s` of the current device; kept by the
// object, grown on demand (the only allocation a steady-state call can make).  The entry is PINNED until
// workspace_unpin: an entry whose kernel has not been enqueued yet is never evicted.
void *workspace_get(pbc_hip_pairing_s *P, hipStream_t s, size_t bytes, int part) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) { fail("no current HIP device"); return nullptr; }
  if (!P->host_ctx) P->host_ctx = new HostCtx();
  HostCtx *H = static_cast<HostCtx *>(P->host_ctx);
  WsEnt *e = nullptr;
  {
    std::lock_guard<std::mutex> lk(H->mu);
    for (auto &w : H->ws)
      if (w->dev == dev && w->st == s) e = w.get();
    if (!e) {
      if (H->ws.size() >= kMaxWs) {        // evict the least recently used entry that no launch holds
        size_t lru = H->ws.size();
        for (size_t i = 0; i < H->ws.size(); i++)
          if (!H->ws[i]->pins && (lru == H->ws.size() || H->ws[i]->used < H->ws[lru]->used)) lru = i;
        if (lru < H->ws.size()) {
          {
            DeviceGuard guard(H->ws[lru]->dev);
            (void) hipDeviceSynchronize();
            if (H->ws[lru]->p) (void) hipFree(H->ws[lru]->p);
            if (H->ws[lru]->p2) (void) hipFree(H->ws[lru]->p2);
            stage_free(H->ws[lru]->hs);
          }
          H->ws.erase(H->ws.begin() + (long) lru);
        }                                  // (every entry pinned: the table grows past kMaxWs for the moment)
      }
      H->ws.emplace_back(new WsEnt{dev, s, nullptr, 0, 0, 0, {}, nullptr, 0});
      e = H->ws.back().get();
    }
    e->used = ++H->ws_clock;
    e->pins++;
  }
  e->issue.lock();                         // (outside the table lock: another thread may be enqueueing on this entry)
  void *&buf = part ? e->p2 : e->p;
  size_t &cap = part ? e->cap2 : e->cap;
  if (cap < bytes) {
    if (buf) { (void) hipStreamSynchronize(s); (void) hipFree(buf); buf = nullptr; cap = 0; }
    if (hipMalloc(&buf, bytes) != hipSuccess) {
      buf = nullptr;
      e->issue.unlock();
      { std::lock_guard<std::mutex> lk(H->mu); e->pins--; }
      fail("device allocation of a %zu-byte product workspace failed", bytes);
      return nullptr;
    }
    cap = bytes;
  }
  return buf;
}
void workspace_unpin(pbc_hip_pairing_s *P, hipStream_t s) {
  int dev = -1;
  HostCtx *H = static_cast<HostCtx *>(P->host_ctx);
  if (!H || hipGetDevice(&dev) != hipSuccess) return;
  WsEnt *e = nullptr;
  {
    std::lock_guard<std::mutex> lk(H->mu);
    for (auto &w : H->ws)
      if (w->dev == dev && w->st == s && w->pins > 0) e = w.get();
    if (e) e->pins--;
  }
  if (e) e->issue.unlock();                // (the calling thread is the one that locked it: ProdWs is scoped to one call)
}
HostStage *workspace_stage(pbc_hip_pairing_s *P, hipStream_t s) {
  int dev = -1;
  HostCtx *H = static_cast<HostCtx *>(P->host_ctx);
  if (!H || hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(H->mu);
  for (auto &w : H->ws)
    if (w->dev == dev && w->st == s && w->pins > 0) return &w->hs;
  return nullptr;
}
// at least `bytes` of device memory for (current device, key); *fresh = the buffer was (re)allocated: its old contents are gone
void *object_scratch(pbc_hip_pairing_s *P, const void *key, size_t bytes, bool *fresh) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) { fail("no current HIP device"); return nullptr; }
  if (!P->host_ctx) P->host_ctx = new HostCtx();
  HostCtx *H = static_cast<HostCtx *>(P->host_ctx);
  std::lock_guard<std::mutex> lk(H->mu);
  ScratchEnt *e = nullptr;
  for (ScratchEnt &x : H->scratch) if (x.dev == dev && x.key == key) e = &x;
  if (!e) { H->scratch.push_back(ScratchEnt{dev, key, nullptr, 0}); e = &H->scratch.back(); }
  if (fresh) *fresh = false;
  if (e->cap < bytes) {
    if (e->p) { (void) hipDeviceSynchronize(); (void) hipFree(e->p); e->p = nullptr; e->cap = 0; }
    if (hipMalloc(&e->p, bytes) != hipSuccess) { e->p = nullptr; fail("device allocation of %zu bytes failed", bytes); return nullptr; }
    e->cap = bytes;
    if (fresh) *fresh = true;
  }
  return e->p;
}
void *own_workspace(const OwnWs &o, hipStream_t s, size_t bytes) {
  if (*o.cap < bytes) {
    if (*o.p) { (void) hipStreamSynchronize(s); (void) hipFree(*o.p); *o.p = nullptr; *o.cap = 0; }
    if (hipMalloc(o.p, bytes) != hipSuccess) { *o.p = nullptr; fail("device allocation of a %zu-byte product workspace failed", bytes); return nullptr; }
    *o.cap = bytes;
  }
  return *o.p;
}
extern "C" int pbc_hip_pairing_release_workspaces(pbc_hip_pairing_t *P) {
  if (!P) return fail("null pairing");
  HostCtx *H = static_cast<HostCtx *>(P->host_ctx);
  if (!H) return 0;
  std::lock_guard<std::mutex> lk(H->mu);
  for (auto &w : H->ws) {
    DeviceGuard guard(w->dev);
    (void) hipDeviceSynchronize();
    if (w->p) (void) hipFree(w->p);
    if (w->p2) (void) hipFree(w->p2);
    stage_free(w->hs);
  }
  H->ws.clear();
  scratch_free_all(H);
  for (int i = 0; i < H->n; i++)        // the chunk buffers and workspaces of the host-buffer path as well (the streams stay)
    if (H->dc[i].dev >= 0) {
      DeviceGuard guard(H->dc[i].dev);
      devctx_free_buffers(H->dc[i]);
    }
  return 0;
}
// the context of position `slot` of the device set (a device listed twice gets two: its workers must not share streams,
// chunk buffers or -- through the streams -- product workspaces); the calling thread's current device must be `dev`
static DevCtx *devctx_get(pbc_hip_pairing_s *P, int slot, int dev, std::string &err) {
  HostCtx *H = static_cast<HostCtx *>(P->host_ctx);
  if (slot < 0 || slot >= kMaxDev) { err = "too many devices in one object"; return nullptr; }
  DevCtx *c = &H->dc[slot];
  {
    std::lock_guard<std::mutex> lk(H->mu);
    if (slot >= H->n) H->n = slot + 1;
  }
  if (c->dev != dev) {                 // the device set changed under this position
    devctx_release(*c);
    c->dev = dev;
  }
  for (int i = 0; i < kSlots; i++)
    if (!c->st[i] && hipStreamCreateWithFlags(&c->st[i], hipStreamNonBlocking) != hipSuccess) { err = "hipStreamCreate failed"; return nullptr; }
  return c;
}
// chunk buffers of ring position `sl` with room for (b1, b2, bt) bytes: allocated when the position is first used (a device
// that gets one chunk holds one set of buffers, not three) and grown on demand
static bool devctx_slot(DevCtx *c, int sl, size_t b1, size_t b2, size_t bt, std::string &err) {
  if (b1 <= c->cap1[sl] && b2 <= c->cap2[sl] && bt <= c->capt[sl]) return true;
  (void) hipStreamSynchronize(c->st[sl]);
  auto grow = [&](void *&p, size_t &cap, size_t want) {
    if (want <= cap) return true;
    if (p) (void) hipFree(p);
    p = nullptr; cap = 0;
    if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return false; }
    cap = want;
    return true;
  };
  if (!grow(c->d1[sl], c->cap1[sl], b1) || !grow(c->d2[sl], c->cap2[sl], b2) || !grow(c->dt[sl], c->capt[sl], bt)) {
    err = "device allocation failed for the chunk buffers";
    return false;
  }
  return true;
}

// The host-buffer path of every batched entry point: n units with per-unit records of u1 and u2 bytes in (g2 may be null
// when u2 == 0) and ut bytes out; `launch` enqueues the work for one chunk on a stream (launch_prod for the pairings, the
// group operations' launcher for those).  zero_copy_ok: the kernels behind `launch` read their records with word loads.
int run_host_generic(pbc_hip_pairing_s *P, uint8_t *gt, size_t ut, const uint8_t *g1, size_t u1, const uint8_t *g2, size_t u2,
                     size_t n, const ChunkLaunch &launch, bool zero_copy_ok) {
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (!n) return 0;
  // An output range that overlaps an input range: the lanes of a launch (and the chunks of a staged call, which travel
  // on several streams) read and write in no particular order, so the results are collected in a buffer of their own
  // and copied over the caller's memory when every input has been read.
  if (ranges_overlap(gt, n * ut, g1, n * u1) || (g2 && ranges_overlap(gt, n * ut, g2, n * u2))) {
    std::vector<uint8_t> tmp(n * ut);
    if (run_host_generic(P, tmp.data(), ut, g1, u1, g2, u2, n, launch, zero_copy_ok)) return 1;
    memcpy(gt, tmp.data(), tmp.size());
    return 0;
  }
  const int ndev = P->ndev > 0 ? P->ndev : 1;
  const int *devs = P->ndev > 0 ? P->devs : &P->device;
  // Chunks: every device gets one share of the batch (at most 2^20 units and 2 GB of records per chunk; three chunk
  // buffers per device are in flight).  Round 1-2 cut a batch into chunks of one chip residency (131072 units) to overlap
  // the copies of one chunk with the kernel of another; measured on MI355X (round 3, profiles/r03_notes.md; pinned host buffers,
  // 2^20 type a pairings): 131072 units 95.2 ms, 262144: 107.3, 524288: 89.6, one chunk: 89.7 = H2D + kernel + D2H -- the
  // copies do not overlap with these kernels (every register and LDS byte of the chip is taken, and the runtime's copy
  // kernels wait for a workgroup to retire), so smaller chunks only add launches that run at partial occupancy
  // (type f, 2^18: 39.9 -> 30.3 ms; 16-term type a products: 305.7 -> 281.3 ms).
  size_t chunk = (n + (size_t) ndev - 1) / (size_t) ndev;
  if (chunk > ((size_t) 1 << 20)) chunk = (size_t) 1 << 20;
  while (chunk > 16384 && chunk * (u1 + u2 + ut) > ((size_t) 2 << 30)) chunk = (chunk + 1) / 2;
  if (P->host_chunk) chunk = P->host_chunk;
  if (chunk > n) chunk = n;
  const size_t nchunks = (n + chunk - 1) / chunk;
  const int used = (size_t) ndev < nchunks ? ndev : (int) nchunks;      // devices that receive at least one chunk
  DeviceGuard guard(devs[0]);
  if (!P->host_ctx) P->host_ctx = new HostCtx();
  if (ensure_derived(P, 0)) return 1;                // once per object, before any worker reads the constants
  uint8_t *zt = nullptr;
  const uint8_t *z1 = nullptr, *z2 = nullptr;
  // (coordinates whose length is not a multiple of four bytes are read byte by byte -- fp_load_be --, and a byte read
  // over PCIe costs a transaction: type a1, 130-byte coordinates, ran at half speed in place; those stay staged)
  if (P->zero_copy && zero_copy_ok && P->len_fq % 4 == 0) {
    zt = (uint8_t *) pinned_dev_ptr(gt, n * ut, ndev > 1);
    z1 = (const uint8_t *) pinned_dev_ptr(g1, n * u1, ndev > 1);
    z2 = g2 ? (const uint8_t *) pinned_dev_ptr(g2, n * u2, ndev > 1) : nullptr;
  }
  const bool zc = zt && z1 && (z2 || !g2);
  // chunks d, d + ndev, d + 2 ndev, ... on device devs[d]
  auto worker = [&](int d, std::string *err) {
    if (hipSetDevice(devs[d]) != hipSuccess) { *err = "hipSetDevice failed"; return; }
    DevCtx *c = devctx_get(P, d, devs[d], *err);
    if (!c) return;
    size_t round = 0;
    if (zc) {                            // the kernels work on the caller's pinned buffers: no staging copies
      const OwnWs own = {&c->ws[0], &c->wscap[0], &c->ws2[0], &c->ws2cap[0], &c->hs[0]};
      for (size_t idx = (size_t) d; idx < nchunks; idx += (size_t) ndev) {
        const size_t off = idx * chunk, m = n - off < chunk ? n - off : chunk;
        if (launch(zt + off * ut, z1 + off * u1, z2 ? z2 + off * u2 : nullptr, m, c->st[0], &own)) { *err = g_err; break; }
      }
      hipError_t e = hipStreamSynchronize(c->st[0]);
      if (e != hipSuccess && err->empty()) *err = std::string("kernel failed: ") + hipGetErrorString(e);
      return;
    }
    for (size_t idx = (size_t) d; idx < nchunks; idx += (size_t) ndev, round++) {
      const int sl = (int) (round % kSlots);
      const size_t off = idx * chunk, m = n - off < chunk ? n - off : chunk;
      hipStream_t st = c->st[sl];
      if (!devctx_slot(c, sl, chunk * u1, g2 ? chunk * u2 : 0, chunk * ut, *err)) break;
      const OwnWs own = {&c->ws[sl], &c->wscap[sl], &c->ws2[sl], &c->ws2cap[sl], &c->hs[sl]};
      if (hipMemcpyAsync(c->d1[sl], g1 + off * u1, m * u1, hipMemcpyHostToDevice, st) != hipSuccess ||
          (g2 && hipMemcpyAsync(c->d2[sl], g2 + off * u2, m * u2, hipMemcpyHostToDevice, st) != hipSuccess)) { *err = "H2D copy failed"; break; }
      if (launch(c->dt[sl], c->d1[sl], g2 ? c->d2[sl] : nullptr, m, st, &own)) { *err = g_err; break; }
      if (hipMemcpyAsync(gt + off * ut, c->dt[sl], m * ut, hipMemcpyDeviceToHost, st) != hipSuccess) { *err = "D2H copy failed"; break; }
    }
    for (int i = 0; i < kSlots; i++) {
      hipError_t e = hipStreamSynchronize(c->st[i]);
      if (e != hipSuccess && err->empty()) *err = std::string("kernel failed: ") + hipGetErrorString(e);
    }
  };
  std::string errs[kMaxDev];
  if (used == 1) {
    worker(0, &errs[0]);
  } else {
    std::thread th[kMaxDev];
    for (int d = 0; d < used; d++) th[d] = std::thread(worker, d, &errs[d]);
    for (int d = 0; d < used; d++) th[d].join();
  }
  for (int d = 0; d < used; d++)
    if (!errs[d].empty()) return fail("device %d: %s", devs[d], errs[d].c_str());
  return 0;
}

static int run_host(pbc_hip_pairing_s *P, uint8_t *gt, const uint8_t *g1, const uint8_t *g2, size_t n, int k) {
  return run_host_generic(P, gt, (size_t) P->lenT, g1, (size_t) k * P->len1, g2, (size_t) k * P->len2, n,
                          [P, k](void *d_gt, const void *d_g1, const void *d_g2, size_t m, hipStream_t s, const OwnWs *own) {
                            return launch_prod(P, d_gt, d_g1, d_g2, m, k, s, false, own);
                          }, true);
}

// Ragged products over host buffers (pbc_hip_element_prod_pairing_ragged_batch): units of different sizes, so the
// batch is cut by TERMS -- one contiguous range of products per position of the device set, balanced by term count
// (a device listed twice gets two), each range in chunks of about 2^20 terms that end at product boundaries (a longer
// product is a chunk of its own) -- and always staged: H2D, ragged_launch, D2H on the ring of three streams per device,
// through the chunk buffers, workspaces and plan staging the object keeps.  offsets: checked by the caller.
int run_host_ragged(pbc_hip_pairing_s *P, uint8_t *gt, const uint8_t *g1, const uint8_t *g2, const uint64_t *offsets, size_t n) {
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (!n) return 0;
  const size_t l1 = (size_t) P->len1, l2 = (size_t) P->len2, lt = (size_t) P->lenT;
  const uint64_t T = offsets[n];
  if (ranges_overlap(gt, n * lt, g1, T * l1) || ranges_overlap(gt, n * lt, g2, T * l2)) {
    std::vector<uint8_t> tmp(n * lt);
    if (run_host_ragged(P, tmp.data(), g1, g2, offsets, n)) return 1;
    memcpy(gt, tmp.data(), tmp.size());
    return 0;
  }
  const int ndev = P->ndev > 0 ? P->ndev : 1;
  const int *devs = P->ndev > 0 ? P->devs : &P->device;
  // range d: products first[d] .. first[d + 1], the first product at which the terms so far reach d T / ndev
  size_t first[kMaxDev + 1];
  first[0] = 0;
  for (int d = 1; d <= ndev; d++) {
    size_t u = first[d - 1];
    if (d == ndev) u = n;
    else while (u < n && offsets[u] * (uint64_t) ndev < T * (uint64_t) d) u++;
    first[d] = u;
  }
  const uint64_t chunk_terms = P->host_chunk ? (uint64_t) P->host_chunk : (uint64_t) 1 << 20;
  DeviceGuard guard(devs[0]);
  if (!P->host_ctx) P->host_ctx = new HostCtx();
  if (ensure_derived(P, 0)) return 1;
  auto worker = [&](int d, std::string *err) {
    if (first[d] == first[d + 1]) return;
    if (hipSetDevice(devs[d]) != hipSuccess) { *err = "hipSetDevice failed"; return; }
    DevCtx *c = devctx_get(P, d, devs[d], *err);
    if (!c) return;
    size_t round = 0;
    for (size_t u0 = first[d]; u0 < first[d + 1]; round++) {
      size_t u1 = u0 + 1;                // at least one product; more while the chunk stays within chunk_terms (and 2^20 products)
      while (u1 < first[d + 1] && offsets[u1 + 1] - offsets[u0] <= chunk_terms && u1 - u0 < ((size_t) 1 << 20)) u1++;
      const size_t m = u1 - u0, t0 = (size_t) offsets[u0], nt = (size_t) (offsets[u1] - offsets[u0]);
      const int sl = (int) (round % kSlots);
      hipStream_t st = c->st[sl];
      if (!devctx_slot(c, sl, nt * l1, nt * l2, m * lt, *err)) break;
      const OwnWs own = {&c->ws[sl], &c->wscap[sl], &c->ws2[sl], &c->ws2cap[sl], &c->hs[sl]};
      if (nt && (hipMemcpyAsync(c->d1[sl], g1 + t0 * l1, nt * l1, hipMemcpyHostToDevice, st) != hipSuccess ||
                 hipMemcpyAsync(c->d2[sl], g2 + t0 * l2, nt * l2, hipMemcpyHostToDevice, st) != hipSuccess)) { *err = "H2D copy failed"; break; }
      if (ragged_launch(P, c->dt[sl], c->d1[sl], c->d2[sl], offsets + u0, m, st, &own)) { *err = g_err; break; }
      if (hipMemcpyAsync(gt + u0 * lt, c->dt[sl], m * lt, hipMemcpyDeviceToHost, st) != hipSuccess) { *err = "D2H copy failed"; break; }
      u0 = u1;
    }
    for (int i = 0; i < kSlots; i++) {
      hipError_t e = hipStreamSynchronize(c->st[i]);
      if (e != hipSuccess && err->empty()) *err = std::string("kernel failed: ") + hipGetErrorString(e);
    }
  };
  std::string errs[kMaxDev];
  if (ndev == 1) {
    worker(0, &errs[0]);
  } else {
    std::thread th[kMaxDev];
    for (int d = 0; d < ndev; d++) th[d] = std::thread(worker, d, &errs[d]);
    for (int d = 0; d < ndev; d++) th[d].join();
  }
  for (int d = 0; d < ndev; d++)
    if (!errs[d].empty()) return fail("device %d: %s", devs[d], errs[d].c_str());
  return 0;
}

// A host-buffer call on the object's OWN device only (host_common.h: the calls on a table set, whose tables live there --
// a device set stays as it is for the other entry points): always staged, H2D -> launch -> D2H per chunk on the ring of
// three streams of that device's context.  The context is the one of the device's position in the device set (position
// 0 without a set), or the last position when the set does not name the device.
int run_host_own_device(pbc_hip_pairing_s *P, uint8_t *out, size_t uo, const uint8_t *in, size_t ui, size_t n, size_t chunk, const RangeLaunch &launch) {
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (!n) return 0;
  if (ranges_overlap(out, n * uo, in, n * ui)) {
    std::vector<uint8_t> tmp(n * uo);
    if (run_host_own_device(P, tmp.data(), uo, in, ui, n, chunk, launch)) return 1;
    memcpy(out, tmp.data(), tmp.size());
    return 0;
  }
  if (chunk < 1) chunk = 1;
  if (chunk > n) chunk = n;
  DeviceGuard guard(P->device);
  if (!P->host_ctx) P->host_ctx = new HostCtx();
  if (ensure_derived(P, 0)) return 1;
  int slot = 0;
  if (P->ndev > 0) {
    slot = kMaxDev - 1;
    for (int d = P->ndev - 1; d >= 0; d--) if (P->devs[d] == P->device) slot = d;
  }
  std::string err;
  DevCtx *c = devctx_get(P, slot, P->device, err);
  if (c) {
    size_t round = 0;
    for (size_t c0 = 0; c0 < n; c0 += chunk, round++) {
      const int sl = (int) (round % kSlots);
      const size_t cnt = n - c0 < chunk ? n - c0 : chunk;
      hipStream_t st = c->st[sl];
      if (!devctx_slot(c, sl, 0, chunk * ui, chunk * uo, err)) break;
      const OwnWs own = {&c->ws[sl], &c->wscap[sl], &c->ws2[sl], &c->ws2cap[sl], &c->hs[sl]};
      if (hipMemcpyAsync(c->d2[sl], in + c0 * ui, cnt * ui, hipMemcpyHostToDevice, st) != hipSuccess) { err = "H2D copy failed"; break; }
      if (launch(c->dt[sl], c->d2[sl], c0, cnt, st, &own)) { err = g_err; break; }
      if (hipMemcpyAsync(out + c0 * uo, c->dt[sl], cnt * uo, hipMemcpyDeviceToHost, st) != hipSuccess) { err = "D2H copy failed"; break; }
    }
    for (int i = 0; i < kSlots; i++) {
      hipError_t e = hipStreamSynchronize(c->st[i]);
      if (e != hipSuccess && err.empty()) err = std::string("kernel failed: ") + hipGetErrorString(e);
    }
  }
  if (!err.empty()) return fail("device %d: %s", P->device, err.c_str());
  return 0;
}

extern "C" int pbc_hip_host_alloc(void **out, size_t bytes) {
  if (!out) return fail("null argument");
  if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) return fail("hipHostMalloc(%zu) failed", bytes);
  return 0;
}
extern "C" void pbc_hip_host_free(void *p) { if (p) (void) hipHostFree(p); }

extern "C" int pbc_hip_element_pairing_batch(pbc_hip_pairing_t *P, uint8_t *gt, const uint8_t *g1,
                                             const uint8_t *g2, size_t n) {
  if (!P) return fail("null pairing");
  return run_host(P, gt, g1, g2, n, 1);
}

static int launch_prod(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k,
                       hipStream_t s, bool upload, const OwnWs *own) {
  if (k < 1) return fail("k must be >= 1");
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (!n) return 0;
  if (upload && ensure_derived(P, s)) return 1;
  ProdWs W(P, s, own);
  if (P->type == 'a' || P->type == '1' || P->type == 'e') return launch_a(P, d_gt, d_g1, d_g2, n, k, s, W);
  if (P->type == 'd' || P->type == 'g') return launch_d(P, d_gt, d_g1, d_g2, n, k, s, W);
  if (P->type == 'f') return launch_f(P, d_gt, d_g1, d_g2, n, k, s, W);
  return fail("unsupported type");
}
int launch_pairings(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, hipStream_t s, const OwnWs *own) {
  return launch_prod(P, d_gt, d_g1, d_g2, n, 1, s, false, own);
}
extern "C" int pbc_hip_element_prod_pairing_batch_dev(pbc_hip_pairing_t *P, void *d_gt, const void *d_g1,
                                                      const void *d_g2, size_t n, int k, void *stream) {
  if (!P) return fail("null pairing");
  return launch_prod(P, d_gt, d_g1, d_g2, n, k, (hipStream_t) stream, true);
}
extern "C" int pbc_hip_element_prod_pairing_batch(pbc_hip_pairing_t *P, uint8_t *gt, const uint8_t *g1,
                                                  const uint8_t *g2, size_t n, int k) {
  if (!P) return fail("null pairing");
  if (k < 1) return fail("k must be >= 1");
  return run_host(P, gt, g1, g2, n, k);
}

// ---- the reference's own limb image as the exchange format (round 6; the element_t route of integration/pbc_hip_glue.c) ----
// element_to_bytes / element_from_bytes cost the host a Montgomery reduction, a GMP export and two allocations per F_q
// coordinate (arith/montfp.c:487-517): 16 host threads convert 4.8 M type a pairs/s while the GPU pairs 13 M
// (profiles/r05_closing_glue.txt).  These entry points take what a montfp element holds (montfp.c:36-39: t = ceil(bits(q) /
// 64) little-endian 64-bit limbs of x 2^(64 t) mod q, fully reduced) -- a memcpy per coordinate on the host -- and do the
// change of Montgomery radix on the device: one F_q product per coordinate with 2^(2 rbits - 64 t) on the way in (then
// the wire format's kernels run unchanged), one with 2^(64 t) on the way out.  A record is the wire record with every
// length_in_bytes(F_q)-byte coordinate replaced by its 8 t-byte limb image; a zero coordinate is t zero limbs.
template <int N>
__global__ void __launch_bounds__(kBlock) raw_to_wire_kernel(uint8_t *out, const uint32_t *in, int words, fp<N> c1, size_t n, KArgs<N> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  fp<N> w, z;
#pragma unroll
  for (int i = 0; i < N; i++) w.v[i] = i < words ? in[idx * (size_t) words + i] : 0;   // (words = 2 t is N or N + 1; the top word of an odd N is zero)
  fp_mul<N>(z, w, c1);                                    // x R_pbc (R^2 / R_pbc) / R = x R: this library's form
  fp_store_be<N>(out + idx * fpk<N>().fbytes, z);
}
template <int N>
__global__ void __launch_bounds__(kBlock) wire_to_raw_kernel(uint32_t *out, const uint8_t *in, int words, fp<N> c2, size_t n, KArgs<N> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  fp<N> x, z;
  fp_load_be<N>(x, in + idx * fpk<N>().fbytes);           // x R
  fp_mul<N>(z, x, c2);                                    // x R R_pbc / R = x R_pbc mod q
#pragma unroll
  for (int i = 0; i <= N; i++)                             // compile-time indices into the register array (words is N or N + 1)
    if (i < words) out[idx * (size_t) words + i] = i < N ? z.v[i < N ? i : N - 1] : 0u;
}
static int raw_prepare(pbc_hip_pairing_s *P) {
  if (P->raw_t) return 0;
  using pbc_host::Big;
  Big q;
  int bits = 0;
  PBC_DISPATCH_N(P->nlimb, { const FpK<N> K = host_fpk<N>(P); q.w.assign(K.p, K.p + N); bits = (int) K.pbits; });
  q.trim();
  const int t = (bits + 63) / 64;
  int rbits = 0;
  PBC_DISPATCH_N(P->nlimb, { rbits = Limbs29<N>::W * Limbs29<N>::L; });
  if (2 * rbits < 64 * t || 2 * t > 34) return fail("limb image: unsupported field width");
  memset(P->raw_c1, 0, sizeof P->raw_c1);
  memset(P->raw_c2, 0, sizeof P->raw_c2);
  Big::pow2_mod(2 * rbits - 64 * t, q).to_words(P->raw_c1, 34);
  Big::pow2_mod(64 * t, q).to_words(P->raw_c2, 34);
  P->raw_t = t;
  return 0;
}
extern "C" int pbc_hip_fq_limb_image_bytes(pbc_hip_pairing_t *P) {
  if (!P || raw_prepare(P)) return 0;
  return 8 * P->raw_t;
}
static int raw_convert(pbc_hip_pairing_s *P, bool to_wire, void *dst, const void *src, size_t leaves, hipStream_t s) {
  if (!leaves) return 0;
  const unsigned grid = (unsigned) ((leaves + kBlock - 1) / kBlock);
  const int words = 2 * P->raw_t;
  PBC_DISPATCH_N(P->nlimb, {
    fp<N> c;
    for (int i = 0; i < N; i++) c.v[i] = to_wire ? P->raw_c1[i] : P->raw_c2[i];
    if (to_wire) hipLaunchKernelGGL(raw_to_wire_kernel<N>, dim3(grid), dim3(kBlock), 0, s, (uint8_t *) dst, (const uint32_t *) src, words, c, leaves, kargs<N>(P));
    else hipLaunchKernelGGL(wire_to_raw_kernel<N>, dim3(grid), dim3(kBlock), 0, s, (uint32_t *) dst, (const uint8_t *) src, words, c, leaves, kargs<N>(P));
  });
  HIP_TRY(hipGetLastError());
  return 0;
}
// limb images in device memory -> the wire-format kernels -> limb images, all on stream s (stream-ordered temporaries)
// (host calls -- one at a time per object -- stage the wire records in a buffer the object keeps per device and slot of the
// chunk ring; the _dev form, which may be in flight on several streams, takes a stream-ordered temporary)
static int launch_prod_raw(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, hipStream_t s, bool upload, const OwnWs *own,
                           const void *host_key = nullptr) {
  if (!n) return 0;
  if (upload && ensure_derived(P, s)) return 1;
  const size_t fb = (size_t) P->len_fq, lv1 = P->len1 / fb, lv2 = P->len2 / fb, lvt = P->lenT / fb, terms = n * (size_t) k;
  uint8_t *tmp = nullptr;
  const size_t b1 = (terms * P->len1 + 15) & ~(size_t) 15, b2 = (terms * P->len2 + 15) & ~(size_t) 15, bt = n * (size_t) P->lenT;
  if (host_key) {
    tmp = (uint8_t *) object_scratch(P, host_key, b1 + b2 + bt, nullptr);
    if (!tmp) return 1;
  } else {
    HIP_TRY(hipMallocAsync((void **) &tmp, b1 + b2 + bt, s));
  }
  int rc = raw_convert(P, true, tmp, d_g1, terms * lv1, s) || raw_convert(P, true, tmp + b1, d_g2, terms * lv2, s) ||
           launch_prod(P, tmp + b1 + b2, tmp, tmp + b1, n, k, s, false, own) || raw_convert(P, false, d_gt, tmp + b1 + b2, n * lvt, s);
  if (!host_key) (void) hipFreeAsync(tmp, s);
  return rc;
}
extern "C" int pbc_hip_element_prod_pairing_batch_limbs(pbc_hip_pairing_t *P, uint8_t *gt, const uint8_t *g1, const uint8_t *g2, size_t n, int k) {
  if (!P) return fail("null pairing");
  if (k < 1) return fail("k must be >= 1");
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (!gt || !g1 || !g2) return fail("null argument");
  if (raw_prepare(P)) return 1;
  const size_t fb = (size_t) P->len_fq, w = 8 * (size_t) P->raw_t;
  return run_host_generic(P, gt, P->lenT / fb * w, g1, (size_t) k * (P->len1 / fb) * w, g2, (size_t) k * (P->len2 / fb) * w, n,
                          [P, k](void *d_gt, const void *d_g1, const void *d_g2, size_t m, hipStream_t s, const OwnWs *own) {
                            // (one staging buffer per slot of a device context's chunk ring: keyed by the slot's workspace cell)
                            return launch_prod_raw(P, d_gt, d_g1, d_g2, m, k, s, false, own, own ? (const void *) own->p : (const void *) P);
                          }, false);     // (staged: the images travel H2D / D2H in chunks; the conversion kernels are not run on mapped host memory)
}
extern "C" int pbc_hip_element_pairing_batch_limbs(pbc_hip_pairing_t *P, uint8_t *gt, const uint8_t *g1, const uint8_t *g2, size_t n) {
  return pbc_hip_element_prod_pairing_batch_limbs(P, gt, g1, g2, n, 1);
}
extern "C" int pbc_hip_element_prod_pairing_batch_limbs_dev(pbc_hip_pairing_t *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, void *stream) {
  if (!P) return fail("null pairing");
  if (k < 1) return fail("k must be >= 1");
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (raw_prepare(P)) return 1;
  return launch_prod_raw(P, d_gt, d_g1, d_g2, n, k, (hipStream_t) stream, true, nullptr);
}

// ---- preprocessed pairings ---------------------------------------------------------------
extern "C" int pbc_hip_pairing_pp_init(pbc_hip_pp_t **out, pbc_hip_pairing_t *P, const uint8_t *g1) {
  if (!out || !P || !g1) return fail("null argument");
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  const bool mnt = P->type == 'd' || P->type == 'g', a1 = P->type == '1' || (P->type == 'a' && P->a_generic);   // a1: bit-by-bit tables
  if (P->type != 'a' && !mnt && !a1)
    return fail("pairing_pp is built for types a, a1, d and g (other types: use element_pairing)");
  pbc_hip_pp_s *pp = new pbc_hip_pp_s();
  pp->P = P;
  void *dg1 = nullptr;
  size_t words = (size_t) (P->a.exp2 + 1) * 3 * 16;
  if (mnt) {                           // one entry per doubling and per addition of the Miller loop
    int steps = P->dconst.rbits - 1;
    for (int m = 1; m <= P->dconst.rbits - 2; m++) steps += ((P->dconst.r[m >> 5] | P->dconst.rm[m >> 5]) >> (m & 31)) & 1;
    words = (size_t) steps * 3 * (size_t) P->nlimb;
  }
  if (a1) {
    int steps = P->a.rbits - 1;
    for (int m = 1; m <= P->a.rbits - 2; m++) steps += ((P->a.r[m >> 5] | P->a.rm[m >> 5]) >> (m & 31)) & 1;
    words = (size_t) steps * 3 * (size_t) P->nlimb;
  }
  DeviceGuard guard(P->device);
  DevBuf bg1;                          // released on every return path; the table and flag belong to pp
  auto bail = [&](const char *what) {
    std::string msg = g_err[0] ? std::string(g_err) : std::string();
    if (pp->tab) (void) hipFree(pp->tab);
    if (pp->valid) (void) hipFree(pp->valid);
    delete pp;
    return msg.empty() ? fail("pairing_pp_init: %s", what) : fail("pairing_pp_init: %s (%s)", what, msg.c_str());
  };
  g_err[0] = 0;
  if (ensure_derived(P, 0)) return bail("deriving the constants failed");
  if (hipMalloc(&pp->tab, words * 4) != hipSuccess || hipMalloc(&pp->valid, 4) != hipSuccess || bg1.alloc(P->len1) != hipSuccess)
    return bail("device allocation failed");
  dg1 = bg1.p;
  if (hipMemcpy(dg1, g1, P->len1, hipMemcpyHostToDevice) != hipSuccess) return bail("H2D copy failed");
  if (mnt) { if (pp_init_launch_d(P, pp, (const uint8_t *) dg1)) return bail("no kernel for this field"); }
  else pp_init_launch_a(P, pp, (const uint8_t *) dg1, a1);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return bail(hipGetErrorString(e));
  *out = pp;
  return 0;
}
extern "C" void pbc_hip_pairing_pp_clear(pbc_hip_pp_t *pp) {
  if (!pp) return;
  DeviceGuard guard(pp->P->device);
  (void) hipFree(pp->tab);
  (void) hipFree(pp->valid);
  delete pp;
}
extern "C" int pbc_hip_pairing_pp_apply_batch_dev(pbc_hip_pp_t *pp, void *d_gt, const void *d_g2, size_t n, void *stream) {
  if (!pp) return fail("null pp");
  if (!n) return 0;
  hipStream_t s = (hipStream_t) stream;
  pbc_hip_pairing_s *P = pp->P;
  if (ensure_derived(P, s)) return 1;
  if (pp->P->type == 'd' || pp->P->type == 'g') return pp_apply_launch_d(pp, d_gt, d_g2, n, s);
  return pp_apply_launch_a(pp, d_gt, d_g2, n, s);
}
extern "C" int pbc_hip_pairing_pp_apply_batch(pbc_hip_pp_t *pp, uint8_t *gt, const uint8_t *g2, size_t n) {
  if (!pp) return fail("null pp");
  if (!n) return 0;
  pbc_hip_pairing_s *P = pp->P;
  DevBuf b2, bt;
  DeviceGuard guard(P->device);
  if (P->zero_copy && P->len_fq % 4 == 0) {   // page-locked caller buffers: the kernel works on them in place (run_host)
    void *z2 = pinned_dev_ptr(g2, n * (size_t) P->len2, false), *zt = pinned_dev_ptr(gt, n * (size_t) P->lenT, false);
    if (z2 && zt && !ranges_overlap(gt, n * (size_t) P->lenT, g2, n * (size_t) P->len2)) {
      if (pbc_hip_pairing_pp_apply_batch_dev(pp, zt, z2, n, 0)) return 1;
      HIP_TRY(hipStreamSynchronize(0));
      return 0;
    }
  }
  HIP_TRY(b2.alloc(n * P->len2));
  HIP_TRY(bt.alloc(n * P->lenT));
  HIP_TRY(hipMemcpy(b2.p, g2, n * P->len2, hipMemcpyHostToDevice));
  int rc = pbc_hip_pairing_pp_apply_batch_dev(pp, bt.p, b2.p, n, 0);
  if (!rc && hipMemcpy(gt, bt.p, n * P->lenT, hipMemcpyDeviceToHost) != hipSuccess) rc = fail("D2H copy failed");
  return rc;
}

// ---- text formats on wire-format records (host_text.h) ----------------------------------------------
namespace {
using pbc_host::Big;
using pbc_host::TextShape;
// the shape of group `group` (0 Z_r, 1 G1, 2 G2, 3 GT) of this pairing and the modulus of its base field
bool text_shape(const pbc_hip_pairing_s *P, int group, TextShape &S, Big &mod) {
  const char *t = P->param_text.data();
  const size_t n = P->param_text.size();
  const bool a1 = P->type == '1';
  if (group == 0) {
    S = TextShape{P->len_zr, 0, 0, false, false};
    return pbc_host::param_big(t, n, a1 ? "n" : "r", mod);
  }
  if (!pbc_host::param_big(t, n, a1 ? "p" : "q", mod)) return false;
  const int deg = P->type == 'd' ? 3 : P->type == 'g' ? 5 : 0;
  S = TextShape{P->len_fq, 0, 0, false, group != 3};
  if (group == 2) {
    if (deg) S.poly = deg;
    else if (P->type == 'f') S.quad = 1;
  } else if (group == 3) {
    if (P->type == 'a' || a1) S.quad = 1;
    else if (deg) { S.quad = 1; S.poly = deg; S.quad_outer = true; }
    else if (P->type == 'f') { S.quad = 1; S.poly = 6; }
    // type e: GT is F_q
  } else if (group != 1) {
    return false;
  }
  return true;
}
// curve_is_valid_point (ecc/curve.c:57-77) for the curves over F_q: y^2 = x^3 + a x + b
bool text_on_curve(const pbc_hip_pairing_s *P, const Big &x, const Big &y, const Big &q) {
  const char *t = P->param_text.data();
  const size_t n = P->param_text.size();
  Big a, b;
  if (P->type == 'a' || P->type == '1') { a.w.push_back(1); }
  else if (P->type == 'f') { if (!pbc_host::param_big(t, n, "b", b)) return false; }
  else if (!pbc_host::param_big(t, n, "a", a) || !pbc_host::param_big(t, n, "b", b)) return false;
  const Big xx = pbc_host::big_mod(Big::mul(x, x), q);
  Big rhs = Big::add(Big::add(pbc_host::big_mod(Big::mul(xx, x), q), pbc_host::big_mod(Big::mul(a, x), q)), b);
  rhs = pbc_host::big_mod(rhs, q);
  return Big::cmp(pbc_host::big_mod(Big::mul(y, y), q), rhs) == 0;
}
bool text_curve_over_fq(const TextShape &S) { return S.curve && !S.quad && !S.poly; }
bool all_zero(const uint8_t *p, int n) { for (int i = 0; i < n; i++) if (p[i]) return false; return true; }
// curve_is_valid_point for the twists (G2 of types d, f, g: curves over F_q^d / F_q^2, ecc/curve.c:57-77 through
// curve_from_bytes :609-623).  The tower arithmetic lives on the device, so the check is the library's own rule for
// records: [1] R through element_mul_zn leaves a point of the curve as it is and turns anything else into O.  Without a
// usable device (text-only use of the library) the record is taken as written -- the first batch call applies the rule.
// 1: on the curve, 0: not (the record deserialises to O), -1: the device call failed (the message is set).  The twists have
// b != 0, so the all-zero record is off the curve and [1] R != O exactly for the points of the curve -- whatever residue
// class representatives the record's coordinates use (coordinates >= q are reduced on load).
int twist_record_on_curve(const pbc_hip_pairing_t *P, int group, const uint8_t *rec, int bytes) {
  if (P->device < 0) return 1;
  std::vector<uint8_t> one((size_t) P->len_zr, 0), out((size_t) bytes, 0);
  one.back() = 1;
  if (pbc_hip_element_mul_zn_batch(const_cast<pbc_hip_pairing_t *>(P), group, out.data(), rec, one.data(), 1)) return -1;
  return all_zero(out.data(), bytes) ? 0 : 1;
}
}  // namespace

extern "C" int pbc_hip_element_snprint(const pbc_hip_pairing_t *P, int group, char *s, size_t n, const uint8_t *rec) {
  if (!P || !rec || (!s && n)) { fail("null argument"); return -1; }
  TextShape S;
  Big mod;
  if (!text_shape(P, group, S, mod)) { fail("element_snprint: group must be 0 (Zr), 1, 2 or 3 (GT)"); return -1; }
  std::string out;
  if (S.curve) {
    const int cb = S.coord_bytes();
    bool inf = all_zero(rec, 2 * cb) && P->type != 'a' && P->type != '1';     // (0, 0) lies on y^2 = x^3 + x
    if (!inf && text_curve_over_fq(S))   // element_from_bytes turns a record off the curve into O (curve_from_bytes, ecc/curve.c:609-623)
      inf = !text_on_curve(P, pbc_host::big_mod(pbc_host::big_from_be(rec, cb), mod), pbc_host::big_mod(pbc_host::big_from_be(rec + cb, cb), mod), mod);
    if (!inf && !text_curve_over_fq(S)) {
      const int on = twist_record_on_curve(P, group, rec, 2 * cb);
      if (on < 0) return -1;
      inf = on == 0;
    }
    if (inf) out = "O";
    else {
      out = "[";
      pbc_host::text_field(out, S, rec, mod);
      out += ", ";
      pbc_host::text_field(out, S, rec + cb, mod);
      out += "]";
    }
  } else {
    pbc_host::text_field(out, S, rec, mod);
  }
  if (n) {
    const size_t c = out.size() < n - 1 ? out.size() : n - 1;
    memcpy(s, out.data(), c);
    s[c] = 0;
  }
  return (int) out.size();
}
extern "C" int pbc_hip_element_set_str(const pbc_hip_pairing_t *P, int group, uint8_t *rec, const char *s, int base) {
  if (!P || !rec || !s) { fail("null argument"); return 0; }
  TextShape S;
  Big mod;
  if (!text_shape(P, group, S, mod)) { fail("element_set_str: group must be 0 (Zr), 1, 2 or 3 (GT)"); return 0; }
  if (!S.curve) return pbc_host::parse_field(S, rec, s, base, mod);
  const int cb = S.coord_bytes();
  memset(rec, 0, (size_t) 2 * cb);
  const char *cp = s;
  while (*cp && isspace((unsigned char) *cp)) cp++;
  if (*cp == 'O') return (int) (cp - s + 1);
  if (*cp != '[') return 0;
  cp++;
  cp += pbc_host::parse_field(S, rec, cp, base, mod);
  while (*cp && isspace((unsigned char) *cp)) cp++;
  if (*cp != ',') { memset(rec, 0, (size_t) 2 * cb); return 0; }
  cp++;
  cp += pbc_host::parse_field(S, rec + cb, cp, base, mod);
  if (*cp != ']') { memset(rec, 0, (size_t) 2 * cb); return 0; }
  if (text_curve_over_fq(S) && !text_on_curve(P, pbc_host::big_from_be(rec, cb), pbc_host::big_from_be(rec + cb, cb), mod)) {
    memset(rec, 0, (size_t) 2 * cb);     // curve_set_str: not on the curve -> O, returns 0
    return 0;
  }
  if (!text_curve_over_fq(S) && !all_zero(rec, 2 * cb) && twist_record_on_curve(P, group, rec, 2 * cb) <= 0) {
    memset(rec, 0, (size_t) 2 * cb);     // off the curve -> O; a failed device call also returns 0, with pbc_hip_last_error set
    return 0;
  }
  return (int) (cp - s + 1);
}
extern "C" int pbc_hip_param_snprint(const pbc_hip_pairing_t *P, char *s, size_t n) {
  if (!P || (!s && n)) { fail("null argument"); return -1; }
  static const char *const KA[] = {"q", "h", "r", "exp2", "exp1", "sign1", "sign0", nullptr};
  static const char *const K1[] = {"p", "n", "l", nullptr};
  static const char *const KD[] = {"q", "n", "h", "r", "a", "b", "k", "nk", "hk", "coeff0", "coeff1", "coeff2", "nqr", nullptr};
  static const char *const KE[] = {"q", "r", "h", "a", "b", "exp2", "exp1", "sign1", "sign0", nullptr};
  static const char *const KF[] = {"q", "r", "b", "beta", "alpha0", "alpha1", nullptr};
  static const char *const KG[] = {"q", "n", "h", "r", "a", "b", "nk", "hk", "coeff0", "coeff1", "coeff2", "coeff3", "coeff4", "nqr", nullptr};
  const char *const *keys = P->type == 'a' ? KA : P->type == '1' ? K1 : P->type == 'd' ? KD : P->type == 'e' ? KE : P->type == 'f' ? KF : KG;
  std::string out = std::string("type ") + (P->type == '1' ? "a1" : std::string(1, (char) P->type)) + "\n";
  for (; *keys; keys++) {
    std::string v;
    if (!pbc_host::param_lookup(P->param_text.data(), P->param_text.size(), *keys, v)) { fail("param_snprint: key %s is missing", *keys); return -1; }
    const bool neg = !v.empty() && v[0] == '-';
    Big z;
    const std::string digits = v.substr(neg || (!v.empty() && v[0] == '+') ? 1 : 0);
    if (!Big::from_dec(z, digits)) { fail("param_snprint: %s is not a decimal integer", *keys); return -1; }
    out += std::string(*keys) + " " + (neg && !z.is_zero() ? "-" : "") + pbc_host::big_to_dec(z) + "\n";
  }
  if (n) {
    const size_t c = out.size() < n - 1 ? out.size() : n - 1;
    memcpy(s, out.data(), c);
    s[c] = 0;
  }
  return (int) out.size();
}

// diagnostics: stage 0 -> the derived constant block of the object (after device init);
// stage 1 (type F) -> Miller values before the final exponentiation
extern "C" int pbc_hip_diag_stage(pbc_hip_pairing_t *P, int stage, uint8_t *out, size_t out_len,
                                  const uint8_t *g1, const uint8_t *g2, size_t n) {
  if (!P) return fail("null pairing");
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (stage == 0) {
    if (ensure_derived(P, 0)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    const void *src = (P->type == 'd' || P->type == 'g') ? (const void *) &P->dconst : P->type == 'f' ? (const void *) &P->fconst : (const void *) &P->a;
    size_t len = (P->type == 'd' || P->type == 'g') ? sizeof P->dconst : P->type == 'f' ? sizeof P->fconst : sizeof P->a;
    memcpy(out, src, len < out_len ? len : out_len);
    return 0;
  }
  if (stage == 1 && P->type == 'f') {
    DevBuf b1, b2, bt;
    HIP_TRY(b1.alloc(n * P->len1));
    HIP_TRY(b2.alloc(n * P->len2));
    HIP_TRY(bt.alloc(n * P->lenT));
    HIP_TRY(hipMemcpy(b1.p, g1, n * P->len1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b2.p, g2, n * P->len2, hipMemcpyHostToDevice));
    if (ensure_derived(P, 0)) return 1;
    if (diag_f_miller(P, bt.p, b1.p, b2.p, n)) return 1;
    HIP_TRY(hipMemcpy(out, bt.p, n * P->lenT < out_len ? n * P->lenT : out_len, hipMemcpyDeviceToHost));
    return 0;
  }
  if (stage >= 10 && P->type == 'f') {   // g1 = operand A, g2 = operand B (GT-format records)
    DevBuf b1, b2, bt;
    size_t bytes = n * P->lenT;
    HIP_TRY(b1.alloc(bytes));
    HIP_TRY(b2.alloc(bytes));
    HIP_TRY(bt.alloc(bytes));
    HIP_TRY(hipMemcpy(b1.p, g1, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b2.p, g2, bytes, hipMemcpyHostToDevice));
    if (ensure_derived(P, 0)) return 1;
    if (diag_f_op(P, stage, bt.p, b1.p, b2.p, n)) return 1;
    HIP_TRY(hipMemcpy(out, bt.p, bytes < out_len ? bytes : out_len, hipMemcpyDeviceToHost));
    return 0;
  }
  return fail("unknown diagnostic stage");
}

extern "C" int pbc_hip_fq_op_batch(pbc_hip_pairing_t *P, int op, uint8_t *c, const uint8_t *a,
                                   const uint8_t *b, size_t n) {
  if (!P) return fail("null pairing");
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (!n) return 0;
  if (op < 0 || op > 6) return fail("bad op");
  size_t bytes = n * (size_t) P->len_fq;
  DevBuf ba, bb, bc;
  DeviceGuard guard(P->device);
  HIP_TRY(ba.alloc(bytes));
  HIP_TRY(bc.alloc(bytes));
  void *da = ba.p, *db = nullptr, *dc = bc.p;
  HIP_TRY(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
  if (b) {
    HIP_TRY(bb.alloc(bytes));
    db = bb.p;
    HIP_TRY(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice));
  }
  if (ensure_derived(P, 0)) return 1;
  unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  PBC_DISPATCH_N(P->nlimb, hipLaunchKernelGGL(fq_op_kernel<N>, dim3(grid), dim3(kBlock), 0, 0, op, (uint8_t *) dc,
                                              (const uint8_t *) da, (const uint8_t *) db, n, kargs<N>(P)));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(c, dc, bytes, hipMemcpyDeviceToHost));
  return 0;
}

template <int V>
static int run_probe(int iters, double *rate, double *ms_out, double ops_per_iter) {
  uint32_t *sink;
  HIP_TRY(hipMalloc(&sink, 64));
  int dev;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  int grid = prop.multiProcessorCount * 8;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  hipLaunchKernelGGL(probe_kernel<V>, dim3(grid), dim3(256), 0, 0, sink, iters / 4 + 1, 1u);
  HIP_TRY(hipEventRecord(e0, 0));
  hipLaunchKernelGGL(probe_kernel<V>, dim3(grid), dim3(256), 0, 0, sink, iters, 3u);
  HIP_TRY(hipEventRecord(e1, 0));
  HIP_TRY(hipEventSynchronize(e1));
  float ms;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  double total = (double) grid * 256.0 * (double) iters * ops_per_iter;
  *rate = total / (ms * 1e-3);
  *ms_out = ms;
  (void) hipFree(sink);
  (void) hipEventDestroy(e0);
  (void) hipEventDestroy(e1);
  return 0;
}

template <int V>
static int run_mul_bench(int iters, int waves_per_simd, double *rate, double *ms_out) {
  int dev;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  int grid = prop.multiProcessorCount * waves_per_simd;
  size_t words = (size_t) grid * 256 * 32;
  uint32_t *in, *out;
  HIP_TRY(hipMalloc(&in, words * 4));
  HIP_TRY(hipMalloc(&out, words * 4));
  HIP_TRY(hipMemset(in, 0x5a, words * 4));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  KArgs<16> K;                         // any odd modulus will do: the instruction stream does not depend on the data
  memset(&K, 0, sizeof K);
  for (int i = 0; i < 16; i++) K.fp.p[i] = K.fp.one[i] = K.fp.r2[i] = K.fp.r3[i] = 0x9e3779b1u + 2u * (uint32_t) i;
  for (int i = 0; i < Limbs29<16>::L; i++) K.fp.p29[i] = (0x12345679u + 2u * (uint32_t) i) & Limbs29<16>::MASK;
  for (int i = 0; i < Inv30<16>::L; i++) K.fp.p30[i] = (0x2468ace1u + 2u * (uint32_t) i) & 0x3fffffffu;
  K.fp.ninv29 = 0x0badcafu; K.fp.qinv30 = 0x1234567u; K.fp.fbytes = 64; K.fp.pbits = 512;
  hipLaunchKernelGGL((mul_bench_kernel<16, V>), dim3(grid), dim3(256), 0, 0, out, in, iters / 8 + 1, K);
  HIP_TRY(hipEventRecord(e0, 0));
  hipLaunchKernelGGL((mul_bench_kernel<16, V>), dim3(grid), dim3(256), 0, 0, out, in, iters, K);
  HIP_TRY(hipEventRecord(e1, 0));
  HIP_TRY(hipEventSynchronize(e1));
  float ms;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  *rate = (double) grid * 256.0 * iters / (ms * 1e-3);
  *ms_out = ms;
  (void) hipFree(in);
  (void) hipFree(out);
  (void) hipEventDestroy(e0);
  (void) hipEventDestroy(e1);
  return 0;
}
extern "C" int pbc_hip_diag_mul_bench(int variant, int iters, int waves_per_simd, double *rate, double *ms) {
  if (waves_per_simd < 1 || waves_per_simd > 8) return fail("waves_per_simd must be 1..8");
  switch (variant) {
    case 1: return run_mul_bench<1>(iters, waves_per_simd, rate, ms);
    case 2: return run_mul_bench<2>(iters, waves_per_simd, rate, ms);
    case 3: return run_mul_bench<3>(iters, waves_per_simd, rate, ms);
    case 4: return run_mul_bench<4>(iters, waves_per_simd, rate, ms);
    case 5: return run_mul_bench<5>(iters, waves_per_simd, rate, ms);
    case 6: return run_mul_bench<6>(iters, waves_per_simd, rate, ms);
    case 7: return run_mul_bench<7>(iters, waves_per_simd, rate, ms);
    case 8: return run_mul_bench<8>(iters, waves_per_simd, rate, ms);
    case 9: return run_mul_bench<9>(iters, waves_per_simd, rate, ms);
    case 10: return run_mul_bench<10>(iters, waves_per_simd, rate, ms);
    default: return fail("unknown mul variant %d", variant);
  }
}

// variant -> lane-instructions per loop iteration (8 REPs x 8 instructions; V1/V10 count MACs)
extern "C" int pbc_hip_int_mac_peak(int variant, int iters, double *rate, double *ms) {
  switch (variant) {
    case 0: return run_probe<0>(iters, rate, ms, 64);
    case 1: return run_probe<1>(iters, rate, ms, 64);
    case 2: return run_probe<2>(iters, rate, ms, 64);
    case 3: return run_probe<3>(iters, rate, ms, 64);
    case 4: return run_probe<4>(iters, rate, ms, 64);
    case 5: return run_probe<5>(iters, rate, ms, 64);
    case 6: return run_probe<6>(iters, rate, ms, 64);
    case 7: return run_probe<7>(iters, rate, ms, 64);
    case 8: return run_probe<8>(iters, rate, ms, 64);
    case 9: return run_probe<9>(iters, rate, ms, 64);
    case 10: return run_probe<10>(iters, rate, ms, 64);
    case 11: return run_probe<11>(iters, rate, ms, 64);
    case 12: return run_probe<12>(iters, rate, ms, 64);
    case 13: return run_probe<13>(iters, rate, ms, 64);
    case 14: return run_probe<14>(iters, rate, ms, 64);
    case 15: return run_probe<15>(iters, rate, ms, 64);
    case 16: return run_probe<16>(iters, rate, ms, 64);
    case 17: return run_probe<17>(iters, rate, ms, 64);
    case 18: return run_probe<18>(iters, rate, ms, 64);
    default: return fail("unknown probe variant %d", variant);
  }
}

