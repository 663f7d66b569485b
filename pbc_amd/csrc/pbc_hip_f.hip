// pbc_hip_f.hip -- kernels and launches of type f (libpbc_hip.so; see host_common.h)
#include "host_common.h"
#include "pairing_fw.cuh"
#include "fw_sched.h"
#include "wave_kernels.cuh"

// Type F: one k-term product (k = 1: a single pairing) per lane.  With fb = fixed byte length of F_q:
// G1 2 fb, G2 4 fb, GT 12 fb bytes (40 / 80 / 240 B for f.param).
// (the 5-word field keeps its Miller accumulator in one 36 KB LDS area per workgroup: four workgroups per CU, two waves per
// SIMD; with PBC_F_AREAS=2 in two areas, one wave per SIMD and the register budget that goes with it)
template <int N, bool BM1, bool XS = false>
__global__ void __launch_bounds__(kBlock, N <= 5 ? (PBC_F_AREAS == 1 ? 2 : 1) : PBC_F_WAVES) f_prod_pairing_kernel(uint8_t *gt, const uint8_t *g1,
                                                                 const uint8_t *g2, size_t n, int k, unsigned *ctr, KArgs<N> ka) {
#ifdef PBC_F_WHATIF_TRACE                        // what-if builds only (tools/whatif_time.py --trace): per-wave start / end / HW_ID behind the results
  const uint64_t trace_t0 = wall_clock64();
#endif
  PBC_RESIDENT_LOOP(n, ctr) {
    size_t idx = PBC_UNIT_INDEX;
    size_t ld = idx < n ? idx : n - 1;
    const int fb = (int) fpk<N>().fbytes, L1 = 2 * fb, L2 = 4 * fb, LT = 12 * fb;
    __attribute__((aligned(4))) uint8_t out[48 * N];
    TypeF<N, BM1, XS>::f_prod_pairing_lane(out, g1 + ld * (k < 0 ? 1 : k) * L1, g2 + ld * (k < 0 ? 1 : k) * L2, k < 0 ? 1 : k, k < 0);
    if (idx < n) {
      uint32_t *dst = reinterpret_cast<uint32_t *>(gt + idx * LT);      // LT = 12 fb is a multiple of 4
      const uint32_t *src = reinterpret_cast<const uint32_t *>(out);
      for (int i = 0; i < LT / 4; i++) dst[i] = src[i];
    }
  }
#ifdef PBC_F_WHATIF_TRACE
  if ((threadIdx.x & 63) == 0) {
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    uint64_t *t = reinterpret_cast<uint64_t *>(gt + ((n * (size_t) (12 * fpk<N>().fbytes) + 255) & ~(size_t) 255)) + (size_t) (blockIdx.x * 2 + (threadIdx.x >> 6)) * 4;
    t[0] = trace_t0; t[1] = wall_clock64(); t[2] = hw; t[3] = xcc;
  }
#endif
}

template <int N>
__global__ void __launch_bounds__(kBlock) f_debug_kernel(int op, uint8_t *out, const uint8_t *a, const uint8_t *b, size_t n, KArgs<N> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const int LT = 12 * (int) fpk<N>().fbytes;
  __attribute__((aligned(4))) uint8_t o[48 * N];
  TypeF<N>::f_debug_lane(op, o, a + idx * LT, b + idx * LT);
  for (int i = 0; i < LT; i++) out[idx * LT + i] = o[i];
}

template <int N> __global__ void f_init_stage1(FConst *out, FRaw raw, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  TypeF<N>::init_stage1(out, raw, c_f);
}
template <int N> __global__ void f_init_stage2(FConst *out, FRaw raw, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  TypeF<N>::init_stage2(out, raw);
}
template <int N> __global__ void f_init_stage3(FConst *out, FRaw raw, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  TypeF<N>::init_stage3(out, raw);
}
template <int N> __global__ void f_init_stage4(FConst *out, FRaw raw, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  TypeF<N>::init_stage4(out, raw);
}

int derive_f(pbc_hip_pairing_s *P, hipStream_t s) {
  DevBuf buf;
  HIP_TRY(buf.alloc(sizeof(FConst)));
  FConst *dbuf = buf.as<FConst>();
  PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL(f_init_stage1<N>, dim3(1), dim3(64), 0, s, dbuf, P->fraw, kargs<N>(P)));
  HIP_TRY(hipMemcpyAsync(&P->fconst, dbuf, sizeof(FConst), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL(f_init_stage2<N>, dim3(1), dim3(64), 0, s, dbuf, P->fraw, kargs<N>(P)));
  HIP_TRY(hipMemcpyAsync(&P->fconst, dbuf, sizeof(FConst), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (P->fraw.e4bits > 0) {          // q = 3 mod 4: the i-basis copy for the pairing kernels
    PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL(f_init_stage3<N>, dim3(1), dim3(64), 0, s, dbuf, P->fraw, kargs<N>(P)));
    HIP_TRY(hipMemcpyAsync(&P->fconst_i, dbuf, sizeof(FConst), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    P->f_bm1 = P->fconst_i.bm1 != 0;
    if (P->f_bm1 && P->fraw.xs_try) {   // a sparse xi for the pairing kernels: the i-basis block rewritten for the basis X' = X / c
      PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL(f_init_stage4<N>, dim3(1), dim3(64), 0, s, dbuf, P->fraw, kargs<N>(P, true)));
      HIP_TRY(hipMemcpyAsync(&P->fconst_i, dbuf, sizeof(FConst), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// small batches on the five-word BN fields: one pairing per wavefront (wave_kernels.cuh, pairing_fw.cuh; the parameter file's own basis)
static constexpr size_t kFwMaxTerms = (size_t) 1 << 19;       // (records of the products' workspace: 320 bytes each)
static bool fw_capable(const pbc_hip_pairing_s *P) { return P->type == 'f' && P->nlimb == 5 && P->fconst.bn_ok; }
static auto fw_build(const pbc_hip_pairing_s *P) {
  return [P](WaveSched &S) {
    const FConst &C = P->fconst;
    return fw::build_schedules(S, C.rbits, wave_digit(C), (uint64_t) C.bn_x[0] | (uint64_t) C.bn_x[1] << 32, C.bn_xneg != 0);
  };
}
extern "C" size_t pbc_hip_diag_fw_schedule(pbc_hip_pairing_t *P, int which, uint64_t *out, size_t cap) {
  return P && fw_capable(P) ? wave_diag_schedule(wave_schedules(P->fw_sched, fw_build(P)), which, wave::SCHED_FINISH, out, cap) : 0;
}

int launch_f(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, hipStream_t s, ProdWs &W) {
  if (k >= 1 && fw_capable(P) && n <= P->f_wave_max && n * (size_t) k <= kFwMaxTerms) {
    // The throughput kernel runs a batch this small at the latency of ONE lane (7 ms a pairing, 5 ms more per further term of a
    // product): a wavefront per pairing -- per TERM for products, then one per product -- instead (pairing_fw.cuh)
    const WaveSched *S = nullptr;
    static const char kSchedKey = 0;
    const uint64_t *d_sched = wave_device_schedules(P, P->fw_sched, fw_build(P), &kSchedKey, &S);
    return d_sched ? wave_launch<FW, 5>(P, d_gt, d_g1, d_g2, n, k, s, W, d_sched, *S) : 1;
  }
  if (P->f_bm1 && P->fconst_i.xs_ok && P->nlimb == 5) {     // ... with a sparse xi
    hipLaunchKernelGGL((f_prod_pairing_kernel<5, true, true>), dim3(PBC_RGRID(f_prod_pairing_kernel<5, true, true>)), dim3(kBlock), 0, s, (uint8_t *) d_gt,
                       (const uint8_t *) d_g1, (const uint8_t *) d_g2, n, k, unit_counter(P, s), kargs<5>(P, true));
  } else if (P->f_bm1) {             // i-basis constants and the instantiation that goes with them
    PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL((f_prod_pairing_kernel<N, true>), dim3(PBC_RGRID(f_prod_pairing_kernel<N, true>)), dim3(kBlock), 0, s, (uint8_t *) d_gt,
                       (const uint8_t *) d_g1, (const uint8_t *) d_g2, n, k, unit_counter(P, s), kargs<N>(P, true)));
  } else {
    PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL((f_prod_pairing_kernel<N, false>), dim3(PBC_RGRID(f_prod_pairing_kernel<N, false>)), dim3(kBlock), 0, s, (uint8_t *) d_gt,
                       (const uint8_t *) d_g1, (const uint8_t *) d_g2, n, k, unit_counter(P, s), kargs<N>(P)));
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// diagnostics: Miller values before the final exponentiation; single F_q^12 operations
int diag_f_miller(pbc_hip_pairing_s *P, void *dt, const void *d1, const void *d2, size_t n) {
  unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL((f_prod_pairing_kernel<N, false>), dim3(grid), dim3(kBlock), 0, 0, (uint8_t *) dt,
                     (const uint8_t *) d1, (const uint8_t *) d2, n, -1, (unsigned *) nullptr, kargs<N>(P)));
  return 0;
}
int diag_f_op(pbc_hip_pairing_s *P, int stage, void *dt, const void *d1, const void *d2, size_t n) {
  unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  PBC_DISPATCH_F(P->nlimb, hipLaunchKernelGGL(f_debug_kernel<N>, dim3(grid), dim3(kBlock), 0, 0, stage, (uint8_t *) dt, (const uint8_t *) d1,
                     (const uint8_t *) d2, n, kargs<N>(P)));
  return 0;
}
