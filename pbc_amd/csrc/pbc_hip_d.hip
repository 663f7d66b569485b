// pbc_hip_d.hip -- kernels and launches of types d and g (libpbc_hip.so; see host_common.h)
#include "host_common.h"
#include "pairing_dw.cuh"
#include "dw_sched.h"
#include "pairing_gw.cuh"
#include "gw_sched.h"
#include "wave_kernels.cuh"

// Types D and G: one k-term product (k = 1: a single pairing) per lane.  With fb = fixed byte length
// of F_q and d = k/2, G1 records are 2 fb, G2 and GT 2 d fb bytes (40 / 120 / 120 B for d159.param,
// 38 / 190 / 190 B for g149.param).
template <int N, int DEG>
static __device__ __forceinline__ void d_prod_unit(size_t idx, uint8_t *gt, const uint8_t *g1, const uint8_t *g2, size_t n, int k, uint32_t *ws) {
  size_t ld = idx < n ? idx : n - 1;
  const int fb = (int) fpk<N>().fbytes, L1 = 2 * fb, L2 = 2 * DEG * fb, LT = 2 * DEG * fb;
  __attribute__((aligned(4))) uint8_t out[8 * DEG * N];
  TypeMNT<N, DEG>::d_prod_pairing_lane(out, g1 + ld * k * L1, g2 + ld * k * L2, k,
                                       ws + (size_t) blockIdx.x * (size_t) k * (TypeMNT<N, DEG>::DL_WORDS * kBlock) + threadIdx.x);
  if (idx < n) {
    if ((LT & 3) == 0) {
      uint32_t *dst = reinterpret_cast<uint32_t *>(gt + idx * LT);
      const uint32_t *src = reinterpret_cast<const uint32_t *>(out);
      for (int i = 0; i < LT / 4; i++) dst[i] = src[i];
    } else {
      for (int i = 0; i < LT; i++) gt[idx * LT + i] = out[i];
    }
  }
}
// (resident workgroups where they pay: kDResident, pairing_d.cuh)
template <int N, int DEG>
__global__ void __launch_bounds__(kBlock, PBC_DF_WAVES) d_prod_pairing_kernel(uint8_t *gt, const uint8_t *g1,
                                                                 const uint8_t *g2, size_t n, int k, uint32_t *ws, unsigned *ctr, KArgs<N> ka) {
  if constexpr (kDResident<N, DEG>) {
    PBC_RESIDENT_LOOP(n, ctr) d_prod_unit<N, DEG>(PBC_UNIT_INDEX, gt, g1, g2, n, k, ws);
  } else {
    d_prod_unit<N, DEG>((size_t) blockIdx.x * kBlock + threadIdx.x, gt, g1, g2, n, k, ws);
  }
}

// small batches: one pairing per wavefront (wave_kernels.cuh) -- type d on the five-, six- and seven-word d = 3 fields (six, seven
// and eight limbs: the level programs do not know the field; pairing_dw.cuh), type g on the five-word field (pairing_gw.cuh)
static constexpr size_t kDwMaxTerms = (size_t) 1 << 20;       // (records of the products' workspace: 160 bytes each)
static bool dw_capable(const pbc_hip_pairing_s *P) { return P->type == 'd' && P->nlimb >= 5 && P->nlimb <= 7 && P->deg == 3; }
static bool gw_capable(const pbc_hip_pairing_s *P) { return P->type == 'g' && P->nlimb == 5 && P->deg == 5; }
#define PBC_DISPATCH_DW(P, ...) do { if ((P)->nlimb == 5) { constexpr int N = 5; __VA_ARGS__; } else if ((P)->nlimb == 6) { constexpr int N = 6; __VA_ARGS__; } \
                                     else { constexpr int N = 7; __VA_ARGS__; } } while (0)
static auto dw_build(const pbc_hip_pairing_s *P) {
  return [P](WaveSched &S) { const DConst &C = P->dconst; return dw::build_schedules(S, C.rbits, wave_digit(C), C.phik, C.phikbits); };
}
static auto gw_build(const pbc_hip_pairing_s *P) {
  return [P](WaveSched &S) { const DConst &C = P->dconst; return gw::build_schedules(S, C.rbits, wave_digit(C), C.phik, C.phikbits); };
}
static const uint64_t *dw_device_schedules(pbc_hip_pairing_s *P, const WaveSched **host) {
  static const char kSchedKey = 0;
  return wave_device_schedules(P, P->dw_sched, dw_build(P), &kSchedKey, host);
}
static const uint64_t *gw_device_schedules(pbc_hip_pairing_s *P, const WaveSched **host) {
  static const char kSchedKey = 0;
  return wave_device_schedules(P, P->gw_sched, gw_build(P), &kSchedKey, host);
}
extern "C" size_t pbc_hip_diag_dw_schedule(pbc_hip_pairing_t *P, int which, uint64_t *out, size_t cap) {
  return P && dw_capable(P) ? wave_diag_schedule(wave_schedules(P->dw_sched, dw_build(P)), which, wave::SCHED_PP, out, cap) : 0;
}
extern "C" size_t pbc_hip_diag_gw_schedule(pbc_hip_pairing_t *P, int which, uint64_t *out, size_t cap) {
  return P && gw_capable(P) ? wave_diag_schedule(wave_schedules(P->gw_sched, gw_build(P)), which, wave::SCHED_PP, out, cap) : 0;
}

// pairing_pp for types d / g: single-lane table derivation, then one second argument per lane
template <int N, int DEG>
__global__ void d_pp_init_kernel(uint32_t *tab, uint32_t *valid, const uint8_t *g1, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  *valid = TypeMNT<N, DEG>::d_pp_init_lane(tab, g1) ? 1u : 0u;
}
template <int N, int DEG>
static __device__ __forceinline__ void d_pp_unit(size_t idx, uint8_t *gt, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ valid,
                                                 const uint8_t *g2, size_t n) {
  size_t ld = idx < n ? idx : n - 1;
  const int fb = (int) fpk<N>().fbytes, L2 = 2 * DEG * fb, LT = 2 * DEG * fb;
  __attribute__((aligned(4))) uint8_t out[8 * DEG * N];
  TypeMNT<N, DEG>::d_pp_apply_lane(out, tab, *valid != 0, g2 + ld * L2);
  if (idx < n) {
    if ((LT & 3) == 0) {
      uint32_t *dst = reinterpret_cast<uint32_t *>(gt + idx * LT);
      const uint32_t *src = reinterpret_cast<const uint32_t *>(out);
      for (int i = 0; i < LT / 4; i++) dst[i] = src[i];
    } else {
      for (int i = 0; i < LT; i++) gt[idx * LT + i] = out[i];
    }
  }
}
template <int N, int DEG>
__global__ void __launch_bounds__(kBlock, PBC_DF_WAVES) d_pp_apply_kernel(uint8_t *gt, const uint32_t *__restrict__ tab,
                                                                          const uint32_t *__restrict__ valid,
                                                                          const uint8_t *g2, size_t n, unsigned *ctr, KArgs<N> ka) {
  if constexpr (kDResident<N, DEG>) {
    PBC_RESIDENT_LOOP(n, ctr) d_pp_unit<N, DEG>(PBC_UNIT_INDEX, gt, tab, valid, g2, n);
  } else {
    d_pp_unit<N, DEG>((size_t) blockIdx.x * kBlock + threadIdx.x, gt, tab, valid, g2, n);
  }
}

// Table sets (pbc_hip_pairing_pp_set_*; host side: pbc_hip_ppset.hip): every table in one launch, one first argument per
// lane (the lane's LDS state is sized for 128-lane workgroups); table t = tabs + t tab_words, the words d_pp_init_kernel writes
template <int N, int DEG>
__global__ void __launch_bounds__(kBlock) d_pp_set_init_kernel(uint32_t *tabs, uint32_t *flags, const uint8_t *g1, size_t m, size_t tab_words, KArgs<N> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= m) return;
  flags[idx] = TypeMNT<N, DEG>::d_pp_init_lane(tabs + idx * tab_words, g1 + idx * 2 * (size_t) fpk<N>().fbytes) ? 1u : 0u;
}
// d_pp_unit on the wave slot `slot` of a plan (pp_set_plan.h, host_common.h PpSlot): the slot's table is wave-uniform
template <int N, int DEG>
static __device__ __forceinline__ void d_pp_set_unit(size_t slot, uint8_t *gt, const uint32_t *__restrict__ tabs, const uint32_t *__restrict__ flags, size_t tab_words,
                                                     const uint8_t *g2, const uint64_t *__restrict__ plan, size_t stride, size_t tmul) {
  const PpSlot sl = pp_set_slot(plan, slot);
  const size_t rec = sl.rec(stride, tmul);
  const int fb = (int) fpk<N>().fbytes, L2 = 2 * DEG * fb, LT = 2 * DEG * fb;
  __attribute__((aligned(4))) uint8_t out[8 * DEG * N];
  TypeMNT<N, DEG>::d_pp_apply_lane(out, tabs + sl.table * tab_words, flags[sl.table] != 0, g2 + rec * L2);
  if (sl.live()) {
    if ((LT & 3) == 0) {
      uint32_t *dst = reinterpret_cast<uint32_t *>(gt + rec * LT);
      const uint32_t *src = reinterpret_cast<const uint32_t *>(out);
      for (int i = 0; i < LT / 4; i++) dst[i] = src[i];
    } else {
      for (int i = 0; i < LT; i++) gt[rec * LT + i] = out[i];
    }
  }
}
template <int N, int DEG>
__global__ void __launch_bounds__(kBlock, PBC_DF_WAVES) d_pp_set_apply_kernel(uint8_t *gt, const uint32_t *__restrict__ tabs, const uint32_t *__restrict__ flags,
                                                                              size_t tab_words, const uint8_t *g2, const uint64_t *__restrict__ plan, size_t slots,
                                                                              size_t stride, size_t tmul, unsigned *ctr, KArgs<N> ka) {
  if constexpr (kDResident<N, DEG>) {
    PBC_RESIDENT_LOOP(slots * 64, ctr) d_pp_set_unit<N, DEG>(vb, gt, tabs, flags, tab_words, g2, plan, stride, tmul);
  } else {
    const size_t slot = (size_t) blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (slot < slots) d_pp_set_unit<N, DEG>(slot, gt, tabs, flags, tab_words, g2, plan, stride, tmul);
  }
}

template <int N, int DEG> __global__ void d_init_stage1(DConst *out, DRaw raw, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  TypeMNT<N, DEG>::init_stage1(out, raw, c_d);
}
template <int N, int DEG> __global__ void d_init_stage2(DConst *out, DRaw raw, KArgs<N> ka) {
  if (threadIdx.x || blockIdx.x) return;
  TypeMNT<N, DEG>::init_stage2(out, raw);
}

int derive_d(pbc_hip_pairing_s *P, hipStream_t s) {
  DevBuf buf;
  HIP_TRY(buf.alloc(sizeof(DConst)));
  DConst *dbuf = buf.as<DConst>();
  PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_init_stage1<N, DEG>), dim3(1), dim3(64), 0, s, dbuf, P->draw, kargs<N>(P)));
  HIP_TRY(hipMemcpyAsync(&P->dconst, dbuf, sizeof(DConst), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_init_stage2<N, DEG>), dim3(1), dim3(64), 0, s, dbuf, P->draw, kargs<N>(P)));
  HIP_TRY(hipMemcpyAsync(&P->dconst, dbuf, sizeof(DConst), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  return 0;
}

int launch_d(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, hipStream_t s, ProdWs &W) {
  unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  // The throughput kernel runs a batch this small at the latency of ONE lane (3.9 ms a pairing, ~2.9 ms more per further term
  // of a product): a wavefront per pairing -- per TERM for products, then one per product -- instead (pairing_dw.cuh).
  // type g: 14.5 ms a pairing on one lane whatever the batch size (+ 6.5 ms per further term of a product); a wavefront per pairing
  // -- per TERM for products, then one per product -- instead (the schedules: kept with the object).  Saturated, the wavefronts
  // finish 430 k pairings or 540 k terms a second: products of many terms reach the lane kernel's time a little earlier
  // (measured: 4 terms ~4600 products, 16 terms ~3800).
  const size_t gw_max = k <= 2 ? P->d_wave_max : (size_t) ((double) P->d_wave_max * (0.7 + 0.8 / k));
  if (gw_capable(P) && k >= 1 && n <= gw_max && n * (size_t) k <= kDwMaxTerms) {
    const WaveSched *S = nullptr;
    const uint64_t *d_sched = gw_device_schedules(P, &S);
    return d_sched ? wave_launch<GW, 5>(P, d_gt, d_g1, d_g2, n, k, s, W, d_sched, *S) : 1;
  }
  if (dw_capable(P) && k >= 1 && n <= P->d_wave_max && n * (size_t) k <= kDwMaxTerms) {
    const WaveSched *S = nullptr;
    const uint64_t *d_sched = dw_device_schedules(P, &S);
    if (!d_sched) return 1;
    PBC_DISPATCH_DW(P, return (wave_launch<DW, N, DW<7>>(P, d_gt, d_g1, d_g2, n, k, s, W, d_sched, *S)));      // (one record size, the largest, for every field)
  }
  if (k == 1) {
    PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_prod_pairing_kernel<N, DEG>), dim3(kDResident<N, DEG> ? PBC_RGRID(d_prod_pairing_kernel<N, DEG>) : grid), dim3(kBlock), 0, s, (uint8_t *) d_gt,
                                                (const uint8_t *) d_g1, (const uint8_t *) d_g2, n, 1, (uint32_t *) nullptr, kDResident<N, DEG> ? unit_counter(P, s) : nullptr, kargs<N>(P)));
  } else {
    size_t rec = 0;                    // words of Miller state per term and lane (the kernel's own constant)
    // (5-word field: products keep one workgroup per 128 units -- the resident shape measured 160 -> 185 ms on 16-term
    // products -- and run without the time-sliced priorities that go with it)
    bool res = false;
    PBC_DISPATCH_D(P, { rec = (size_t) TypeMNT<N, DEG>::DL_WORDS; res = kDResident<N, DEG> && N != 5; if (res) grid = PBC_RGRID(d_prod_pairing_kernel<N, DEG>); });      // one workspace record per RESIDENT workgroup
    void *ws = W.get((size_t) grid * (size_t) k * rec * kBlock * sizeof(uint32_t));
    if (!ws) return 1;
    PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_prod_pairing_kernel<N, DEG>), dim3(grid), dim3(kBlock), 0, s, (uint8_t *) d_gt,
                                                (const uint8_t *) d_g1, (const uint8_t *) d_g2, n, k, (uint32_t *) ws, res ? unit_counter(P, s) : nullptr, kargs<N>(P, false, !res)));
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int pp_init_launch_d(pbc_hip_pairing_s *P, pbc_hip_pp_s *pp, const uint8_t *dg1) {
  PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_pp_init_kernel<N, DEG>), dim3(1), dim3(64), 0, 0, pp->tab, pp->valid, dg1, kargs<N>(P)));
  return 0;
}
int pp_apply_launch_d(pbc_hip_pp_s *pp, void *d_gt, const void *d_g2, size_t n, hipStream_t s) {
  pbc_hip_pairing_s *P = pp->P;
  unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  if (gw_capable(P) && n <= P->d_wave_max) {
    const WaveSched *S = nullptr;
    const uint64_t *d_sched = gw_device_schedules(P, &S);
    return d_sched ? wave_pp_launch<GW, 5>(pp, d_gt, d_g2, n, s, d_sched, *S) : 1;
  }
  if (dw_capable(P) && n <= P->d_wave_max) {
    const WaveSched *S = nullptr;
    const uint64_t *d_sched = dw_device_schedules(P, &S);
    if (!d_sched) return 1;
    PBC_DISPATCH_DW(P, return (wave_pp_launch<DW, N>(pp, d_gt, d_g2, n, s, d_sched, *S)));
  }
  PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_pp_apply_kernel<N, DEG>), dim3(kDResident<N, DEG> ? PBC_RGRID(d_pp_apply_kernel<N, DEG>) : grid), dim3(kBlock), 0, s, (uint8_t *) d_gt,
                                           pp->tab, pp->valid, (const uint8_t *) d_g2, n, kDResident<N, DEG> ? unit_counter(P, s) : nullptr, kargs<N>(P)));
  HIP_TRY(hipGetLastError());
  return 0;
}

int pp_set_init_launch_d(pbc_hip_pairing_s *P, pbc_hip_pp_set_s *set, hipStream_t s) {
  PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_pp_set_init_kernel<N, DEG>), dim3((unsigned) ((set->m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, set->tabs, set->flags,
                                       (const uint8_t *) set->g1, set->m, set->tab_words, kargs<N>(P)));
  HIP_TRY(hipGetLastError());
  return 0;
}
// every batch size on the lane kernel (the wave kernels serve one table per launch: DESIGN.md 4.6)
int pp_set_apply_launch_d(pbc_hip_pp_set_s *set, void *d_out, const void *d_g2, const uint64_t *d_plan, size_t slots, size_t stride, size_t tmul, hipStream_t s) {
  pbc_hip_pairing_s *P = set->P;
  const size_t n = slots * 64;         // (the unit range of the resident loop: PBC_RGRID)
  PBC_DISPATCH_D(P, hipLaunchKernelGGL((d_pp_set_apply_kernel<N, DEG>), dim3(kDResident<N, DEG> ? PBC_RGRID(d_pp_set_apply_kernel<N, DEG>) : (unsigned) ((slots + 1) / 2)),
                                       dim3(kBlock), 0, s, (uint8_t *) d_out, (const uint32_t *) set->tabs, (const uint32_t *) set->flags, set->tab_words,
                                       (const uint8_t *) d_g2, d_plan, slots, stride, tmul, kDResident<N, DEG> ? unit_counter(P, s) : nullptr, kargs<N>(P)));
  HIP_TRY(hipGetLastError());
  return 0;
}
