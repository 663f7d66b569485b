// wave_kernels.cuh -- the kernels and the host plumbing of the one-pairing-per-wavefront routes (wave_vm.cuh), once for every
// family (F = DW, FW, GW: pairing_dw.cuh, pairing_fw.cuh, pairing_gw.cuh): one wavefront per workgroup, record offsets from
// the family's wire counts; the schedules of an object, built on first use and uploaded once per device; the launches.
#pragma once
#include "host_common.h"
#include "wave_vm.cuh"

// element_pairing
template <template <int> class F, int N>
__global__ void __launch_bounds__(64) wave_pairing_kernel(uint8_t *gt, const uint8_t *g1, const uint8_t *g2, size_t n, const uint64_t *sched, KArgs<N> ka) {
  const size_t idx = blockIdx.x;
  if (idx >= n) return;
  const size_t fb = fpk<N>().fbytes;
  F<N>::VM::template pairing<F<N>>(gt + idx * F<N>::kGT * fb, g1 + idx * F<N>::kG1 * fb, g2 + idx * F<N>::kG2 * fb, sched);
}
// element_prod_pairing on wavefronts: the Miller value of every TERM (n k wavefronts), then one wavefront per product
template <template <int> class F, int N>
__global__ void __launch_bounds__(64) wave_miller_kernel(uint32_t *recs, const uint8_t *g1, const uint8_t *g2, size_t terms, const uint64_t *sched, KArgs<N> ka) {
  const size_t idx = blockIdx.x;
  if (idx >= terms) return;
  const size_t fb = fpk<N>().fbytes;
  F<N>::VM::template miller_term<F<N>>(recs + idx * F<N>::VM::rec_words(F<N>::kCoef), g1 + idx * F<N>::kG1 * fb, g2 + idx * F<N>::kG2 * fb, sched);
}
template <template <int> class F, int N>
__global__ void __launch_bounds__(64) wave_finish_kernel(uint8_t *gt, const uint32_t *recs, size_t n, int k, const uint64_t *sched, KArgs<N> ka) {
  const size_t idx = blockIdx.x;
  if (idx >= n) return;
  F<N>::VM::template finish<F<N>>(gt + idx * F<N>::kGT * fpk<N>().fbytes, recs + idx * (size_t) k * F<N>::VM::rec_words(F<N>::kCoef), k, sched);
}
// pairing_pp_apply on wavefronts
template <template <int> class F, int N>
__global__ void __launch_bounds__(64) wave_pp_apply_kernel(uint8_t *gt, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ valid, const uint8_t *g2,
                                                           size_t n, const uint64_t *sched, KArgs<N> ka) {
  const size_t idx = blockIdx.x;
  if (idx >= n) return;
  const size_t fb = fpk<N>().fbytes;
  F<N>::VM::template pp_apply<F<N>>(gt + idx * F<N>::kGT * fb, tab, *valid != 0, g2 + idx * F<N>::kG2 * fb, sched);
}

// the signed digit of r at position m (r = C.r - C.rm, both non-negative: DConst, FConst), as the schedule builders ask for it
template <class Const>
static auto wave_digit(const Const &C) {
  return [&C](int m) { return (int) ((C.r[m >> 5] >> (m & 31)) & 1) - (int) ((C.rm[m >> 5] >> (m & 31)) & 1); };
}
// The schedules for this object's curve ({dw,fw,gw}_sched.h), built on first use and kept with the object (S: its member).
// build(S) -> false: the tables lack a program; the schedules stay empty and every caller fails.
inline std::mutex &wave_schedules_mutex() { static std::mutex mu; return mu; }     // one for the library: first uses are rare
template <class Build>
static const WaveSched &wave_schedules(WaveSched &S, const Build &build) {
  std::lock_guard<std::mutex> lk(wave_schedules_mutex());
  if (S.e.empty() && !build(S)) S.e.clear();
  return S;
}
// ... and on the device (24 to 50 KB, read-only, one copy per device the object runs on -- uploaded on first use, kept with the
// object under `key`); nullptr: no schedules
template <class Build>
static const uint64_t *wave_device_schedules(pbc_hip_pairing_s *P, WaveSched &member, const Build &build, const void *key, const WaveSched **host) {
  const WaveSched &S = wave_schedules(member, build);
  if (S.e.empty()) return nullptr;
  bool fresh = false;
  uint64_t *d_sched = (uint64_t *) object_scratch(P, key, S.e.size() * sizeof(uint64_t), &fresh);
  if (!d_sched) return nullptr;
  if (fresh && hipMemcpy(d_sched, S.e.data(), S.e.size() * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  *host = &S;
  return d_sched;
}
// pbc_hip_diag_{dw,fw,gw}_schedule: schedule `which` (0 .. last) of S
static size_t wave_diag_schedule(const WaveSched &S, int which, int last, uint64_t *out, size_t cap) {
  if (which < 0 || which > last || S.e.empty()) return 0;
  const size_t first = S.off[which], end = which < 3 ? S.off[which + 1] : S.e.size();
  for (size_t i = first; i < end && i - first < cap; i++) out[i - first] = S.e[i];
  return end - first;
}
// n products of k pairings each: k = 1 one wavefront per pairing; else one per TERM, then one per product.  FREC: the family
// whose record sizes the workspace request.
template <template <int> class F, int N, class FREC = F<N>>
static int wave_launch(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, hipStream_t s, ProdWs &W, const uint64_t *d_sched, const WaveSched &S) {
  if (k == 1) {
    hipLaunchKernelGGL((wave_pairing_kernel<F, N>), dim3((unsigned) n), dim3(64), 0, s, (uint8_t *) d_gt, (const uint8_t *) d_g1, (const uint8_t *) d_g2, n, d_sched + S.off[wave::SCHED_PAIRING], kargs<N>(P));
  } else {
    const size_t terms = n * (size_t) k;
    uint32_t *recs = (uint32_t *) W.get(terms * FREC::VM::rec_words(FREC::kCoef) * sizeof(uint32_t));
    if (!recs) return 1;
    hipLaunchKernelGGL((wave_miller_kernel<F, N>), dim3((unsigned) terms), dim3(64), 0, s, recs, (const uint8_t *) d_g1, (const uint8_t *) d_g2, terms, d_sched + S.off[wave::SCHED_MILLER], kargs<N>(P));
    hipLaunchKernelGGL((wave_finish_kernel<F, N>), dim3((unsigned) n), dim3(64), 0, s, (uint8_t *) d_gt, (const uint32_t *) recs, n, k, d_sched + S.off[wave::SCHED_FINISH], kargs<N>(P));
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
template <template <int> class F, int N>
static int wave_pp_launch(pbc_hip_pp_s *pp, void *d_gt, const void *d_g2, size_t n, hipStream_t s, const uint64_t *d_sched, const WaveSched &S) {
  if (S.lines > wave::kMaxLines) return 1;
  hipLaunchKernelGGL((wave_pp_apply_kernel<F, N>), dim3((unsigned) n), dim3(64), 0, s, (uint8_t *) d_gt, (const uint32_t *) pp->tab, (const uint32_t *) pp->valid, (const uint8_t *) d_g2, n,
                     d_sched + S.off[wave::SCHED_PP], kargs<N>(pp->P));
  HIP_TRY(hipGetLastError());
  return 0;
}
