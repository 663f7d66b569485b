// pbc_hip_mpz.hip -- kernels and C-ABI entry points of element_mul_mpz / element_pow_mpz with one integer for the batch
// (group_mpz.cuh, mpz_plan.h; include/pbc_hip.h pbc_hip_element_mul_mpz_batch): libpbc_hip.so; see host_common.h
#include "host_common.h"
#include "group_mpz.cuh"
#include "mpz_plan.h"

// dig: the digit string of the call (device, read-only for the kernel: the lanes read it on the scalar unit), nd: its
// length -- the loop bound is this ARGUMENT, never something found in the buffer.
// G1 / G2 over a field policy: the fast lane writes the results it can finish and a flag per unit; the complete lane
// writes the flagged units (flags == null: every unit -- "hip_group_slow 1")
template <class F, int W>
__global__ void __launch_bounds__(kBlock, 2) ec_mpz_fast_kernel(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd, uint8_t *flags, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = 2 * (size_t) F::bytes();
  flags[idx] = ec_mpz_fast_lane<F, W>(out + idx * L, in + idx * L, dig, nd) ? 0 : 1;
}
template <class F>
__global__ void __launch_bounds__(kBlock, 2) ec_mpz_complete_kernel(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd, int w, const uint8_t *flags, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  if (flags && !flags[idx]) return;
  const size_t L = 2 * (size_t) F::bytes();
  ec_mpz_complete_lane<F>(out + idx * L, in + idx * L, dig, nd, w);
}
// G1 of the 5-word fields (d159.param, f.param): the fast lane in limb form (group_l5.cuh), as l5_gmul_kernel
template <class KP, int W>
__global__ void __launch_bounds__(kBlock, 2) l5_mpz_kernel(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd, uint8_t *flags, size_t n, KArgs<5> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = 2 * (size_t) fpk<5>().fbytes;
  flags[idx] = MpzL5<KP>::template fast_lane<W>(out + idx * L, in + idx * L, dig, nd) ? 0 : 1;
}
// Type a, 512-bit field: the limb-form lanes, resident workgroups as the ladder of element_mul_zn (al_gmul_kernel).
// W = 0: the Lucas lane on GT records instead of the point lane (both records are 8 N bytes)
template <int N, int W>
__global__ void __launch_bounds__(kBlock, PBC_A_WAVES) al_mpz_kernel(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd, uint8_t *flags, size_t n, unsigned *ctr, KArgs<N> ka) {
  PBC_RESIDENT_LOOP(n, ctr) {
    size_t idx = PBC_UNIT_INDEX;
    size_t ld = idx < n ? idx : n - 1;
    constexpr int L = 8 * N;
    __attribute__((aligned(16))) uint8_t o[L];
    bool ok;
    if constexpr (W == 0) ok = MpzAL<N>::gt_fast_lane(o, in + ld * L, dig, nd);
    else ok = MpzAL<N>::template fast_lane<W>(o, in + ld * L, dig, nd);
    if (idx < n) {
      flags[idx] = ok ? 0 : 1;
      if (ok) {
        uint4 *dst = reinterpret_cast<uint4 *>(out + idx * L);
        const uint4 *src = reinterpret_cast<const uint4 *>(o);
#pragma unroll
        for (int i = 0; i < L / 16; i++) dst[i] = src[i];
      }
    }
  }
}
// GT of type f (5-word fields): the cyclotomic lane of element_pow_zn (group_ops.cuh f_gt_pow_cyc_lane) on ONE Z_r record
// that every lane reads -- zr: the record of k behind the digits; elements outside the cyclotomic subgroup are flagged
// for gt_mpz_kernel (f_gtpow_kernel with a uniform scalar)
template <int N, bool BM1, bool XS>
__global__ void __launch_bounds__(kBlock, 2) f_mpz_gtpow_kernel(uint8_t *out, const uint8_t *a, const uint8_t *zr, int zlen, uint8_t *flags, size_t n, KArgs<N> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  size_t ld = idx < n ? idx : n - 1;
  const int LT = 12 * (int) fpk<N>().fbytes;
  __attribute__((aligned(4))) uint8_t o[48 * N];
  const bool ok = f_gt_pow_cyc_lane<TypeF<N, BM1, XS>>(o, a + ld * LT, zr, zlen);
  if (idx < n) {
    flags[idx] = ok ? 0 : 1;
    if (ok) {
      uint32_t *dst = reinterpret_cast<uint32_t *>(out + idx * LT);
      const uint32_t *src = reinterpret_cast<const uint32_t *>(o);
      for (int i = 0; i < LT / 4; i++) dst[i] = src[i];
    }
  }
}
// GT over a field policy: x^k for any field element (flags != null: the lanes the Lucas / cyclotomic lane reported)
template <class G>
__global__ void __launch_bounds__(kBlock, 2) gt_mpz_kernel(uint8_t *out, const uint8_t *in, const uint32_t *dig, int nd, const uint8_t *flags, size_t n, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  if (flags && !flags[idx]) return;
  gt_mpz_lane<G>(out + idx * (size_t) G::bytes(), in + idx * (size_t) G::bytes(), dig, nd);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static bool symmetric(const pbc_hip_pairing_s *P) { return P->type == 'a' || P->type == '1' || P->type == 'e'; }
// F = the field policy of group 1 / 2: F_q for G1 and the G2 of the symmetric types, the twist's field otherwise
#define PBC_DISPATCH_MPZ(P_, group_, ...)                                                      \
  do {                                                                                         \
    if ((group_) == 2 && !symmetric(P_)) PBC_DISPATCH_TWIST(P_, __VA_ARGS__);                  \
    else { PBC_DISPATCH_N((P_)->nlimb, { typedef FqOps<N> F; __VA_ARGS__; }); }                \
  } while (0)
#define PBC_DISPATCH_MPZ_GT(P_, ...)                                                           \
  do {                                                                                         \
    if ((P_)->type == 'a' || (P_)->type == '1') { if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if ((P_)->type == 'e') { if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if ((P_)->type == 'f') { PBC_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); } \
    else { PBC_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                      \
  } while (0)

// the digits of a call and their width (mpz_plan.h mpz_recode: GT the bits; points the plain or the width-4 NAF, by k)
static int mpz_recode(int group, const uint8_t *k, size_t klen, std::vector<int8_t> &digits) {
  return pbc_host::mpz_recode(group == 3, k, klen, digits);
}

// One call's digits on their way to the device: the second buffer of the (device, stream) workspace, ONE stream-ordered
// copy from the workspace's page-locked staging -- behind the kernels of an earlier call on this stream, which still
// read THEIR digits from the same bytes; the staging is not rewritten before this copy has been made (stage_acquire
// waits for the event recorded behind the previous one).  The plan of a table set travels the same way.
// `rec` (may be empty): bytes that travel behind the digits, at the next 16-byte boundary (*rec_at)
const uint32_t *digits_upload(ProdWs &W, const std::vector<int8_t> &dig, const std::vector<uint8_t> &rec, const uint8_t **rec_at, hipStream_t s) {
  const size_t off = (dig.size() + 16) & ~(size_t) 15;       // whole words, at least one
  const size_t bytes = off + ((rec.size() + 3) & ~(size_t) 3);
  uint8_t *buf = (uint8_t *) W.get2(bytes);
  if (!buf) return nullptr;
  HostStage *hs = W.stage();
  if (!hs) { fail("internal: no staging for the digits"); return nullptr; }
  uint8_t *h = (uint8_t *) stage_acquire(*hs, bytes);
  if (!h) return nullptr;
  memset(h, 0, bytes);
  if (!dig.empty()) memcpy(h, dig.data(), dig.size());
  if (!rec.empty()) memcpy(h + off, rec.data(), rec.size());
  *rec_at = buf + off;
  if (hipMemcpyAsync(buf, h, bytes, hipMemcpyHostToDevice, s) != hipSuccess) { fail("uploading the digits failed"); return nullptr; }
  if (stage_copied(*hs, s)) return nullptr;
  return (const uint32_t *) buf;
}

// enqueue n units on stream s (device pointers); `own`: the workspace of a host-path stream, else the object's table entry
// of (device, stream), pinned with its issue lock until the kernels are enqueued (ProdWs)
static int mpz_launch(pbc_hip_pairing_s *P, int group, void *d_out, const void *d_in, const std::vector<int8_t> &digits, int w, size_t n,
                      hipStream_t s, const OwnWs *own) {
  if (!n) return 0;
  uint8_t *out = (uint8_t *) d_out;
  const uint8_t *in = (const uint8_t *) d_in;
  const unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  const int nd = (int) digits.size();
  const bool fast_a = P->type == 'a' && !P->a_generic && !P->group_slow;
  // GT of type f: k as a Z_r record for the cyclotomic lane, where it fits and pays (mpz_plan.h mpz_gt_wants_record)
  const bool cyc_f = group == 3 && P->type == 'f' && P->nlimb == 5 && !P->group_slow && pbc_host::mpz_gt_wants_record(digits, (size_t) P->len_zr);
  std::vector<uint8_t> rec;
  if (cyc_f) {
    rec.assign((size_t) P->len_zr, 0);
    for (int i = 0; i < nd; i++) if (digits[(size_t) i]) rec[rec.size() - 1 - (size_t) (i >> 3)] |= (uint8_t) (1u << (i & 7));
  }
  ProdWs W(P, s, own);
  const uint8_t *zr = nullptr;
  const uint32_t *dig = digits_upload(W, digits, rec, &zr, s);
  if (!dig) return 1;
  uint8_t *flags = nullptr;
  if (!P->group_slow && (group != 3 || fast_a || cyc_f)) {
    flags = (uint8_t *) W.get(n);
    if (!flags) return 1;
  }
  if (group == 3) {
    if (fast_a)
      hipLaunchKernelGGL((al_mpz_kernel<16, 0>), dim3(PBC_RGRID(al_mpz_kernel<16, 0>)), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, unit_counter(P, s), kargs<16>(P));
    if (cyc_f) {                       // (the instantiation the object's pairing kernels use, as element_pow_zn chooses it)
      if (P->f_bm1 && P->fconst_i.xs_ok)
        hipLaunchKernelGGL((f_mpz_gtpow_kernel<5, true, true>), dim3(grid), dim3(kBlock), 0, s, out, in, zr, P->len_zr, flags, n, kargs<5>(P, true));
      else if (P->f_bm1)
        hipLaunchKernelGGL((f_mpz_gtpow_kernel<5, true, false>), dim3(grid), dim3(kBlock), 0, s, out, in, zr, P->len_zr, flags, n, kargs<5>(P, true));
      else
        hipLaunchKernelGGL((f_mpz_gtpow_kernel<5, false, false>), dim3(grid), dim3(kBlock), 0, s, out, in, zr, P->len_zr, flags, n, kargs<5>(P));
    }
    PBC_DISPATCH_MPZ_GT(P, hipLaunchKernelGGL(gt_mpz_kernel<G>, dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, (const uint8_t *) flags, n, kargs<G::NW>(P)));
  } else if (fast_a) {
    if (w == 2) hipLaunchKernelGGL((al_mpz_kernel<16, 2>), dim3(PBC_RGRID(al_mpz_kernel<16, 2>)), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, unit_counter(P, s), kargs<16>(P));
    else hipLaunchKernelGGL((al_mpz_kernel<16, 4>), dim3(PBC_RGRID(al_mpz_kernel<16, 4>)), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, unit_counter(P, s), kargs<16>(P));
    hipLaunchKernelGGL(ec_mpz_complete_kernel<FqOps<16>>, dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, w, (const uint8_t *) flags, n, kargs<16>(P));
  } else if (flags && group == 1 && P->nlimb == 5 && ((P->type == 'd' && P->deg == 3 && P->dconst.limb_ok) || (P->type == 'f' && P->fconst.pl_ok))) {
    // (the borrowed constants of the pairing kernels' limb-form steps fit this q: host_params.h limb_ok / pl_ok)
    if (P->type == 'd') {
      if (w == 2) hipLaunchKernelGGL((l5_mpz_kernel<KPd, 2>), dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, kargs<5>(P));
      else hipLaunchKernelGGL((l5_mpz_kernel<KPd, 4>), dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, kargs<5>(P));
    } else {
      if (w == 2) hipLaunchKernelGGL((l5_mpz_kernel<KPf, 2>), dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, kargs<5>(P));
      else hipLaunchKernelGGL((l5_mpz_kernel<KPf, 4>), dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, kargs<5>(P));
    }
    hipLaunchKernelGGL(ec_mpz_complete_kernel<FqOps<5>>, dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, w, (const uint8_t *) flags, n, kargs<5>(P));
  } else {
    PBC_DISPATCH_MPZ(P, group, {
      if (flags && w == 2) hipLaunchKernelGGL((ec_mpz_fast_kernel<F, 2>), dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, kargs<F::NW>(P));
      else if (flags) hipLaunchKernelGGL((ec_mpz_fast_kernel<F, 4>), dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, flags, n, kargs<F::NW>(P));
      hipLaunchKernelGGL(ec_mpz_complete_kernel<F>, dim3(grid), dim3(kBlock), 0, s, out, in, dig, nd, w, (const uint8_t *) flags, n, kargs<F::NW>(P));
    });
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
// everything that can be refused without a device, in the order the header states
static int mpz_check(const pbc_hip_pairing_s *P, int group, const void *out, const void *in, const uint8_t *k, size_t klen, size_t n) {
  if (!P) return fail("null pairing");
  if (group < 1 || group > 3) return fail("element_mul_mpz: group must be 1, 2 or 3 (GT)");
  if (klen > PBC_HIP_MPZ_MAX_BYTES) return fail("element_mul_mpz: klen %zu exceeds PBC_HIP_MPZ_MAX_BYTES (%d)", klen, PBC_HIP_MPZ_MAX_BYTES);
  if (klen && !k) return fail("null argument: k with klen > 0");
  if (n && (!out || !in)) return fail("null argument");
  if (!n) return 0;
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  return 0;
}
static size_t mpz_len(const pbc_hip_pairing_s *P, int group) { return (size_t) (group == 1 ? P->len1 : group == 2 ? P->len2 : P->lenT); }

extern "C" int pbc_hip_element_mul_mpz_batch(pbc_hip_pairing_t *P, int group, uint8_t *out, const uint8_t *in, const uint8_t *k, size_t klen, size_t n) {
  if (mpz_check(P, group, out, in, k, klen, n)) return 1;
  if (!n) return 0;
  {
    DeviceGuard guard(P->ndev > 0 ? P->devs[0] : P->device);
    if (ensure_derived(P, 0)) return 1;
  }
  std::vector<int8_t> digits;
  const int w = mpz_recode(group, k, klen, digits);
  const size_t L = mpz_len(P, group);
  return run_host_generic(P, out, L, in, L, nullptr, 0, n,
                          [P, group, &digits, w](void *d_out, const void *d_in, const void *, size_t m, hipStream_t s, const OwnWs *own) {
                            return mpz_launch(P, group, d_out, d_in, digits, w, m, s, own);
                          }, false);
}
extern "C" int pbc_hip_element_mul_mpz_batch_dev(pbc_hip_pairing_t *P, int group, void *d_out, const void *d_in, const uint8_t *k, size_t klen, size_t n, void *stream) {
  if (mpz_check(P, group, d_out, d_in, k, klen, n)) return 1;
  if (!n) return 0;
  if (ensure_derived(P, 0)) return 1;
  std::vector<int8_t> digits;
  const int w = mpz_recode(group, k, klen, digits);      // k is read here, before the call returns
  return mpz_launch(P, group, d_out, d_in, digits, w, n, (hipStream_t) stream, nullptr);
}
// the digit string the kernels of such a call run on.  w = 0: the library's own choice for a call on points (the plain
// NAF or the width-4 NAF, mpz_plan.h mpz_recode); w = 1: the bits (GT); w >= 2: the width-w NAF.  Digit i at out[i], the
// first `cap` of them; returns their number
extern "C" size_t pbc_hip_diag_mpz_digits(const uint8_t *k, size_t klen, int w, int8_t *out, size_t cap) {
  if ((klen && !k) || klen > PBC_HIP_MPZ_MAX_BYTES || w < 0 || w > pbc_host::kMpzMaxWidth) return 0;
  std::vector<int8_t> digits;
  if (w) pbc_host::mpz_digits(k, klen, w, digits);
  else (void) pbc_host::mpz_recode(false, k, klen, digits);
  for (size_t i = 0; out && i < digits.size() && i < cap; i++) out[i] = digits[i];
  return digits.size();
}
