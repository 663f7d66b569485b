// pbc_hip_gtdiv.hip -- kernels and C-ABI entry points of element_invert / element_div on GT and of element_cmp
// (group_gtdiv.cuh, cmp_plan.h; include/pbc_hip.h pbc_hip_element_invert_GT_batch, pbc_hip_element_cmp_batch):
// libpbc_hip.so; see host_common.h
#include "host_common.h"
#include "group_gtdiv.cuh"
#include "mpz_plan.h"
#include "cmp_plan.h"

// GT: one kernel each; the inversion in the subfield sits behind a per-lane branch (generic: every lane takes it)
template <class G>
__global__ void __launch_bounds__(kBlock, 2) gt_invert_kernel(uint8_t *out, const uint8_t *a, bool generic, size_t n, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = (size_t) G::bytes();
  (void) gt_invert_lane<G>(out + idx * L, a + idx * L, generic);
}
template <class G>
__global__ void __launch_bounds__(kBlock, 2) gt_div_kernel(uint8_t *out, const uint8_t *a, const uint8_t *b, bool generic, size_t n, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = (size_t) G::bytes();
  (void) gt_div_lane<G>(out + idx * L, a + idx * L, b + idx * L, generic);
}
// element_cmp on the plain groups: load, compare, one byte
template <int N>
__global__ void __launch_bounds__(kBlock) zr_cmp_kernel(uint8_t *res, const uint8_t *a, const uint8_t *b, size_t n, KArgs<N> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = fpk<N>().fbytes;
  res[idx] = zr_cmp_lane<N>(a + idx * L, b + idx * L);
}
template <class G>
__global__ void __launch_bounds__(kBlock, 2) gt_cmp_kernel(uint8_t *res, const uint8_t *a, const uint8_t *b, size_t n, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = (size_t) G::bytes();
  res[idx] = gt_cmp_lane<G>(a + idx * L, b + idx * L);
}
template <class F>
__global__ void __launch_bounds__(kBlock, 2) ec_cmp_plain_kernel(uint8_t *res, const uint8_t *a, const uint8_t *b, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = 2 * (size_t) F::bytes();
  res[idx] = ec_cmp_plain_lane<F>(a + idx * L, b + idx * L);
}
// The coset compare of the twists: the fast lane writes every verdict and a flag; the complete lane rewrites the verdicts
// of the flagged lanes (flags == null: of every lane -- "hip_group_slow 1").  dig / nd: the digits of c - 1 (pbc_hip_mpz.hip)
template <class F, int W>
__global__ void __launch_bounds__(kBlock, 2) ec_cmp_fast_kernel(uint8_t *res, const uint8_t *a, const uint8_t *b, const uint32_t *dig, int nd, uint8_t *flags, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = 2 * (size_t) F::bytes();
  bool flag;
  const uint8_t v = ec_cmp_fast_lane<F, W>(a + idx * L, b + idx * L, dig, nd, flag);
  flags[idx] = flag ? 1 : 0;
  res[idx] = v;
}
template <class F>
__global__ void __launch_bounds__(kBlock, 2) ec_cmp_complete_kernel(uint8_t *res, const uint8_t *a, const uint8_t *b, const uint32_t *dig, int nd, int w, const uint8_t *flags, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  if (flags && !flags[idx]) return;
  const size_t L = 2 * (size_t) F::bytes();
  res[idx] = ec_cmp_complete_lane<F>(a + idx * L, b + idx * L, dig, nd, w);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static bool symmetric(const pbc_hip_pairing_s *P) { return P->type == 'a' || P->type == '1' || P->type == 'e'; }
#define PBC_DISPATCH_GTDIV(P_, ...)                                                            \
  do {                                                                                         \
    if ((P_)->type == 'a' || (P_)->type == '1') { if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if ((P_)->type == 'e') { if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if ((P_)->type == 'f') { PBC_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); } \
    else { PBC_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                      \
  } while (0)

// d_b == null: invert
static int gtdiv_launch(pbc_hip_pairing_s *P, void *d_out, const void *d_a, const void *d_b, size_t n, hipStream_t s) {
  if (!n) return 0;
  uint8_t *out = (uint8_t *) d_out;
  const uint8_t *a = (const uint8_t *) d_a, *b = (const uint8_t *) d_b;
  const unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  const bool generic = P->group_slow;
  PBC_DISPATCH_GTDIV(P, {
    if (b) hipLaunchKernelGGL(gt_div_kernel<G>, dim3(grid), dim3(kBlock), 0, s, out, a, b, generic, n, kargs<G::NW>(P));
    else hipLaunchKernelGGL(gt_invert_kernel<G>, dim3(grid), dim3(kBlock), 0, s, out, a, generic, n, kargs<G::NW>(P));
  });
  HIP_TRY(hipGetLastError());
  return 0;
}
// everything that can be refused without a device, in the order the header states
static int gtdiv_check(const pbc_hip_pairing_s *P, const char *what, bool binary, const void *out, const void *a, const void *b, size_t n) {
  if (!P) return fail("null pairing");
  if (n && (!out || !a || (binary && !b))) return fail("%s: null argument", what);
  if (!n) return 0;
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  return 0;
}
static int gtdiv_host(pbc_hip_pairing_t *P, const char *what, bool binary, uint8_t *out, const uint8_t *a, const uint8_t *b, size_t n) {
  if (gtdiv_check(P, what, binary, out, a, b, n)) return 1;
  if (!n) return 0;
  {
    DeviceGuard guard(P->ndev > 0 ? P->devs[0] : P->device);
    if (ensure_derived(P, 0)) return 1;
  }
  const size_t L = (size_t) P->lenT;
  return run_host_generic(P, out, L, a, L, b, b ? L : 0, n,
                          [P](void *d_out, const void *d_a, const void *d_b, size_t m, hipStream_t s, const OwnWs *) {
                            return gtdiv_launch(P, d_out, d_a, d_b, m, s);
                          }, false);
}
static int gtdiv_dev(pbc_hip_pairing_t *P, const char *what, bool binary, void *d_out, const void *d_a, const void *d_b, size_t n, void *stream) {
  if (gtdiv_check(P, what, binary, d_out, d_a, d_b, n)) return 1;
  if (!n) return 0;
  if (ensure_derived(P, 0)) return 1;
  return gtdiv_launch(P, d_out, d_a, d_b, n, (hipStream_t) stream);
}
extern "C" int pbc_hip_element_invert_GT_batch(pbc_hip_pairing_t *P, uint8_t *out, const uint8_t *a, size_t n) {
  return gtdiv_host(P, "element_invert_GT", false, out, a, nullptr, n);
}
extern "C" int pbc_hip_element_div_GT_batch(pbc_hip_pairing_t *P, uint8_t *out, const uint8_t *a, const uint8_t *b, size_t n) {
  return gtdiv_host(P, "element_div_GT", true, out, a, b, n);
}
extern "C" int pbc_hip_element_invert_GT_batch_dev(pbc_hip_pairing_t *P, void *d_out, const void *d_a, size_t n, void *stream) {
  return gtdiv_dev(P, "element_invert_GT", false, d_out, d_a, nullptr, n, stream);
}
extern "C" int pbc_hip_element_div_GT_batch_dev(pbc_hip_pairing_t *P, void *d_out, const void *d_a, const void *d_b, size_t n, void *stream) {
  return gtdiv_dev(P, "element_div_GT", true, d_out, d_a, d_b, n, stream);
}

// ---- element_cmp ------------------------------------------------------------------------------------------------------------
// The digits of a call on a twist: c - 1 for the integer c the kernels walk (cmp_plan.h), recoded as a call of
// element_mul_mpz on points would recode it (mpz_plan.h mpz_recode: the plain or the width-4 NAF)
struct CmpPlan {
  bool coset = false;
  std::vector<int8_t> digits;
  int w = 2;
};
static int cmp_plan(const pbc_hip_pairing_s *P, int group, CmpPlan &C) {
  C.coset = group == 2 && !symmetric(P);
  if (!C.coset) return 0;
  std::vector<uint8_t> c;
  if (!pbc_host::cmp_quotient(P->param_text.data(), P->param_text.size(), 1, c) || c.empty())
    return fail("element_cmp: quotient_cmp cannot be derived from the parameter text");
  if (c.size() > PBC_HIP_MPZ_MAX_BYTES) return fail("element_cmp: quotient_cmp exceeds PBC_HIP_MPZ_MAX_BYTES");
  for (size_t i = c.size(); i-- > 0;) if (c[i]--) break;         // c - 1 (c >= 1)
  C.w = pbc_host::mpz_recode(false, c.data(), c.size(), C.digits);
  return 0;
}
static int cmp_launch(pbc_hip_pairing_s *P, int group, const CmpPlan &C, void *d_res, const void *d_a, const void *d_b, size_t n, hipStream_t s, const OwnWs *own) {
  if (!n) return 0;
  uint8_t *res = (uint8_t *) d_res;
  const uint8_t *a = (const uint8_t *) d_a, *b = (const uint8_t *) d_b;
  const unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  if (group == 0) {
    PBC_DISPATCH_N(P->zr_nlimb, {
      KArgs<N> K;
      if (zr_kargs<N>(P, K)) return 1;
      hipLaunchKernelGGL(zr_cmp_kernel<N>, dim3(grid), dim3(kBlock), 0, s, res, a, b, n, K);
    });
  } else if (group == 3) {
    PBC_DISPATCH_GTDIV(P, hipLaunchKernelGGL(gt_cmp_kernel<G>, dim3(grid), dim3(kBlock), 0, s, res, a, b, n, kargs<G::NW>(P)));
  } else if (!C.coset) {
    PBC_DISPATCH_N(P->nlimb, hipLaunchKernelGGL(ec_cmp_plain_kernel<FqOps<N>>, dim3(grid), dim3(kBlock), 0, s, res, a, b, n, kargs<N>(P)));
  } else {
    // the digits of THIS call, stream-ordered (pbc_hip_mpz.hip digits_upload); the flags in the workspace's first buffer
    ProdWs W(P, s, own);
    const uint8_t *unused = nullptr;
    const uint32_t *dig = digits_upload(W, C.digits, std::vector<uint8_t>(), &unused, s);
    if (!dig) return 1;
    uint8_t *flags = nullptr;
    if (!P->group_slow) {
      flags = (uint8_t *) W.get(n);
      if (!flags) return 1;
    }
    const int nd = (int) C.digits.size(), w = C.w;
    PBC_DISPATCH_TWIST(P, {
      if (flags && w == 2) hipLaunchKernelGGL((ec_cmp_fast_kernel<F, 2>), dim3(grid), dim3(kBlock), 0, s, res, a, b, dig, nd, flags, n, kargs<F::NW>(P));
      else if (flags) hipLaunchKernelGGL((ec_cmp_fast_kernel<F, 4>), dim3(grid), dim3(kBlock), 0, s, res, a, b, dig, nd, flags, n, kargs<F::NW>(P));
      hipLaunchKernelGGL(ec_cmp_complete_kernel<F>, dim3(grid), dim3(kBlock), 0, s, res, a, b, dig, nd, w, (const uint8_t *) flags, n, kargs<F::NW>(P));
    });
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
static int cmp_check(const pbc_hip_pairing_s *P, int group, const void *res, const void *a, const void *b, size_t n) {
  if (!P) return fail("null pairing");
  if (n && (!res || !a || !b)) return fail("element_cmp: null argument");
  if (group < 0 || group > 3) return fail("element_cmp: group must be 0 (Z_r), 1, 2 or 3 (GT)");
  if (!n) return 0;
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (group == 0 && !P->zr_nlimb) return fail("Z_r: no arithmetic for this group order");
  return 0;
}
static size_t cmp_len(const pbc_hip_pairing_s *P, int group) {
  return (size_t) (group == 0 ? P->len_zr : group == 1 ? P->len1 : group == 2 ? P->len2 : P->lenT);
}
extern "C" int pbc_hip_element_cmp_batch(pbc_hip_pairing_t *P, int group, uint8_t *res, const uint8_t *a, const uint8_t *b, size_t n) {
  if (cmp_check(P, group, res, a, b, n)) return 1;
  if (!n) return 0;
  {
    DeviceGuard guard(P->ndev > 0 ? P->devs[0] : P->device);
    if (ensure_derived(P, 0)) return 1;
  }
  CmpPlan C;
  if (cmp_plan(P, group, C)) return 1;
  const size_t L = cmp_len(P, group);
  return run_host_generic(P, res, 1, a, L, b, L, n,
                          [P, group, &C](void *d_res, const void *d_a, const void *d_b, size_t m, hipStream_t s, const OwnWs *own) {
                            return cmp_launch(P, group, C, d_res, d_a, d_b, m, s, own);
                          }, false);
}
extern "C" int pbc_hip_element_cmp_batch_dev(pbc_hip_pairing_t *P, int group, void *d_res, const void *d_a, const void *d_b, size_t n, void *stream) {
  if (cmp_check(P, group, d_res, d_a, d_b, n)) return 1;
  if (!n) return 0;
  if (ensure_derived(P, 0)) return 1;
  CmpPlan C;
  if (cmp_plan(P, group, C)) return 1;
  return cmp_launch(P, group, C, d_res, d_a, d_b, n, (hipStream_t) stream, nullptr);
}
// quotient_cmp of G2 (which = 0) or the integer the kernels walk (which = 1) as a big-endian magnitude: the first `cap`
// bytes at out; returns its length, 0 where element_cmp is a plain comparison.  Pure host code.
extern "C" size_t pbc_hip_diag_quotient_cmp(pbc_hip_pairing_t *P, int group, int which, uint8_t *out, size_t cap) {
  if (!P || group != 2 || which < 0 || which > 1 || symmetric(P)) return 0;
  std::vector<uint8_t> c;
  if (!pbc_host::cmp_quotient(P->param_text.data(), P->param_text.size(), which, c)) return 0;
  for (size_t i = 0; out && i < c.size() && i < cap; i++) out[i] = c[i];
  return c.size();
}
