// pbc_hip_member.hip -- kernels and C-ABI entry points of the membership verdicts (group_member.cuh;
// include/pbc_hip.h pbc_hip_element_membership_batch): libpbc_hip.so; see host_common.h
#include "host_common.h"
#include "group_member.cuh"

// G1 / G2 over a field policy: the fast lane writes every verdict and a flag; the complete lane rewrites the verdicts of
// the flagged lanes (flags == null: of every lane -- "hip_group_slow 1").  One byte per unit is all either of them stores.
template <class F, class RP>
__global__ void __launch_bounds__(kBlock, 2) ec_member_fast_kernel(uint8_t *res, const uint8_t *in, uint8_t *flags, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  bool flag;
  const uint8_t v = ec_member_fast_lane<F, RP>(in + idx * 2 * (size_t) F::bytes(), flag);
  flags[idx] = flag ? 1 : 0;
  res[idx] = v;
}
template <class F, class RP>
__global__ void __launch_bounds__(kBlock, 2) ec_member_complete_kernel(uint8_t *res, const uint8_t *in, const uint8_t *flags, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  if (flags && !flags[idx]) return;
  res[idx] = ec_member_complete_lane<F, RP>(in + idx * 2 * (size_t) F::bytes());
}
// Type a, 512-bit field: the fast lane in limb form, resident workgroups as the ladder of element_mul_zn (al_gmul_kernel)
template <int N>
__global__ void __launch_bounds__(kBlock, PBC_A_WAVES) al_member_kernel(uint8_t *res, const uint8_t *in, uint8_t *flags, size_t n, unsigned *ctr, KArgs<N> ka) {
  PBC_RESIDENT_LOOP(n, ctr) {
    size_t idx = PBC_UNIT_INDEX;
    size_t ld = idx < n ? idx : n - 1;
    bool flag;
    const uint8_t v = MemberAL<N>::fast_lane(in + ld * 8 * N, flag);
    if (idx < n) {
      flags[idx] = flag ? 1 : 0;
      res[idx] = v;
    }
  }
}
template <int N>
__global__ void __launch_bounds__(kBlock, PBC_A_WAVES) al_gt_member_kernel(uint8_t *res, const uint8_t *in, int zlen, uint8_t *flags, size_t n, unsigned *ctr, KArgs<N> ka) {
  PBC_RESIDENT_LOOP(n, ctr) {
    size_t idx = PBC_UNIT_INDEX;
    size_t ld = idx < n ? idx : n - 1;
    bool flag;
    const uint8_t v = MemberAL<N>::gt_fast_lane(in + ld * 8 * N, zlen, flag);
    if (idx < n) {
      flags[idx] = flag ? 1 : 0;
      res[idx] = v;
    }
  }
}
// GT over a field policy: x^r by square-and-multiply (flags != null: the lanes al_gt_member_kernel reported)
template <class G, class RP>
__global__ void __launch_bounds__(kBlock, 2) gt_member_kernel(uint8_t *res, const uint8_t *in, const uint8_t *flags, size_t n, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  if (flags && !flags[idx]) return;
  res[idx] = gt_member_lane<G, RP>(in + idx * (size_t) G::bytes());
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// F = the field policy of group 1 / 2, RP = where the constant block keeps r (group_member.cuh ROf*)
#define PBC_DISPATCH_MEMBER(P_, group_, ...)                                                                            \
  do {                                                                                                                  \
    const int t_ = (P_)->type;                                                                                          \
    if (t_ == 'a' || t_ == '1') { typedef ROfA RP; if ((P_)->nlimb == 16) { typedef FqOps<16> F; __VA_ARGS__; } else { typedef FqOps<33> F; __VA_ARGS__; } } \
    else if (t_ == 'e') { typedef ROfE RP; if ((P_)->nlimb == 16) { typedef FqOps<16> F; __VA_ARGS__; } else { typedef FqOps<33> F; __VA_ARGS__; } } \
    else if (t_ == 'f') {                                                                                               \
      typedef ROfF RP;                                                                                                  \
      if ((group_) == 2) { PBC_DISPATCH_F((P_)->nlimb, { typedef Fq2Ops<N> F; __VA_ARGS__; }); }                         \
      else { PBC_DISPATCH_F((P_)->nlimb, { typedef FqOps<N> F; __VA_ARGS__; }); }                                       \
    } else {                                                                                                            \
      typedef ROfD RP;                                                                                                  \
      if ((group_) == 2) { PBC_DISPATCH_D(P_, { typedef FdOps<N, DEG> F; __VA_ARGS__; }); }                             \
      else { PBC_DISPATCH_D(P_, { typedef FqOps<N> F; (void) DEG; __VA_ARGS__; }); }                                    \
    }                                                                                                                   \
  } while (0)
#define PBC_DISPATCH_MEMBER_GT(P_, ...)                                                                                 \
  do {                                                                                                                  \
    const int t_ = (P_)->type;                                                                                          \
    if (t_ == 'a' || t_ == '1') { typedef ROfA RP; if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if (t_ == 'e') { typedef ROfE RP; if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if (t_ == 'f') { typedef ROfF RP; PBC_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); }           \
    else { typedef ROfD RP; PBC_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                              \
  } while (0)

// enqueue n units on stream s (device pointers); `own`: the workspace of a host-path stream, else the object's table entry
// of (device, stream), pinned with its issue lock until the kernels are enqueued (ProdWs)
static int member_launch(pbc_hip_pairing_s *P, int group, void *d_res, const void *d_in, size_t n, hipStream_t s, const OwnWs *own) {
  if (!n) return 0;
  uint8_t *res = (uint8_t *) d_res;
  const uint8_t *in = (const uint8_t *) d_in;
  const unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  const bool fast_a = P->type == 'a' && !P->a_generic && !P->group_slow;
  ProdWs W(P, s, own);
  uint8_t *flags = nullptr;
  if (!P->group_slow && (group != 3 || fast_a)) {
    flags = (uint8_t *) W.get(n);
    if (!flags) return 1;
  }
  if (group == 3) {
    if (fast_a)
      hipLaunchKernelGGL(al_gt_member_kernel<16>, dim3(PBC_RGRID(al_gt_member_kernel<16>)), dim3(kBlock), 0, s, res, in, P->len_zr, flags, n, unit_counter(P, s), kargs<16>(P));
    PBC_DISPATCH_MEMBER_GT(P, hipLaunchKernelGGL((gt_member_kernel<G, RP>), dim3(grid), dim3(kBlock), 0, s, res, in, (const uint8_t *) flags, n, kargs<G::NW>(P)));
  } else if (fast_a) {
    hipLaunchKernelGGL(al_member_kernel<16>, dim3(PBC_RGRID(al_member_kernel<16>)), dim3(kBlock), 0, s, res, in, flags, n, unit_counter(P, s), kargs<16>(P));
    hipLaunchKernelGGL((ec_member_complete_kernel<FqOps<16>, ROfA>), dim3(grid), dim3(kBlock), 0, s, res, in, (const uint8_t *) flags, n, kargs<16>(P));
  } else {
    PBC_DISPATCH_MEMBER(P, group, {
      if (flags) hipLaunchKernelGGL((ec_member_fast_kernel<F, RP>), dim3(grid), dim3(kBlock), 0, s, res, in, flags, n, kargs<F::NW>(P));
      hipLaunchKernelGGL((ec_member_complete_kernel<F, RP>), dim3(grid), dim3(kBlock), 0, s, res, in, (const uint8_t *) flags, n, kargs<F::NW>(P));
    });
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
static int member_check(const pbc_hip_pairing_s *P, int group, const void *res, const void *in, size_t n) {
  if (!P) return fail("null pairing");
  if (group < 1 || group > 3) return fail("element_membership: group must be 1, 2 or 3 (GT)");
  if (n && (!res || !in)) return fail("null argument");
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  return 0;
}
static size_t member_len(const pbc_hip_pairing_s *P, int group) { return (size_t) (group == 1 ? P->len1 : group == 2 ? P->len2 : P->lenT); }

extern "C" int pbc_hip_element_membership_batch(pbc_hip_pairing_t *P, int group, uint8_t *res, const uint8_t *in, size_t n) {
  if (member_check(P, group, res, in, n)) return 1;
  if (!n) return 0;
  {
    DeviceGuard guard(P->ndev > 0 ? P->devs[0] : P->device);
    if (ensure_derived(P, 0)) return 1;
  }
  return run_host_generic(P, res, 1, in, member_len(P, group), nullptr, 0, n,
                          [P, group](void *d_res, const void *d_in, const void *, size_t m, hipStream_t s, const OwnWs *own) {
                            return member_launch(P, group, d_res, d_in, m, s, own);
                          }, false);
}
extern "C" int pbc_hip_element_membership_batch_dev(pbc_hip_pairing_t *P, int group, void *d_res, const void *d_in, size_t n, void *stream) {
  if (member_check(P, group, d_res, d_in, n)) return 1;
  if (!n) return 0;
  if (ensure_derived(P, 0)) return 1;
  return member_launch(P, group, d_res, d_in, n, (hipStream_t) stream, nullptr);
}
