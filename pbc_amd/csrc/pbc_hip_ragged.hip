// pbc_hip_ragged.hip -- ragged products of pairings: one call, a term count per product (include/pbc_hip.h
// pbc_hip_element_prod_pairing_ragged_batch): libpbc_hip.so; see host_common.h
#include "host_common.h"
#include "group_more.cuh"

// ---- kernels of the GT route (one unit per lane; lane bodies: group_more.cuh) ------------------------------------
// one byte per term: both records deserialise to a point other than O
template <class F1, class F2>
__global__ void __launch_bounds__(kBlock, 2) ragged_flag_kernel(uint8_t *flags, const uint8_t *g1, const uint8_t *g2, size_t n, KArgs<F1::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  flags[idx] = term_flag_lane<F1, F2>(g1 + idx * 2 * (size_t) F1::bytes(), g2 + idx * 2 * (size_t) F2::bytes());
}
// Output record j of a fold level belongs to the product u with oout[u] <= j < oout[u + 1] (binary search over the
// level's offsets; an empty product shares its offset with its successor and is never found) and is the product of the
// records oin[u] + b F .. of its block b = j - oout[u] (ragged_plan.h).
static __device__ __forceinline__ size_t ragged_find(const uint64_t *o, size_t n, uint64_t j) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (o[mid + 1] > j) hi = mid; else lo = mid + 1;
  }
  return lo;
}
template <class G>
__global__ void __launch_bounds__(kBlock, 2) ragged_gt_fold_kernel(uint8_t *out, uint8_t *fout, const uint8_t *in, const uint8_t *fin,
                                                                    const uint64_t *oin, const uint64_t *oout, size_t n, size_t nout, unsigned F,
                                                                    KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= nout) return;
  const size_t u = ragged_find(oout, n, idx), L = (size_t) G::bytes();
  const uint64_t start = oin[u] + (idx - oout[u]) * F, left = oin[u + 1] - start;
  const int cnt = (int) (left < F ? left : F);
  fout[idx] = gt_fold_lane<G>(out + idx * L, in + start * L, fin + start, cnt);
}
// one product per lane: its last records (at most F; none: the identity) -> GT bytes
template <class G>
__global__ void __launch_bounds__(kBlock, 2) ragged_gt_finish_kernel(uint8_t *gt, const uint8_t *in, const uint8_t *fin, const uint64_t *off, size_t n,
                                                                      KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = (size_t) G::bytes();
  const uint64_t a = off[idx], b = off[idx + 1];
  gt_fold_finish_lane<G>(gt + idx * L, in + a * L, fin + a, (int) (b - a));
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// G = GT as a field policy; F1 / F2 = the field policies of G1 / G2 (the policies ec_affine_op_kernel runs over)
#define PBC_RAGGED_DISPATCH(P_, ...)                                                                                          \
  do {                                                                                                                        \
    if ((P_)->type == 'a' || (P_)->type == '1') {                                                                             \
      if ((P_)->nlimb == 16) { typedef GtA<16> G [[maybe_unused]]; typedef FqOps<16> F1 [[maybe_unused]]; typedef F1 F2 [[maybe_unused]]; __VA_ARGS__; }                         \
      else { typedef GtA<33> G [[maybe_unused]]; typedef FqOps<33> F1 [[maybe_unused]]; typedef F1 F2 [[maybe_unused]]; __VA_ARGS__; }                                           \
    } else if ((P_)->type == 'e') {                                                                                           \
      if ((P_)->nlimb == 16) { typedef GtE<16> G [[maybe_unused]]; typedef FqOps<16> F1 [[maybe_unused]]; typedef F1 F2 [[maybe_unused]]; __VA_ARGS__; }                         \
      else { typedef GtE<33> G [[maybe_unused]]; typedef FqOps<33> F1 [[maybe_unused]]; typedef F1 F2 [[maybe_unused]]; __VA_ARGS__; }                                           \
    } else if ((P_)->type == 'f') {                                                                                           \
      PBC_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G [[maybe_unused]]; typedef FqOps<N> F1 [[maybe_unused]]; typedef Fq2Ops<N> F2 [[maybe_unused]]; __VA_ARGS__; });             \
    } else {                                                                                                                  \
      PBC_DISPATCH_D(P_, { typedef GtD<N, DEG> G [[maybe_unused]]; typedef FqOps<N> F1 [[maybe_unused]]; typedef FdOps<N, DEG> F2 [[maybe_unused]]; __VA_ARGS__; });             \
    }                                                                                                                         \
  } while (0)

// The folds and the finish of the GT route on records and flag bytes that are in place (host_common.h; also the tail of
// a product over a table set, pbc_hip_ppset.hip): one fold kernel per level, the records ping-pong between the two areas
int ragged_gt_reduce(pbc_hip_pairing_s *P, void *d_gt, void *cur_, void *fcur_, void *nxt_, void *fnxt_, const uint64_t *const *d_plan,
                     const size_t *sizes, int nl, size_t n, unsigned F, hipStream_t s) {
  uint8_t *cur = (uint8_t *) cur_, *nxt = (uint8_t *) nxt_, *fcur = (uint8_t *) fcur_, *fnxt = (uint8_t *) fnxt_;
  for (int l = 0; l + 1 < nl; l++) {
    const size_t nout = sizes[(size_t) l + 1];
    const unsigned grid = (unsigned) ((nout + kBlock - 1) / kBlock);
    PBC_RAGGED_DISPATCH(P, hipLaunchKernelGGL(ragged_gt_fold_kernel<G>, dim3(grid), dim3(kBlock), 0, s, nxt, fnxt, (const uint8_t *) cur, (const uint8_t *) fcur,
                                              d_plan[(size_t) l], d_plan[(size_t) l + 1], n, nout, F, kargs<G::NW>(P)));
    std::swap(cur, nxt);
    std::swap(fcur, fnxt);
  }
  const unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  PBC_RAGGED_DISPATCH(P, hipLaunchKernelGGL(ragged_gt_finish_kernel<G>, dim3(grid), dim3(kBlock), 0, s, (uint8_t *) d_gt, (const uint8_t *) cur, (const uint8_t *) fcur,
                                            d_plan[(size_t) nl - 1], n, kargs<G::NW>(P)));
  HIP_TRY(hipGetLastError());
  return 0;
}

static size_t ws_round(size_t b) { return (b + 255) & ~(size_t) 255; }
static bool record_route(const pbc_hip_pairing_s *P) { return P->type == 'a' && !P->a_generic; }

// One launch group: n products, at most kRaggedMaxTerms terms, offsets[0] .. offsets[n] (host) relative to the device
// arrays.  Everything the group keeps lives in the SECOND buffer of the (device, stream) workspace, held with its issue
// lock until the last kernel is enqueued: the plan, then the records of the levels (two areas, used in turn) and, on the
// GT route, their flag bytes.  The plan reaches the device with ONE stream-ordered copy from the workspace's page-locked
// staging: behind the kernels of an earlier call on this stream, which still read THEIR plan from the same bytes, and
// the staging is not rewritten before the copy that reads it is done (HostStage).  No allocation in the steady state.
static int ragged_group(pbc_hip_pairing_s *P, uint8_t *d_gt, const uint8_t *d_g1, const uint8_t *d_g2, const uint64_t *offsets, size_t n,
                        hipStream_t s, const OwnWs *own) {
  const unsigned F = (unsigned) P->ragged_fold;
  std::vector<std::vector<uint64_t>> levels;
  pbc_host::ragged_plan(offsets, n, F, levels);
  const int nl = (int) levels.size();
  std::vector<size_t> sizes((size_t) nl);
  for (int l = 0; l < nl; l++) sizes[(size_t) l] = (size_t) levels[(size_t) l][n];
  const size_t T = sizes[0], lt = (size_t) P->lenT;
  const bool rec_route = record_route(P);
  const size_t rec = rec_route ? AL<16>::MREC * sizeof(uint4) : lt;
  const size_t plan_bytes = (size_t) nl * (n + 1) * sizeof(uint64_t);
  const size_t nA = T ? T : 1, nB = nl > 1 ? sizes[1] : 0;
  const size_t offA = ws_round(plan_bytes), offB = offA + ws_round(nA * rec);
  const size_t offFA = offB + ws_round(nB * rec), offFB = offFA + ws_round(rec_route ? 0 : nA);
  const size_t total = offFB + ws_round(rec_route ? 0 : nB);
  ProdWs W(P, s, own);
  uint8_t *buf = (uint8_t *) W.get2(total);
  if (!buf) return 1;
  HostStage *hs = W.stage();
  if (!hs) return fail("internal: a ragged launch without host staging");
  uint64_t *h = (uint64_t *) stage_acquire(*hs, plan_bytes);
  if (!h) return 1;
  std::vector<const uint64_t *> d_plan((size_t) nl);
  for (int l = 0; l < nl; l++) {
    memcpy(h + (size_t) l * (n + 1), levels[(size_t) l].data(), (n + 1) * sizeof(uint64_t));
    d_plan[(size_t) l] = (const uint64_t *) buf + (size_t) l * (n + 1);
  }
  HIP_TRY(hipMemcpyAsync(buf, h, plan_bytes, hipMemcpyHostToDevice, s));
  if (stage_copied(*hs, s)) return 1;
  if (rec_route) return ragged_records_a(P, d_gt, d_g1, d_g2, n, F, d_plan.data(), sizes.data(), nl, buf + offA, buf + offB, s);
  // GT route: the T terms as single pairings through the pairings' own launcher (wave and lane kernels are chosen there,
  // as for a k = 1 batch of T units), one flag byte per term, then the folds over GT records
  uint8_t *cur = buf + offA, *nxt = buf + offB, *fcur = buf + offFA, *fnxt = buf + offFB;
  if (T) {
    if (launch_pairings(P, cur, d_g1, d_g2, T, s, own)) return 1;
    const unsigned grid = (unsigned) ((T + kBlock - 1) / kBlock);
    PBC_RAGGED_DISPATCH(P, hipLaunchKernelGGL((ragged_flag_kernel<F1, F2>), dim3(grid), dim3(kBlock), 0, s, fcur, d_g1, d_g2, T, kargs<F1::NW>(P)));
  }
  return ragged_gt_reduce(P, d_gt, cur, fcur, nxt, fnxt, d_plan.data(), sizes.data(), nl, n, F, s);
}
// a call whose terms exceed kRaggedMaxTerms: launch groups that end at product boundaries, one after the other on s
int ragged_launch(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, const uint64_t *offsets, size_t n,
                  hipStream_t s, const OwnWs *own) {
  const size_t l1 = (size_t) P->len1, l2 = (size_t) P->len2, lt = (size_t) P->lenT;
  for (size_t u0 = 0, u1; u0 < n; u0 = u1) {
    u1 = u0 + 1;
    while (u1 < n && offsets[u1 + 1] - offsets[u0] <= pbc_host::kRaggedMaxTerms) u1++;
    const size_t t0 = (size_t) (offsets[u0] - offsets[0]);
    if (ragged_group(P, (uint8_t *) d_gt + u0 * lt, (const uint8_t *) d_g1 + t0 * l1, (const uint8_t *) d_g2 + t0 * l2, offsets + u0, u1 - u0, s, own)) return 1;
  }
  return 0;
}

// argument checks first, then the device: the checks run without a GPU
static int ragged_check_args(const pbc_hip_pairing_s *P, const void *gt, const void *g1, const void *g2, const uint64_t *offsets, size_t n) {
  if (!P) return fail("null pairing");
  if (!gt || !g1 || !g2 || !offsets) return fail("null argument");
  size_t at = 0;
  switch (pbc_host::ragged_check(offsets, n, &at)) {
    case 1: return fail("ragged products: offsets[0] must be 0 (got %llu)", (unsigned long long) offsets[0]);
    case 2: return fail("ragged products: offsets decrease at index %zu (%llu > %llu)", at, (unsigned long long) offsets[at], (unsigned long long) offsets[at + 1]);
    case 3: return fail("ragged products: product %zu has %llu terms, more than 2^22", at, (unsigned long long) (offsets[at + 1] - offsets[at]));
    default: return 0;
  }
}
extern "C" int pbc_hip_element_prod_pairing_ragged_batch_dev(pbc_hip_pairing_t *P, void *d_gt, const void *d_g1, const void *d_g2,
                                                             const uint64_t *offsets, size_t n, void *stream) {
  if (ragged_check_args(P, d_gt, d_g1, d_g2, offsets, n)) return 1;
  if (!n) return 0;
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  if (ensure_derived(P, (hipStream_t) stream)) return 1;
  return ragged_launch(P, d_gt, d_g1, d_g2, offsets, n, (hipStream_t) stream, nullptr);
}
extern "C" int pbc_hip_element_prod_pairing_ragged_batch(pbc_hip_pairing_t *P, uint8_t *gt, const uint8_t *g1, const uint8_t *g2,
                                                         const uint64_t *offsets, size_t n) {
  if (ragged_check_args(P, gt, g1, g2, offsets, n)) return 1;
  if (!n) return 0;
  return run_host_ragged(P, gt, g1, g2, offsets, n);
}
// the plan of a call, for the tests: per level its length (n + 1) and its offsets, level 0 (the caller's array) first;
// returns the number of values the whole plan takes (at most `cap` are written), 0 for arguments the entry points refuse
extern "C" size_t pbc_hip_diag_ragged_plan(pbc_hip_pairing_t *P, const uint64_t *offsets, size_t n, uint64_t *out, size_t cap) {
  if (ragged_check_args(P, offsets, offsets, offsets, offsets, n)) return 0;
  std::vector<std::vector<uint64_t>> levels;
  pbc_host::ragged_plan(offsets, n, (unsigned) P->ragged_fold, levels);
  size_t at = 0;
  for (const auto &lv : levels) {
    if (out && at < cap) out[at] = lv.size();
    at++;
    for (uint64_t v : lv) { if (out && at < cap) out[at] = v; at++; }
  }
  return at;
}
