// pbc_hip_ppset.hip -- sets of preprocessed first arguments: many tables of pairing_pp_init in one object, one launch to
// build them, one call to apply them segment by segment or as the fixed first arguments of a batch of products
// (include/pbc_hip.h pbc_hip_pairing_pp_set_*): libpbc_hip.so; see host_common.h.  The kernels that run a family's lane
// bodies live with that family (pbc_hip_a.hip, pbc_hip_d.hip); here: the object, the plans, the GT route's flag kernel.
#include "host_common.h"
#include "group_more.cuh"

// One byte per term of a product over a set: the table's flag AND the G2 record deserialises to a point other than O
// (ec_load_affine, as ragged_flag_kernel reads it).  Term-major as the apply kernels: the lane of (table j, unit u)
// writes byte u m + j.
template <class F2>
__global__ void __launch_bounds__(kBlock) pp_set_flag_kernel(uint8_t *out, const uint32_t *__restrict__ flags, const uint8_t *g2, size_t n, size_t m, KArgs<F2::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n * m) return;
  typename F2::el x, y;
  const unsigned ok = ec_load_affine<F2>(x, y, g2 + idx * 2 * (size_t) F2::bytes());
  out[idx] = (uint8_t) (ok & (unsigned) (flags[idx % m] != 0));
}
// F2 = the field policy of G2 of a family that has preprocessed pairings
#define PBC_PPSET_DISPATCH(P_, ...)                                                                    \
  do {                                                                                                 \
    if ((P_)->type == 'a' || (P_)->type == '1') {                                                      \
      if ((P_)->nlimb == 16) { typedef FqOps<16> F2; __VA_ARGS__; } else { typedef FqOps<33> F2; __VA_ARGS__; } \
    } else {                                                                                           \
      PBC_DISPATCH_D(P_, { typedef FdOps<N, DEG> F2; __VA_ARGS__; });                                  \
    }                                                                                                  \
  } while (0)

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static size_t ws_round(size_t b) { return (b + 255) & ~(size_t) 255; }
static bool is_mnt(const pbc_hip_pairing_s *P) { return P->type == 'd' || P->type == 'g'; }
static bool is_a1(const pbc_hip_pairing_s *P) { return P->type == '1' || (P->type == 'a' && P->a_generic); }   // bit-by-bit tables
static bool record_route(const pbc_hip_pairing_s *P) { return P->type == 'a' && !P->a_generic; }
// words of one table, as pbc_hip_pairing_pp_init sizes it (known on the host: the loop's digits come with the parameters)
static size_t pp_table_words(const pbc_hip_pairing_s *P) {
  if (is_mnt(P)) {                     // one entry per doubling and per addition of the Miller loop
    int steps = P->dconst.rbits - 1;
    for (int i = 1; i <= P->dconst.rbits - 2; i++) steps += ((P->dconst.r[i >> 5] | P->dconst.rm[i >> 5]) >> (i & 31)) & 1;
    return (size_t) steps * 3 * (size_t) P->nlimb;
  }
  if (is_a1(P)) {
    int steps = P->a.rbits - 1;
    for (int i = 1; i <= P->a.rbits - 2; i++) steps += ((P->a.r[i >> 5] | P->a.rm[i >> 5]) >> (i & 31)) & 1;
    return (size_t) steps * 3 * (size_t) P->nlimb;
  }
  return (size_t) (P->a.exp2 + 1) * 3 * 16;
}

// argument checks first, then the device: the checks run without a GPU
static int pp_set_create(pbc_hip_pp_set_t **out, pbc_hip_pairing_s *P, const void *g1, size_t m, bool from_device, hipStream_t s) {
  if (!out || !P || !g1) return fail("null argument");
  if (!m) return fail("pairing_pp_set_init: a set holds at least one table (m == 0)");
  if (P->type != 'a' && !is_mnt(P) && !is_a1(P))
    return fail("pairing_pp is built for types a, a1, d and g (other types: use element_pairing)");
  const size_t words = pp_table_words(P), l1 = (size_t) P->len1;
  if (m > (SIZE_MAX - 1024) / (words * 4 + 4 + l1))
    return fail("pairing_pp_set_init: %zu tables of %zu bytes overflow size_t", m, words * 4);
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  DeviceGuard guard(P->device);        // the set lives on the device the pairing object was created on, whatever is current
  if (ensure_derived(P, s)) return 1;
  const size_t off_flags = ws_round(m * words * 4), off_g1 = off_flags + ws_round(m * 4), total = off_g1 + m * l1;
  void *mem = nullptr;
  if (hipMalloc(&mem, total) != hipSuccess) { (void) hipGetLastError(); return fail("pairing_pp_set_init: device allocation of %zu bytes failed", total); }
  pbc_hip_pp_set_s *set = new pbc_hip_pp_set_s{P, P->device, m, words, mem, (uint32_t *) mem, (uint32_t *) ((uint8_t *) mem + off_flags), (uint8_t *) mem + off_g1};
  auto bail = [&](const char *what, hipError_t e) {
    (void) hipFree(mem);
    delete set;
    return e == hipSuccess ? fail("pairing_pp_set_init: %s", what) : fail("pairing_pp_set_init: %s (%s)", what, hipGetErrorString(e));
  };
  hipError_t e = from_device ? hipMemcpyAsync(set->g1, g1, m * l1, hipMemcpyDeviceToDevice, s) : hipMemcpy(set->g1, g1, m * l1, hipMemcpyHostToDevice);
  if (e != hipSuccess) return bail("copying the G1 records failed", e);
  if (is_mnt(P) ? pp_set_init_launch_d(P, set, s) : pp_set_init_launch_a(P, set, is_a1(P), s)) return bail("the table kernel could not be launched", hipSuccess);
  if (!from_device && (e = hipStreamSynchronize(s)) != hipSuccess) return bail("the table kernel failed", e);
  *out = set;
  return 0;
}
extern "C" int pbc_hip_pairing_pp_set_init(pbc_hip_pp_set_t **out, pbc_hip_pairing_t *P, const uint8_t *g1, size_t m) {
  return pp_set_create(out, P, g1, m, false, 0);
}
extern "C" int pbc_hip_pairing_pp_set_init_dev(pbc_hip_pp_set_t **out, pbc_hip_pairing_t *P, const void *d_g1, size_t m, void *stream) {
  return pp_set_create(out, P, d_g1, m, true, (hipStream_t) stream);
}
extern "C" void pbc_hip_pairing_pp_set_clear(pbc_hip_pp_set_t *set) {
  if (!set) return;
  DeviceGuard guard(set->device);
  (void) hipFree(set->mem);            // (waits for the kernels that still read the tables)
  delete set;
}
extern "C" size_t pbc_hip_pairing_pp_set_count(const pbc_hip_pp_set_t *set) { return set ? set->m : 0; }

// The plan of one launch on its way to the device: `bytes` of the second workspace buffer, the first `plan.size()`
// values of which are the plan -- ONE stream-ordered copy from the workspace's page-locked staging, behind the kernels
// of an earlier call on this stream (which still read THEIR plan from the same bytes); the staging is not rewritten
// before the copy that reads it is done (HostStage).  The entry stays pinned, its issue lock held, while W lives.
static uint8_t *plan_upload(ProdWs &W, const std::vector<uint64_t> &plan, size_t bytes, hipStream_t s) {
  const size_t pb = plan.size() * sizeof(uint64_t);
  uint8_t *buf = (uint8_t *) W.get2(bytes);
  if (!buf) return nullptr;
  HostStage *hs = W.stage();
  if (!hs) { fail("internal: a table-set launch without host staging"); return nullptr; }
  void *h = stage_acquire(*hs, pb);
  if (!h) return nullptr;
  memcpy(h, plan.data(), pb);
  if (hipMemcpyAsync(buf, h, pb, hipMemcpyHostToDevice, s) != hipSuccess) { fail("uploading the plan failed"); return nullptr; }
  if (stage_copied(*hs, s)) return nullptr;
  return buf;
}
static int family_apply(pbc_hip_pp_set_s *set, void *d_out, const void *d_g2, const uint64_t *d_plan, size_t slots, size_t stride, size_t tmul, hipStream_t s) {
  return is_mnt(set->P) ? pp_set_apply_launch_d(set, d_out, d_g2, d_plan, slots, stride, tmul, s)
                        : pp_set_apply_launch_a(set, d_out, d_g2, d_plan, slots, stride, tmul, s);
}

// ---- segmented apply -----------------------------------------------------------------------------------------------
// the units c0 <= i < c1 of a call (device pointers to unit c0's records), constants already derived
static int apply_launch(pbc_hip_pp_set_s *set, void *d_gt, const void *d_g2, const uint64_t *offsets, uint64_t c0, uint64_t c1, hipStream_t s, const OwnWs *own) {
  std::vector<uint64_t> plan;
  pbc_host::pp_set_plan_range(offsets, set->m, c0, c1, plan);
  const size_t slots = plan.size() / pbc_host::kPpSetSlotWords;
  if (!slots) return 0;
  ProdWs W(set->P, s, own);
  const uint8_t *buf = plan_upload(W, plan, plan.size() * sizeof(uint64_t), s);
  if (!buf) return 1;
  return family_apply(set, d_gt, d_g2, (const uint64_t *) buf, slots, 1, 0, s);
}
static int apply_check_args(const pbc_hip_pp_set_s *set, const void *gt, const void *g2, const uint64_t *offsets) {
  if (!set) return fail("null pp set");
  if (!gt || !g2 || !offsets) return fail("null argument");
  size_t at = 0;
  switch (pbc_host::pp_set_check(offsets, set->m, &at)) {
    case 1: return fail("pairing_pp_set_apply: offsets[0] must be 0 (got %llu)", (unsigned long long) offsets[0]);
    case 2: return fail("pairing_pp_set_apply: offsets decrease at index %zu (%llu > %llu)", at, (unsigned long long) offsets[at], (unsigned long long) offsets[at + 1]);
    default: return 0;
  }
}
extern "C" int pbc_hip_pairing_pp_set_apply_batch_dev(pbc_hip_pp_set_t *set, void *d_gt, const void *d_g2, const uint64_t *offsets, void *stream) {
  if (apply_check_args(set, d_gt, d_g2, offsets)) return 1;
  const uint64_t n = offsets[set->m];
  if (!n) return 0;
  if (ensure_derived(set->P, (hipStream_t) stream)) return 1;
  return apply_launch(set, d_gt, d_g2, offsets, 0, n, (hipStream_t) stream, nullptr);
}
extern "C" int pbc_hip_pairing_pp_set_apply_batch(pbc_hip_pp_set_t *set, uint8_t *gt, const uint8_t *g2, const uint64_t *offsets) {
  if (apply_check_args(set, gt, g2, offsets)) return 1;
  pbc_hip_pairing_s *P = set->P;
  const size_t chunk = P->host_chunk ? P->host_chunk : (size_t) 1 << 20;
  return run_host_own_device(P, gt, (size_t) P->lenT, g2, (size_t) P->len2, (size_t) offsets[set->m], chunk,
                             [set, offsets](void *d_out, const void *d_in, size_t c0, size_t cnt, hipStream_t s, const OwnWs *own) {
                               return apply_launch(set, d_out, d_in, offsets, c0, c0 + cnt, s, own);
                             });
}
// the plan of such a call, for the tests: three values per wave slot (table, first unit, count), in slot order
extern "C" size_t pbc_hip_diag_pp_set_plan(pbc_hip_pairing_t *P, const uint64_t *offsets, size_t m, uint64_t *out, size_t cap) {
  size_t at = 0;
  if (!P || !offsets || !m || pbc_host::pp_set_check(offsets, m, &at)) return 0;
  std::vector<uint64_t> plan;
  pbc_host::pp_set_plan(offsets, m, plan);
  for (size_t i = 0; out && i < plan.size() && i < cap; i++) out[i] = plan[i];
  return plan.size();
}

// ---- products over the set ---------------------------------------------------------------------------------------------
constexpr size_t kProdGroupTerms = (size_t) 1 << 22;      // terms of one launch group (the workspace bound of launch_prod)
// One launch group: nu products, term records u m + j of d_g2.  Everything the group keeps lives in the second buffer of
// the (device, stream) workspace: the slot plan, then -- 512-bit type a -- the Miller records of the terms, or -- the
// other families -- the level arrays of the fold (ragged_plan.h over the uniform offsets u m), the GT records of the
// levels (two areas, used in turn) and their flag bytes.
static int prod_group(pbc_hip_pp_set_s *set, uint8_t *d_gt, const uint8_t *d_g2, size_t nu, hipStream_t s, const OwnWs *own) {
  pbc_hip_pairing_s *P = set->P;
  const size_t m = set->m, T = nu * m;
  std::vector<uint64_t> plan;
  pbc_host::pp_set_prod_plan(m, nu, plan);
  const size_t slots = plan.size() / pbc_host::kPpSetSlotWords;
  ProdWs W(P, s, own);
  if (record_route(P)) {
    const size_t off_rec = ws_round(plan.size() * sizeof(uint64_t));
    uint8_t *buf = plan_upload(W, plan, off_rec + T * AL<16>::MREC * sizeof(uint4), s);
    if (!buf) return 1;
    return pp_set_records_a(set, d_gt, d_g2, (const uint64_t *) buf, slots, nu, buf + off_rec, s);
  }
  // the GT route: the segmented apply term-major into GT records, one flag byte per term, then the ragged call's folds
  const unsigned F = (unsigned) P->ragged_fold;
  std::vector<uint64_t> uniform(nu + 1);
  for (size_t u = 0; u <= nu; u++) uniform[u] = (uint64_t) u * m;
  std::vector<std::vector<uint64_t>> levels;
  pbc_host::ragged_plan(uniform.data(), nu, F, levels);
  const int nl = (int) levels.size();
  std::vector<size_t> sizes((size_t) nl);
  const size_t off_levels = plan.size();                   // (in values of the upload)
  for (int l = 0; l < nl; l++) {
    sizes[(size_t) l] = (size_t) levels[(size_t) l][nu];
    plan.insert(plan.end(), levels[(size_t) l].begin(), levels[(size_t) l].end());
  }
  const size_t lt = (size_t) P->lenT, nB = nl > 1 ? sizes[1] : 0;
  const size_t offA = ws_round(plan.size() * sizeof(uint64_t)), offB = offA + ws_round(T * lt);
  const size_t offFA = offB + ws_round(nB * lt), offFB = offFA + ws_round(T), total = offFB + ws_round(nB);
  uint8_t *buf = plan_upload(W, plan, total, s);
  if (!buf) return 1;
  std::vector<const uint64_t *> d_levels((size_t) nl);
  for (int l = 0; l < nl; l++) d_levels[(size_t) l] = (const uint64_t *) buf + off_levels + (size_t) l * (nu + 1);
  if (family_apply(set, buf + offA, d_g2, (const uint64_t *) buf, slots, m, 1, s)) return 1;
  const unsigned grid = (unsigned) ((T + kBlock - 1) / kBlock);
  PBC_PPSET_DISPATCH(P, hipLaunchKernelGGL(pp_set_flag_kernel<F2>, dim3(grid), dim3(kBlock), 0, s, buf + offFA, (const uint32_t *) set->flags, d_g2, nu, m, kargs<F2::NW>(P)));
  HIP_TRY(hipGetLastError());
  return ragged_gt_reduce(P, d_gt, buf + offA, buf + offFA, buf + offB, buf + offFB, d_levels.data(), sizes.data(), nl, nu, F, s);
}
// a call of more than 2^22 terms: launch groups of whole products, one after the other on s
static int prod_launch(pbc_hip_pp_set_s *set, void *d_gt, const void *d_g2, size_t n, hipStream_t s, const OwnWs *own) {
  pbc_hip_pairing_s *P = set->P;
  const size_t per = std::max<size_t>(1, kProdGroupTerms / set->m);
  for (size_t u0 = 0; u0 < n; u0 += per)
    if (prod_group(set, (uint8_t *) d_gt + u0 * (size_t) P->lenT, (const uint8_t *) d_g2 + u0 * set->m * (size_t) P->len2, std::min(per, n - u0), s, own)) return 1;
  return 0;
}
static int prod_check_args(const pbc_hip_pp_set_s *set, const void *gt, const void *g2, size_t n) {
  if (!set) return fail("null pp set");
  if (!n) return 0;
  if (!gt || !g2) return fail("null argument");
  if (n > SIZE_MAX / (set->m * (size_t) set->P->len2)) return fail("pairing_pp_set_prod: %zu products of %zu terms overflow size_t", n, set->m);
  return 0;
}
extern "C" int pbc_hip_pairing_pp_set_prod_batch_dev(pbc_hip_pp_set_t *set, void *d_gt, const void *d_g2, size_t n, void *stream) {
  if (prod_check_args(set, d_gt, d_g2, n)) return 1;
  if (!n) return 0;
  if (ensure_derived(set->P, (hipStream_t) stream)) return 1;
  return prod_launch(set, d_gt, d_g2, n, (hipStream_t) stream, nullptr);
}
extern "C" int pbc_hip_pairing_pp_set_prod_batch(pbc_hip_pp_set_t *set, uint8_t *gt, const uint8_t *g2, size_t n) {
  if (prod_check_args(set, gt, g2, n)) return 1;
  if (!n) return 0;
  pbc_hip_pairing_s *P = set->P;
  const size_t chunk = std::max<size_t>(1, (P->host_chunk ? P->host_chunk : (size_t) 1 << 20) / set->m);     // (terms per chunk, as the ragged call)
  return run_host_own_device(P, gt, (size_t) P->lenT, g2, set->m * (size_t) P->len2, n, chunk,
                             [set](void *d_out, const void *d_in, size_t, size_t cnt, hipStream_t s, const OwnWs *own) {
                               return prod_launch(set, d_out, d_in, cnt, s, own);
                             });
}
