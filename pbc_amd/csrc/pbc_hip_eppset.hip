// pbc_hip_eppset.hip -- sets of fixed-base tables on G1, G2 and GT: many tables of element_pp_init in one object, one
// launch to build them, one call to raise them segment by segment or as the fixed bases of a batch of multi-base powers
// (include/pbc_hip.h pbc_hip_element_pp_set_*; lane bodies: group_ppset.cuh): libpbc_hip.so; see host_common.h
#include "host_common.h"
#include "group_ppset.cuh"

// ---- building the set: one entry per lane ------------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(kBlock, 2) eppset_ec_init_kernel(uint32_t *tabs, uint8_t *flags, const uint8_t *bases, int zlen, size_t units, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= units) return;
  ec_pp_set_entry_lane<F>(tabs, flags, bases, zlen, idx);
}
template <class G>
__global__ void __launch_bounds__(kBlock, 2) eppset_gt_init_kernel(uint32_t *tabs, const uint8_t *bases, int zlen, size_t units, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= units) return;
  gt_pp_set_entry_lane<G>(tabs, bases, zlen, idx);
}
// ---- segmented powers: lane idx works on unit u0 + idx of the call (records idx of out / z), its table from the offsets
// tflags[t] != 0: table t is "complete only" -- its units are reported without a look at the table
template <class F>
__global__ void __launch_bounds__(kBlock, 2) eppset_ec_pow_kernel(uint8_t *out, const uint32_t *__restrict__ tabs, const uint8_t *z, int zlen, const uint64_t *__restrict__ offsets,
                                                                   size_t m, const uint8_t *__restrict__ tflags, uint8_t *flags, size_t u0, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t t = pp_set_table_of(offsets, m, u0 + idx), L = 2 * (size_t) F::bytes();
  if (tflags[t]) { flags[idx] = 1; return; }
  flags[idx] = ec_pp_pow_lane<F>(out + idx * L, tabs + t * ec_pp_table_words<F>(zlen), z + idx * (size_t) zlen, zlen) ? 0 : 1;
}
// the complete ladder on the unit's own base (flags == null: every unit -- "hip_group_slow 1")
template <class F>
__global__ void __launch_bounds__(kBlock, 2) eppset_ec_mul_kernel(uint8_t *out, const uint8_t *bases, const uint8_t *z, int zlen, const uint64_t *__restrict__ offsets, size_t m,
                                                                   const uint8_t *flags, size_t u0, size_t n, KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  if (flags && !flags[idx]) return;
  const size_t t = pp_set_table_of(offsets, m, u0 + idx), L = 2 * (size_t) F::bytes();
  ec_mul_lane<F>(out + idx * L, bases + t * L, z + idx * (size_t) zlen, zlen);
}
template <class G>
__global__ void __launch_bounds__(kBlock, 2) eppset_gt_pow_kernel(uint8_t *out, const uint32_t *__restrict__ tabs, const uint8_t *z, int zlen, const uint64_t *__restrict__ offsets,
                                                                   size_t m, size_t u0, size_t n, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t t = pp_set_table_of(offsets, m, u0 + idx);
  gt_pp_pow_lane<G>(out + idx * (size_t) G::bytes(), tabs + t * gt_pp_table_words<G>(zlen), z + idx * (size_t) zlen, zlen);
}
// ---- multi-base powers: unit idx holds m scalars --------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(kBlock, 2) eppset_ec_prod_kernel(uint8_t *out, const uint32_t *__restrict__ tabs, size_t m, const uint8_t *z, int zlen, uint8_t *flags, size_t n,
                                                                    KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  const size_t L = 2 * (size_t) F::bytes();
  flags[idx] = ec_pp_set_prod_lane<F>(out + idx * L, tabs, m, z + idx * m * (size_t) zlen, zlen) ? 0 : 1;
}
template <class F>
__global__ void __launch_bounds__(kBlock, 2) eppset_ec_prod_complete_kernel(uint8_t *out, const uint8_t *bases, size_t m, const uint8_t *z, int zlen, const uint8_t *flags, size_t n,
                                                                             KArgs<F::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  if (flags && !flags[idx]) return;
  const size_t L = 2 * (size_t) F::bytes();
  ec_pp_set_prod_complete_lane<F>(out + idx * L, bases, m, z + idx * m * (size_t) zlen, zlen);
}
template <class G>
__global__ void __launch_bounds__(kBlock, 2) eppset_gt_prod_kernel(uint8_t *out, const uint32_t *__restrict__ tabs, size_t m, const uint8_t *z, int zlen, size_t n, KArgs<G::NW> ka) {
  size_t idx = (size_t) blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  gt_pp_set_prod_lane<G>(out + idx * (size_t) G::bytes(), tabs, m, z + idx * m * (size_t) zlen, zlen);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static bool symmetric(const pbc_hip_pairing_s *P) { return P->type == 'a' || P->type == '1' || P->type == 'e'; }
// F = the field policy of group 1 / 2, G = GT as a field policy (as pbc_hip_group.hip)
#define PBC_DISPATCH_EPP(P_, group_, ...)                                                      \
  do {                                                                                         \
    if ((group_) == 2 && !symmetric(P_)) PBC_DISPATCH_TWIST(P_, __VA_ARGS__);                  \
    else { PBC_DISPATCH_N((P_)->nlimb, { typedef FqOps<N> F; __VA_ARGS__; }); }                \
  } while (0)
#define PBC_DISPATCH_EPP_GT(P_, ...)                                                           \
  do {                                                                                         \
    if ((P_)->type == 'a' || (P_)->type == '1') { if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if ((P_)->type == 'e') { if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if ((P_)->type == 'f') { PBC_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); } \
    else { PBC_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                      \
  } while (0)

// m tables in ONE allocation: the tables (table t: tabs + t tab_words, the words pbc_hip_element_pp_init derives from
// base t), one "is O" byte per entry of the curve groups as the table kernel left it, one "complete only" byte per table
// (the OR of its entry bytes: made on the host before the first call that needs it, ensure_flags), the m base records
struct pbc_hip_element_pp_set_s {
  pbc_hip_pairing_s *P;
  int group, device;
  size_t m, tab_words, per, lrec;      // per: entries of one table
  void *mem;
  uint32_t *tabs;
  uint8_t *eflags, *tflags, *bases;
  hipEvent_t built;                    // recorded behind the table kernel
  std::mutex mu;
  bool flags_ready, any_complete;      // any_complete: some table is "complete only"
};
static size_t ws_round(size_t b) { return (b + 255) & ~(size_t) 255; }
static size_t rec_len(const pbc_hip_pairing_s *P, int group) { return (size_t) (group == 3 ? P->lenT : group == 2 ? P->len2 : P->len1); }

// the per-table flags, on the host and in the set's allocation: once, before the first call that uses them
static int ensure_flags(pbc_hip_element_pp_set_s *set) {
  std::lock_guard<std::mutex> lock(set->mu);
  if (set->flags_ready) return 0;
  DeviceGuard guard(set->device);
  HIP_TRY(hipEventSynchronize(set->built));
  std::vector<uint8_t> ef(set->m * set->per), tf(set->m, 0);
  HIP_TRY(hipMemcpy(ef.data(), set->eflags, ef.size(), hipMemcpyDeviceToHost));
  for (size_t t = 0; t < set->m; t++)
    for (size_t e = 0; e < set->per; e++) tf[t] |= ef[t * set->per + e] != 0;
  for (uint8_t f : tf) set->any_complete |= f != 0;
  HIP_TRY(hipMemcpy(set->tflags, tf.data(), tf.size(), hipMemcpyHostToDevice));
  set->flags_ready = true;
  return 0;
}

// argument checks first, then the device: the checks run without a GPU
static int set_create(pbc_hip_element_pp_set_t **out, pbc_hip_pairing_s *P, int group, const void *bases, size_t m, bool from_device, hipStream_t s) {
  if (!out || !P || !bases) return fail("null argument");
  if (group < 1 || group > 3) return fail("element_pp_set_init: group must be 1, 2 or 3 (GT)");
  if (!m) return fail("element_pp_set_init: a set holds at least one table (m == 0)");
  size_t words_el = 0;
  if (group == 3) PBC_DISPATCH_EPP_GT(P, words_el = G::WORDS_EL);
  else PBC_DISPATCH_EPP(P, group, words_el = F::WORDS_EL);
  const size_t rows = (size_t) P->len_zr, lrec = rec_len(P, group);
  const size_t per = group == 3 ? rows << kPpWin : rows * kPpRowLen;
  const size_t tab_words = per * words_el * (group == 3 ? 1 : 2);
  if (m > (SIZE_MAX - 4096) / (tab_words * 4 + per + 1 + lrec))
    return fail("element_pp_set_init: %zu tables of %zu bytes overflow size_t", m, tab_words * 4);
  if (P->device < 0) return fail("no HIP device: libpbc_hip has no CPU fallback");
  DeviceGuard guard(P->device);        // the set lives on the device the pairing object was created on, whatever is current
  if (ensure_derived(P, s)) return 1;
  const size_t off_ef = ws_round(m * tab_words * 4), off_tf = off_ef + ws_round(m * per), off_b = off_tf + ws_round(m), total = off_b + m * lrec;
  void *mem = nullptr;
  if (hipMalloc(&mem, total) != hipSuccess) { (void) hipGetLastError(); return fail("element_pp_set_init: device allocation of %zu bytes failed", total); }
  uint8_t *b = (uint8_t *) mem;
  pbc_hip_element_pp_set_s *set = new pbc_hip_element_pp_set_s{P, group, P->device, m, tab_words, per, lrec, mem, (uint32_t *) mem, b + off_ef, b + off_tf, b + off_b,
                                                               nullptr, {}, group == 3, false};
  auto bail = [&](const char *what, hipError_t e) {
    if (set->built) (void) hipEventDestroy(set->built);
    (void) hipFree(mem);
    delete set;
    return e == hipSuccess ? fail("element_pp_set_init: %s", what) : fail("element_pp_set_init: %s (%s)", what, hipGetErrorString(e));
  };
  hipError_t e = hipEventCreateWithFlags(&set->built, hipEventDisableTiming);
  if (e != hipSuccess) { set->built = nullptr; return bail("no event", e); }
  e = from_device ? hipMemcpyAsync(set->bases, bases, m * lrec, hipMemcpyDeviceToDevice, s) : hipMemcpy(set->bases, bases, m * lrec, hipMemcpyHostToDevice);
  if (e != hipSuccess) return bail("copying the base records failed", e);
  if ((e = hipMemsetAsync(set->tflags, 0, m, s)) != hipSuccess) return bail("clearing the flags failed", e);
  const size_t units = m * per;
  if ((units + kBlock - 1) / kBlock > 0x7fffffffu) return bail("too many table entries for one launch", hipSuccess);
  const unsigned grid = (unsigned) ((units + kBlock - 1) / kBlock);
  auto launch = [&]() -> int {
    if (group == 3) PBC_DISPATCH_EPP_GT(P, hipLaunchKernelGGL(eppset_gt_init_kernel<G>, dim3(grid), dim3(kBlock), 0, s, set->tabs, (const uint8_t *) set->bases, P->len_zr, units, kargs<G::NW>(P)));
    else PBC_DISPATCH_EPP(P, group, hipLaunchKernelGGL(eppset_ec_init_kernel<F>, dim3(grid), dim3(kBlock), 0, s, set->tabs, set->eflags, (const uint8_t *) set->bases, P->len_zr, units, kargs<F::NW>(P)));
    return 0;
  };
  if (launch() || hipGetLastError() != hipSuccess) return bail("the table kernel could not be launched", hipSuccess);
  if ((e = hipEventRecord(set->built, s)) != hipSuccess) return bail("recording the event failed", e);
  if (!from_device) {
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail("the table kernel failed", e);
    if (ensure_flags(set)) { const std::string why = pbc_hip_last_error(); return bail(why.c_str(), hipSuccess); }    // (a copy: fail() writes the buffer it would read)
  }
  *out = set;
  return 0;
}
extern "C" int pbc_hip_element_pp_set_init(pbc_hip_element_pp_set_t **out, pbc_hip_pairing_t *P, int group, const uint8_t *bases, size_t m) {
  return set_create(out, P, group, bases, m, false, 0);
}
extern "C" int pbc_hip_element_pp_set_init_dev(pbc_hip_element_pp_set_t **out, pbc_hip_pairing_t *P, int group, const void *d_bases, size_t m, void *stream) {
  return set_create(out, P, group, d_bases, m, true, (hipStream_t) stream);
}
extern "C" void pbc_hip_element_pp_set_clear(pbc_hip_element_pp_set_t *set) {
  if (!set) return;
  DeviceGuard guard(set->device);
  (void) hipFree(set->mem);            // (waits for the kernels that still read the tables)
  (void) hipEventDestroy(set->built);
  delete set;
}
extern "C" size_t pbc_hip_element_pp_set_count(const pbc_hip_element_pp_set_t *set) { return set ? set->m : 0; }

// ---- segmented powers --------------------------------------------------------------------------------------------------
// The offsets of a call on their way to the device: the second buffer of the (device, stream) workspace, ONE
// stream-ordered copy from the workspace's page-locked staging -- behind the kernels of an earlier call on this stream,
// which still read THEIR offsets from the same bytes (pbc_hip_ppset.hip plan_upload)
static const uint64_t *offsets_upload(ProdWs &W, const uint64_t *offsets, size_t m, hipStream_t s) {
  const size_t bytes = (m + 1) * sizeof(uint64_t);
  void *buf = W.get2(bytes);
  if (!buf) return nullptr;
  HostStage *hs = W.stage();
  if (!hs) { fail("internal: a table-set launch without host staging"); return nullptr; }
  void *h = stage_acquire(*hs, bytes);
  if (!h) return nullptr;
  memcpy(h, offsets, bytes);
  if (hipMemcpyAsync(buf, h, bytes, hipMemcpyHostToDevice, s) != hipSuccess) { fail("uploading the offsets failed"); return nullptr; }
  if (stage_copied(*hs, s)) return nullptr;
  return (const uint64_t *) buf;
}
// the units c0 <= u < c0 + n of a call (device pointers to unit c0's records), constants derived, flags read back
static int pow_launch(pbc_hip_element_pp_set_s *set, void *d_out, const void *d_zr, const uint64_t *offsets, size_t c0, size_t n, hipStream_t s, const OwnWs *own) {
  pbc_hip_pairing_s *P = set->P;
  if (!n) return 0;
  uint8_t *o = (uint8_t *) d_out;
  const uint8_t *z = (const uint8_t *) d_zr;
  const unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  const size_t m = set->m;
  ProdWs W(P, s, own);
  uint8_t *flags = nullptr;
  if (set->group != 3 && !P->group_slow && !(flags = (uint8_t *) W.get(n))) return 1;
  const uint64_t *offs = offsets_upload(W, offsets, m, s);
  if (!offs) return 1;
  if (set->group == 3) {
    PBC_DISPATCH_EPP_GT(P, hipLaunchKernelGGL(eppset_gt_pow_kernel<G>, dim3(grid), dim3(kBlock), 0, s, o, (const uint32_t *) set->tabs, z, P->len_zr, offs, m, c0, n, kargs<G::NW>(P)));
  } else {
    PBC_DISPATCH_EPP(P, set->group, {
      if (flags) hipLaunchKernelGGL(eppset_ec_pow_kernel<F>, dim3(grid), dim3(kBlock), 0, s, o, (const uint32_t *) set->tabs, z, P->len_zr, offs, m, (const uint8_t *) set->tflags, flags, c0, n, kargs<F::NW>(P));
      hipLaunchKernelGGL(eppset_ec_mul_kernel<F>, dim3(grid), dim3(kBlock), 0, s, o, (const uint8_t *) set->bases, z, P->len_zr, offs, m, (const uint8_t *) flags, c0, n, kargs<F::NW>(P));
    });
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
static int offsets_check(const uint64_t *offsets, size_t m) {
  if (offsets[0] != 0) return fail("element_pp_set_pow_zn: offsets[0] must be 0 (got %llu)", (unsigned long long) offsets[0]);
  for (size_t t = 0; t < m; t++)
    if (offsets[t] > offsets[t + 1])
      return fail("element_pp_set_pow_zn: offsets decrease at index %zu (%llu > %llu)", t, (unsigned long long) offsets[t], (unsigned long long) offsets[t + 1]);
  return 0;
}
static int pow_check_args(const pbc_hip_element_pp_set_s *set, const void *out, const void *zr, const uint64_t *offsets) {
  if (!set) return fail("null element_pp set");
  if (!out || !zr || !offsets) return fail("null argument");
  return offsets_check(offsets, set->m);
}
// the check of a call's offsets alone, as the two entry points below make it (a set needs a device, this does not)
extern "C" int pbc_hip_diag_element_pp_set_offsets(const uint64_t *offsets, size_t m) {
  if (!offsets) return fail("null argument");
  if (!m) return fail("element_pp_set_init: a set holds at least one table (m == 0)");
  return offsets_check(offsets, m);
}
extern "C" int pbc_hip_element_pp_set_pow_zn_batch_dev(pbc_hip_element_pp_set_t *set, void *d_out, const void *d_zr, const uint64_t *offsets, void *stream) {
  if (pow_check_args(set, d_out, d_zr, offsets)) return 1;
  const uint64_t n = offsets[set->m];
  if (!n) return 0;
  if (ensure_derived(set->P, (hipStream_t) stream) || ensure_flags(set)) return 1;
  return pow_launch(set, d_out, d_zr, offsets, 0, (size_t) n, (hipStream_t) stream, nullptr);
}
extern "C" int pbc_hip_element_pp_set_pow_zn_batch(pbc_hip_element_pp_set_t *set, uint8_t *out, const uint8_t *zr, const uint64_t *offsets) {
  if (pow_check_args(set, out, zr, offsets)) return 1;
  const uint64_t n = offsets[set->m];
  if (!n) return 0;
  pbc_hip_pairing_s *P = set->P;
  if (ensure_flags(set)) return 1;
  const size_t chunk = P->host_chunk ? P->host_chunk : (size_t) 1 << 20;
  return run_host_own_device(P, out, set->lrec, zr, (size_t) P->len_zr, (size_t) n, chunk,
                             [set, offsets](void *d_out, const void *d_in, size_t c0, size_t cnt, hipStream_t s, const OwnWs *own) {
                               return pow_launch(set, d_out, d_in, offsets, c0, cnt, s, own);
                             });
}

// ---- multi-base powers -----------------------------------------------------------------------------------------------
// n units on stream s (device pointers); a set with a "complete only" table and "hip_group_slow 1": the complete lane alone
static int prod_launch(pbc_hip_element_pp_set_s *set, void *d_out, const void *d_zr, size_t n, hipStream_t s, const OwnWs *own) {
  pbc_hip_pairing_s *P = set->P;
  if (!n) return 0;
  uint8_t *o = (uint8_t *) d_out;
  const uint8_t *z = (const uint8_t *) d_zr;
  const unsigned grid = (unsigned) ((n + kBlock - 1) / kBlock);
  const size_t m = set->m;
  if (set->group == 3) {
    PBC_DISPATCH_EPP_GT(P, hipLaunchKernelGGL(eppset_gt_prod_kernel<G>, dim3(grid), dim3(kBlock), 0, s, o, (const uint32_t *) set->tabs, m, z, P->len_zr, n, kargs<G::NW>(P)));
  } else {
    ProdWs W(P, s, own);
    uint8_t *flags = nullptr;
    if (!set->any_complete && !P->group_slow && !(flags = (uint8_t *) W.get(n))) return 1;
    PBC_DISPATCH_EPP(P, set->group, {
      if (flags) hipLaunchKernelGGL(eppset_ec_prod_kernel<F>, dim3(grid), dim3(kBlock), 0, s, o, (const uint32_t *) set->tabs, m, z, P->len_zr, flags, n, kargs<F::NW>(P));
      hipLaunchKernelGGL(eppset_ec_prod_complete_kernel<F>, dim3(grid), dim3(kBlock), 0, s, o, (const uint8_t *) set->bases, m, z, P->len_zr, (const uint8_t *) flags, n, kargs<F::NW>(P));
    });
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
static int prod_check_args(const pbc_hip_element_pp_set_s *set, const void *out, const void *zr, size_t n) {
  if (!set) return fail("null element_pp set");
  if (!n) return 0;
  if (!out || !zr) return fail("null argument");
  if (n > SIZE_MAX / (set->m * (size_t) set->P->len_zr) || n > SIZE_MAX / set->lrec || (n + kBlock - 1) / kBlock > 0x7fffffffu)
    return fail("element_pp_set_prod: %zu units of %zu scalars overflow size_t", n, set->m);
  return 0;
}
extern "C" int pbc_hip_element_pp_set_prod_batch_dev(pbc_hip_element_pp_set_t *set, void *d_out, const void *d_zr, size_t n, void *stream) {
  if (prod_check_args(set, d_out, d_zr, n)) return 1;
  if (!n) return 0;
  if (ensure_derived(set->P, (hipStream_t) stream) || ensure_flags(set)) return 1;
  return prod_launch(set, d_out, d_zr, n, (hipStream_t) stream, nullptr);
}
extern "C" int pbc_hip_element_pp_set_prod_batch(pbc_hip_element_pp_set_t *set, uint8_t *out, const uint8_t *zr, size_t n) {
  if (prod_check_args(set, out, zr, n)) return 1;
  if (!n) return 0;
  pbc_hip_pairing_s *P = set->P;
  if (ensure_flags(set)) return 1;
  const size_t chunk = std::max<size_t>(1, (P->host_chunk ? P->host_chunk : (size_t) 1 << 20) / set->m);     // (scalars per chunk)
  return run_host_own_device(P, out, set->lrec, zr, set->m * (size_t) P->len_zr, n, chunk,
                             [set](void *d_out, const void *d_in, size_t, size_t cnt, hipStream_t s, const OwnWs *own) {
                               return prod_launch(set, d_out, d_in, cnt, s, own);
                             });
}
