// host_common.h -- what the translation units of libpbc_hip.so share: launch geometry, the dispatch over the built-in
// field widths, the constant block of a launch, and the functions that cross translation units.  The library is built
// from one .hip file per pairing family (pbc_hip_a.hip: types a, a1, e; pbc_hip_d.hip: types d, g; pbc_hip_f.hip: type f),
// one for the group operations (pbc_hip_group.hip) and pbc_hip.hip (the C-ABI, the host-buffer path, text formats,
// probes), compiled in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pbc_hip.h"
#include "fp.cuh"
#include "hostbn.h"
#include "pairing_a.cuh"
#include "pairing_al.cuh"
#include "pairing_d.cuh"
#include "pairing_f.cuh"
#include "pairing_e.cuh"
#include "group_al.cuh"
#include "group_l5.cuh"

using namespace pbc;

#include "host_params.h"
#include "ragged_plan.h"
#include "pp_set_plan.h"

#define HIP_TRY(x)                                                                   \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) return fail("%s: %s", #x, hipGetErrorString(e_));          \
  } while (0)

// device allocation released on every return path
struct DevBuf {
  void *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void) hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};
// the calling thread's current device is restored on every return path (callers such as torch keep their own)
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (dev >= 0 && dev != prev) (void) hipSetDevice(dev);
  }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
  ~DeviceGuard() { if (prev >= 0) (void) hipSetDevice(prev); }
};

// ---------------------------------------------------------------------------------------
// launch geometry
// ---------------------------------------------------------------------------------------
constexpr int kBlock = 128;
#ifndef PBC_HIP_ZERO_COPY_DEFAULT
#define PBC_HIP_ZERO_COPY_DEFAULT 1
#endif
// Resident workgroups (the 5-word type f kernel).  The kernel is launched with at most as many workgroups as the chip
// holds at once (resident_grid below) and every workgroup walks the batch in strides of the grid: a lane runs its pairings
// one after the other.  With one workgroup per 128 units the dispatcher refills the CUs round by round, and with 36 KB of
// LDS per workgroup the rounds do not pack: a few workgroups find their LDS slot taken and wait for the NEXT round, so a
// 2^18 batch (two rounds of 1024 workgroups) takes three (tools/occ_schedule_probe.hip: mean residency 1.4 waves per SIMD; a
// single wave gets a multiply-add through only every 9.1 cycles, two share the pipe at 4.6).  All control flow is
// data-independent, so equal shares finish together.  Measured on the other kernels (types a, d, products,
// preprocessed pairings: 8 or more rounds, or LDS to spare): 3 - 4 % SLOWER than one workgroup per 128 units -- they keep
// the plain grid (profiles/r03_notes.md).
// Which 64-unit block a wave works on next: a fixed stride over the grid (ctr == null; iteration `it` of workgroup b's wave w
// takes block (b + it gridDim) 2 + w -- lane t of the workgroup works on unit (b + it gridDim) 128 + t), or the next value
// of a per-launch counter ("hip_dynamic 1": waves that finish early fetch more; control flow stays data-independent).
static __device__ __forceinline__ size_t pbc_unit_block(unsigned *ctr, size_t it) {
  unsigned v;
  if (ctr) {
    v = 0;
    if ((threadIdx.x & 63) == 0) v = atomicAdd(ctr, 1u);
  } else {
    v = (unsigned) (((size_t) blockIdx.x + it * gridDim.x) * (kBlock / 64) + (threadIdx.x >> 6));
  }
  return (size_t) (unsigned) __builtin_amdgcn_readfirstlane((int) v);
}
#define PBC_RESIDENT_LOOP(n, ctr) for (size_t it_ = 0, nvb_ = ((n) + 63) / 64, vb = pbc_unit_block(ctr, 0); vb < nvb_; vb = pbc_unit_block(ctr, ++it_))
#define PBC_UNIT_INDEX (vb * 64 + (threadIdx.x & 63))
// One wave slot of a table-set plan (pp_set_plan.h; the kernels *_pp_set_*): descriptor `slot` of `plan`, every field
// made wave-uniform, so that the table pointer derived from it stays in scalar registers (the apply lanes convert the
// table's words on the scalar unit).  rec(): the record a lane works on -- lanes at or beyond `count` are clamped to the
// slot's last unit and store nothing, the `ld` clamp of the other kernels.  stride / tmul: 1 / 0 for a segmented apply
// (unit i is record i); m / 1 for a product over the set (unit u of table j is term record u m + j).
struct PpSlot {
  size_t table, first;
  unsigned count;
  __device__ __forceinline__ bool live() const { return (threadIdx.x & 63) < count; }
  __device__ __forceinline__ size_t rec(size_t stride, size_t tmul) const {
    const unsigned lane = threadIdx.x & 63;
    return (first + (lane < count ? lane : count - 1)) * stride + table * tmul;
  }
};
static __device__ __forceinline__ uint64_t pbc_uniform64(uint64_t v) {
  const uint32_t lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) v), hi = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) (v >> 32));
  return ((uint64_t) hi << 32) | lo;
}
static __device__ __forceinline__ PpSlot pp_set_slot(const uint64_t *__restrict__ plan, size_t slot) {
  const uint64_t *d = plan + slot * pbc_host::kPpSetSlotWords;
  PpSlot s;
  s.table = (size_t) pbc_uniform64(d[0]);
  s.first = (size_t) pbc_uniform64(d[1]);
  s.count = (unsigned) pbc_uniform64(d[2]);
  return s;
}
static_assert(kBlock == D_LANES, "pairing_d.cuh sizes its LDS state for 128-lane workgroups");
#ifndef PBC_DF_WAVES
#define PBC_DF_WAVES 2
#endif
#ifndef PBC_A_WAVES
#define PBC_A_WAVES 2     // waves per SIMD the pairing kernels are register-budgeted for (measured: 1 -> 2 = +32 %)
#endif
#ifndef PBC_A1_WAVES
#define PBC_A1_WAVES 2    // 33-word fields.  Rounds 1-4 ran them at one wave per SIMD (512 registers; with the products in
#endif                    // registers two waves spilled: a1 158 k -> 119 k pairings/s).  On memory operands the product
                          // bodies need 121-248 registers and a second wave is what keeps the multiply-add pipe fed
                          // (profiles/r05_ab_wide.txt; 256-lane workgroups, pbc_hip_a.hip kWide)
#ifndef PBC_F_WAVES
#define PBC_F_WAVES PBC_DF_WAVES
#endif

// Type D / G kernels exist per (field width, d); N and DEG are compile-time inside the expression
#define PBC_DISPATCH_D(P_, ...)                                                        \
  switch ((P_)->nlimb * 8 + (P_)->deg) {                                               \
    case 5 * 8 + 3: { constexpr int N = 5, DEG = 3; __VA_ARGS__; } break;              \
    case 6 * 8 + 3: { constexpr int N = 6, DEG = 3; __VA_ARGS__; } break;              \
    case 7 * 8 + 3: { constexpr int N = 7, DEG = 3; __VA_ARGS__; } break;              \
    case 5 * 8 + 5: { constexpr int N = 5, DEG = 5; __VA_ARGS__; } break;              \
    default: return fail("internal: no type d/g kernel for %d-word fields, degree %d", (P_)->nlimb, (P_)->deg); \
  }

// type f kernels: 5-word (f.param) and 8-word (256-bit BN) fields
#define PBC_DISPATCH_F(nl, ...)                               \
  switch (nl) {                                               \
    case 5: { constexpr int N = 5; __VA_ARGS__; } break;      \
    case 8: { constexpr int N = 8; __VA_ARGS__; } break;      \
    default: return fail("internal: no type f kernel for %d-word fields", (int) (nl)); \
  }
// any built-in field width (PBC_FOR_EACH_N)
#define PBC_DISPATCH_N(nl, ...)                               \
  switch (nl) {                                               \
    case 5: { constexpr int N = 5; __VA_ARGS__; } break;             \
    case 6: { constexpr int N = 6; __VA_ARGS__; } break;             \
    case 7: { constexpr int N = 7; __VA_ARGS__; } break;             \
    case 8: { constexpr int N = 8; __VA_ARGS__; } break;             \
    case 16: { constexpr int N = 16; __VA_ARGS__; } break;           \
    case 33: { constexpr int N = 33; __VA_ARGS__; } break;           \
    default: return fail("internal: no kernel for %d-word fields", (int) (nl)); \
  }

// the constant block of an object, passed by value as the LAST argument of every kernel (fp.cuh, "KArgs")
template <int N>
static KArgs<N> kargs(const pbc_hip_pairing_s *P, bool for_pairing = false, bool no_fair = false) {
  KArgs<N> K;
  fill_kargs<N>(P, K, for_pairing);
  if (no_fair) { const uint32_t opt = 1u; memcpy(K.head + KOFF_OPT, &opt, 4); }    // this launch without time-sliced priorities
  return K;
}


// F = field policy of the G2 twist of an asymmetric type
#define PBC_DISPATCH_TWIST(P_, ...)                                                           \
  do {                                                                                        \
    if ((P_)->type == 'f') { PBC_DISPATCH_F((P_)->nlimb, { typedef Fq2Ops<N> F; __VA_ARGS__; }); } \
    else { PBC_DISPATCH_D(P_, { typedef FdOps<N, DEG> F; __VA_ARGS__; }); }                   \
  } while (0)

// ---------------------------------------------------------------------------------------
// functions that cross translation units
// ---------------------------------------------------------------------------------------
// pbc_hip.hip
int ensure_derived(pbc_hip_pairing_s *P, hipStream_t s);        // self-test + device-side derivation of an object's constants, once
unsigned resident_grid(const pbc_hip_pairing_s *P, const void *kernel, size_t n);
unsigned *unit_counter(pbc_hip_pairing_s *P, hipStream_t s);   // "hip_dynamic 1": a zeroed per-launch counter (enqueued on s); null otherwise
#define PBC_RGRID(...) resident_grid(P, reinterpret_cast<const void *>(&__VA_ARGS__), n)
void *pinned_dev_ptr(const void *host, size_t bytes, bool shared);
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb);
void *workspace_get(pbc_hip_pairing_s *P, hipStream_t s, size_t bytes, int part = 0);   // part 1: the entry's second buffer (ProdWs::get2)
void workspace_unpin(pbc_hip_pairing_s *P, hipStream_t s);
// A workspace that belongs to one stream of a device context of the host-buffer path: grown on demand, freed with the context.
// Page-locked host staging that belongs to a workspace (ragged products: the plan of a call on its way to the device).
// An asynchronous copy reads it after the call has returned, so the next call waits for THAT COPY -- not for the
// kernels behind it -- before it writes: `ev` is recorded right behind the copy.
struct HostStage { void *h = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; };
void *stage_acquire(HostStage &st, size_t bytes);      // at least `bytes`, no copy in flight (grown on demand; null: fail() was called)
int stage_copied(HostStage &st, hipStream_t s);        // call right after enqueueing the copy that reads the staging
void stage_free(HostStage &st);
struct OwnWs { void **p; size_t *cap; void **p2; size_t *cap2; HostStage *stage = nullptr; };     // (p2 / cap2: the second buffer, ProdWs::get2)
HostStage *workspace_stage(pbc_hip_pairing_s *P, hipStream_t s);   // the staging of the PINNED table entry of (current device, s)
void *own_workspace(const OwnWs &o, hipStream_t s, size_t bytes);
void *object_scratch(pbc_hip_pairing_s *P, const void *key, size_t bytes, bool *fresh);    // small per-(device, key) buffers the object keeps (pbc_hip.hip)
// The workspace of one product launch: the caller's own (host-buffer path) or the object's table entry for (device,
// stream), which stays pinned until the launch's kernels are enqueued (the destructor unpins).
struct ProdWs {
  pbc_hip_pairing_s *P;
  hipStream_t s;
  const OwnWs *own;
  bool pinned = false;
  ProdWs(pbc_hip_pairing_s *P_, hipStream_t s_, const OwnWs *own_) : P(P_), s(s_), own(own_) {}
  ProdWs(const ProdWs &) = delete;
  ProdWs &operator=(const ProdWs &) = delete;
  ~ProdWs() { if (pinned) workspace_unpin(P, s); }
  void *get(size_t bytes) {
    if (own) return own_workspace(*own, s, bytes);
    void *w = workspace_get(P, s, bytes);      // pins the entry and takes its issue lock (pbc_hip.hip WsEnt)
    if (w && pinned) workspace_unpin(P, s);    // a second request of the same call: one pin, one lock level
    pinned = pinned || w != nullptr;
    return w;
  }
  // A second buffer of the same workspace, for a call that keeps intermediates of its own ACROSS a launcher that asks
  // get() for what its kernels need (is_almost_coddh: the GT records of its 2 n pairings): the two requests must not
  // share bytes, and a launcher's request may grow -- move -- the first buffer.  Same entry, same pin, same issue lock.
  void *get2(size_t bytes) {
    if (own) { const OwnWs second = {own->p2, own->cap2, nullptr, nullptr}; return own_workspace(second, s, bytes); }
    void *w = workspace_get(P, s, bytes, 1);
    if (w && pinned) workspace_unpin(P, s);
    pinned = pinned || w != nullptr;
    return w;
  }
  // the workspace's host staging (after get / get2: the table entry is pinned and its issue lock held)
  HostStage *stage() { return own ? own->stage : (pinned ? workspace_stage(P, s) : nullptr); }
};
// One call's digit string on its way to the device (pbc_hip_mpz.hip): the workspace's second buffer, one stream-ordered
// copy from its page-locked staging; `rec` (may be empty): bytes that travel behind the digits (*rec_at).  Null: fail() was called
const uint32_t *digits_upload(ProdWs &W, const std::vector<int8_t> &dig, const std::vector<uint8_t> &rec, const uint8_t **rec_at, hipStream_t s);
// The host-buffer path (pbc_hip.hip): chunks over the device set, page-locked buffers in place, anything else staged
// through per-device chunk buffers that the object keeps.  `launch` enqueues one chunk (device pointers) on a stream.
typedef std::function<int(void *d_out, const void *d_a, const void *d_b, size_t m, hipStream_t s, const OwnWs *own)> ChunkLaunch;
int run_host_generic(pbc_hip_pairing_s *P, uint8_t *out, size_t ut, const uint8_t *a, size_t u1, const uint8_t *b, size_t u2,
                     size_t n, const ChunkLaunch &launch, bool zero_copy_ok);
// n single pairings on stream s through the launch path of element_pairing_batch (pbc_hip.hip launch_prod, k = 1: wave
// routes and lane kernels are chosen there); constants already derived
int launch_pairings(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, hipStream_t s, const OwnWs *own);
// Ragged products (pbc_hip_ragged.hip): n products on stream s, product u = terms offsets[u] - offsets[0] .. of the
// device arrays (offsets: HOST memory, n + 1 values, checked by the caller; read before the call returns)
int ragged_launch(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, const uint64_t *offsets, size_t n,
                  hipStream_t s, const OwnWs *own);
// ... over host buffers (pbc_hip.hip): contiguous ranges of products, balanced by terms, over the device set
int run_host_ragged(pbc_hip_pairing_s *P, uint8_t *gt, const uint8_t *g1, const uint8_t *g2, const uint64_t *offsets, size_t n);
// The record route of the 512-bit type a (pbc_hip_a.hip): Miller records of the T terms, folds, finish.  d_plan: the
// level arrays on the device (each n + 1 values), sizes[i] = records of level i; recA / recB: room for sizes[0] / sizes[1] records
int ragged_records_a(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, unsigned F,
                     const uint64_t *const *d_plan, const size_t *sizes, int nlevels, void *recA, void *recB, hipStream_t s);
// Per-family launchers: k-term products (k = 1: single pairings) of n units on stream s; constants already derived.
int launch_a(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, hipStream_t s, ProdWs &W);   // pbc_hip_a.hip: a, a1, e
int launch_d(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, hipStream_t s, ProdWs &W);   // pbc_hip_d.hip: d, g
int launch_f(pbc_hip_pairing_s *P, void *d_gt, const void *d_g1, const void *d_g2, size_t n, int k, hipStream_t s, ProdWs &W);   // pbc_hip_f.hip
// one-time derivations on the device (single-lane kernels; results land in the object)
int derive_d(pbc_hip_pairing_s *P, hipStream_t s);
int derive_e(pbc_hip_pairing_s *P, hipStream_t s);
int derive_f(pbc_hip_pairing_s *P, hipStream_t s);
// preprocessed pairings: table derivation (one lane) and application (one second argument per lane)
struct pbc_hip_pp_s {
  pbc_hip_pairing_s *P;
  uint32_t *tab;      // device: type a [exp2 + 1][3][16] words; types d / g [steps][3][ND] words
  uint32_t *valid;    // device flag: first argument was a finite curve point
};
void pp_init_launch_a(pbc_hip_pairing_s *P, pbc_hip_pp_s *pp, const uint8_t *d_g1, bool a1);
int pp_init_launch_d(pbc_hip_pairing_s *P, pbc_hip_pp_s *pp, const uint8_t *d_g1);
int pp_apply_launch_a(pbc_hip_pp_s *pp, void *d_gt, const void *d_g2, size_t n, hipStream_t s);
int pp_apply_launch_d(pbc_hip_pp_s *pp, void *d_gt, const void *d_g2, size_t n, hipStream_t s);
// Table sets (pbc_hip_ppset.hip; include/pbc_hip.h pbc_hip_pp_set_t): m tables of pairing_pp_init in ONE allocation,
// table after table (table t: tabs + t tab_words, the layout pp_init_launch_* write), then one flag word per table and a
// copy of the m G1 records.
struct pbc_hip_pp_set_s {
  pbc_hip_pairing_s *P;
  int device;
  size_t m, tab_words;
  void *mem;          // the allocation
  uint32_t *tabs;     // device: [m][tab_words]
  uint32_t *flags;    // device: [m], first argument t was a finite curve point
  uint8_t *g1;        // device: [m] G1 records
};
// one lane per first argument: every table and flag of the set, one launch on s
int pp_set_init_launch_a(pbc_hip_pairing_s *P, pbc_hip_pp_set_s *set, bool a1, hipStream_t s);
int pp_set_init_launch_d(pbc_hip_pairing_s *P, pbc_hip_pp_set_s *set, hipStream_t s);
// The wave slots of a device-resident plan on the lane kernels: slot -> (table, units), lane -> record rec = (first +
// lane) stride + table tmul of d_g2, GT record rec of d_out (PpSlot above)
int pp_set_apply_launch_a(pbc_hip_pp_set_s *set, void *d_out, const void *d_g2, const uint64_t *d_plan, size_t slots, size_t stride, size_t tmul, hipStream_t s);
int pp_set_apply_launch_d(pbc_hip_pp_set_s *set, void *d_out, const void *d_g2, const uint64_t *d_plan, size_t slots, size_t stride, size_t tmul, hipStream_t s);
// The record route of a product over a set (512-bit type a): the plan's slots (term-major, pp_set_prod_plan) leave the
// Miller record of term u m + j in recs, then al_prod_finish_kernel multiplies the m records of each of the n products
int pp_set_records_a(pbc_hip_pp_set_s *set, void *d_gt, const void *d_g2, const uint64_t *d_plan, size_t slots, size_t n, void *recs, hipStream_t s);
// The folds of the GT route of a ragged call (pbc_hip_ragged.hip) on records that are already in place: cur / fcur hold
// sizes[0] GT records and their flag bytes, nxt / fnxt have room for sizes[1]; d_plan: the level arrays on the device
int ragged_gt_reduce(pbc_hip_pairing_s *P, void *d_gt, void *cur, void *fcur, void *nxt, void *fnxt, const uint64_t *const *d_plan,
                     const size_t *sizes, int nlevels, size_t n, unsigned F, hipStream_t s);
// A host-buffer call that runs on the object's OWN device only (a table set lives there): n units of ui bytes in and uo
// bytes out, staged in chunks of `chunk` units through the chunk buffers, streams and workspaces of that device's
// context; `launch` enqueues the units c0 .. c0 + cnt of a chunk (device pointers to the chunk's first records)
typedef std::function<int(void *d_out, const void *d_in, size_t c0, size_t cnt, hipStream_t s, const OwnWs *own)> RangeLaunch;
int run_host_own_device(pbc_hip_pairing_s *P, uint8_t *out, size_t uo, const uint8_t *in, size_t ui, size_t n, size_t chunk, const RangeLaunch &launch);
// type f diagnostics (pbc_hip_diag_stage)
int diag_f_miller(pbc_hip_pairing_s *P, void *dt, const void *d1, const void *d2, size_t n);
int diag_f_op(pbc_hip_pairing_s *P, int stage, void *dt, const void *d1, const void *d2, size_t n);
