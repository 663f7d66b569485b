// hostsim_member.cpp -- TEST INFRASTRUCTURE: the host mirror (hostsim.cpp: the device headers compiled for the CPU, one
// lane per call) plus the lane bodies of the membership kernels (group_member.cuh), with the dispatch of
// pbc_hip_member.hip.  Built by tests/test_member_cpu.py into a library of its own.  Not part of the product.
#include "hostsim.cpp"
#include "../../pbc_amd/csrc/group_member.cuh"

// F = the field policy of group 1 / 2, RP = where the constant block keeps r (pbc_hip_member.hip PBC_DISPATCH_MEMBER)
#define HS_DISPATCH_MEMBER(P_, group_, ...)                                                                       \
  do {                                                                                                            \
    const int t_ = (P_)->type;                                                                                    \
    if (t_ == 'a' || t_ == '1') { typedef ROfA RP; if ((P_)->nlimb == 16) { typedef FqOps<16> F; __VA_ARGS__; } else { typedef FqOps<33> F; __VA_ARGS__; } } \
    else if (t_ == 'e') { typedef ROfE RP; if ((P_)->nlimb == 16) { typedef FqOps<16> F; __VA_ARGS__; } else { typedef FqOps<33> F; __VA_ARGS__; } } \
    else if (t_ == 'f') {                                                                                         \
      typedef ROfF RP;                                                                                            \
      if ((group_) == 2) { HS_DISPATCH_F((P_)->nlimb, { typedef Fq2Ops<N> F; __VA_ARGS__; }); }                    \
      else { HS_DISPATCH_F((P_)->nlimb, { typedef FqOps<N> F; __VA_ARGS__; }); }                                  \
    } else {                                                                                                      \
      typedef ROfD RP;                                                                                            \
      if ((group_) == 2) { HS_DISPATCH_D(P_, { typedef FdOps<N, DEG> F; __VA_ARGS__; }); }                        \
      else { HS_DISPATCH_D(P_, { typedef FqOps<N> F; (void) DEG; __VA_ARGS__; }); }                               \
    }                                                                                                             \
  } while (0)
#define HS_DISPATCH_MEMBER_GT(P_, ...)                                                                            \
  do {                                                                                                            \
    const int t_ = (P_)->type;                                                                                    \
    if (t_ == 'a' || t_ == '1') { typedef ROfA RP; if ((P_)->nlimb == 16) { typedef GtA<16> G; __VA_ARGS__; } else { typedef GtA<33> G; __VA_ARGS__; } } \
    else if (t_ == 'e') { typedef ROfE RP; if ((P_)->nlimb == 16) { typedef GtE<16> G; __VA_ARGS__; } else { typedef GtE<33> G; __VA_ARGS__; } } \
    else if (t_ == 'f') { typedef ROfF RP; HS_DISPATCH_F((P_)->nlimb, { typedef GtF<N> G; __VA_ARGS__; }); }      \
    else { typedef ROfD RP; HS_DISPATCH_D(P_, { typedef GtD<N, DEG> G; __VA_ARGS__; }); }                         \
  } while (0)

extern "C" {

// G1 / G2 (group 1 / 2).  mode 0: as the library -- the fast lane, and the complete lane where it raised its flag;
// 1: the complete lane alone ("hip_group_slow 1"); 2: the fast lane alone (verdicts as it left them).  flags[i]: the
// fast lane's flag (0 in mode 1).  The 512-bit type a field takes the limb-form fast lane, bound tracker armed.
int hostsim_member_points(void *h, int group, int mode, uint8_t *res, uint8_t *flags, const uint8_t *in, size_t n) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  if (group != 1 && group != 2) return 1;
  activate(P);
  const size_t L = (size_t) (group == 2 ? P->len2 : P->len1);
  const bool fast_a = P->type == 'a' && !P->a_generic;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *rec = in + i * L;
    bool flag = false;
    uint8_t v = 0xff;
    if (mode != 1) {
      if (fast_a) v = MemberAL<16>::fast_lane(rec, flag);
      else HS_DISPATCH_MEMBER(P, group, (v = ec_member_fast_lane<F, RP>(rec, flag)));
    }
    if (mode == 1 || (mode == 0 && flag)) HS_DISPATCH_MEMBER(P, group, (v = ec_member_complete_lane<F, RP>(rec)));
    flags[i] = flag ? 1 : 0;
    res[i] = v;
  }
  return 0;
}
// GT.  mode 0: as the library (the 512-bit type a field: the Lucas lane, the generic lane where it raised its flag; other
// fields: the generic lane); 1: the generic lane alone; 2: the Lucas lane alone (type a fast path only)
int hostsim_member_gt(void *h, int mode, uint8_t *res, uint8_t *flags, const uint8_t *in, size_t n) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  activate(P);
  const size_t L = (size_t) P->lenT;
  const bool fast_a = P->type == 'a' && !P->a_generic;
  if (mode == 2 && !fast_a) return 1;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *rec = in + i * L;
    bool flag = false;
    uint8_t v = 0xff;
    if (mode != 1 && fast_a) v = MemberAL<16>::gt_fast_lane(rec, P->len_zr, flag);
    if (mode == 1 || (mode == 0 && (flag || !fast_a))) HS_DISPATCH_MEMBER_GT(P, (v = gt_member_lane<G, RP>(rec)));
    flags[i] = flag ? 1 : 0;
    res[i] = v;
  }
  return 0;
}

}
