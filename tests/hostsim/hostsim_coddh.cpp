// hostsim_coddh.cpp -- TEST INFRASTRUCTURE: the host mirror (hostsim.cpp: the device headers compiled for the CPU, one
// lane per call) plus the lane body of coddh_verdict_kernel (group_more.cuh coddh_verdict_lane), with the type dispatch
// of the kernel in pbc_hip_group.hip.  Built by tests/test_coddh_cpu.py into a library of its own.  Not part of the product.
#include "hostsim.cpp"

extern "C" {

// res[i] = verdict on the GT records t0[i], t1[i] (lenT bytes each); almost != 0: PBC_HIP_CODDH_ALMOST
int hostsim_coddh(void *h, uint8_t *res, const uint8_t *t0, const uint8_t *t1, size_t n, int almost) {
  pbc_hip_pairing_s *P = (pbc_hip_pairing_s *) h;
  activate(P);
  const size_t L = (size_t) P->lenT;
  const bool al = almost != 0;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *x = t0 + i * L, *y = t1 + i * L;
    uint8_t v = 0xff;
    if (P->type == 'a' || P->type == '1') { if (P->nlimb == 16) v = coddh_verdict_lane<GtA<16>>(x, y, al); else v = coddh_verdict_lane<GtA<33>>(x, y, al); }
    else if (P->type == 'e') { if (P->nlimb == 16) v = coddh_verdict_lane<GtE<16>>(x, y, al); else v = coddh_verdict_lane<GtE<33>>(x, y, al); }
    else if (P->type == 'f') { HS_DISPATCH_F(P->nlimb, v = coddh_verdict_lane<GtF<N>>(x, y, al)); }
    else { HS_DISPATCH_D(P, (v = coddh_verdict_lane<GtD<N, DEG>>(x, y, al))); }
    res[i] = v;
  }
  return 0;
}

}
