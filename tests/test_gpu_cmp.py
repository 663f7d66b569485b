"""GPU test of the verification lines of example/bls.c:100-105 as a batch (include/pbc_hip.h): two pairings,
element_cmp, element_invert on GT, element_cmp again -- against pbc_hip_is_almost_coddh_batch, unit for unit, on the
reference's own runs of the BLS flow (tests/golden/d159_bls32.bin, f_bls32.bin) with signatures rebuilt from their x alone
and one forged lane."""
import os
import struct

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _load_bls(name):
    raw = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
    assert raw[:8] == b"PBCBLS01"
    t, n, hlen, l1, l2, lz = struct.unpack("<6I", raw[8:32])
    arr = np.frombuffer(raw, np.uint8)
    off, out = 32, {}
    for nm, cnt, ln in (("digests", n, hlen), ("h", n, l1), ("sig", n, l1), ("g", 1, l2), ("pk", 1, l2), ("sk", 1, lz)):
        out[nm] = arr[off:off + cnt * ln].reshape(cnt, ln).copy()
        off += cnt * ln
    return out


@pytest.mark.parametrize("name,vec", [("d159", "d159_bls32.bin"), ("f", "f_bls32.bin")])
def test_bls_verification_lines_as_a_batch(hips, name, vec):
    """temp1 = e(sig, g), temp2 = e(h, pk); accept if !element_cmp(temp1, temp2), else element_invert(temp1) and accept if
    !element_cmp(temp1, temp2): the ALMOST verdicts of is_almost_coddh, which holds both outcomes (rebuilt signatures of
    either sign) and a rejection (the forged lane)"""
    H = hips[name]
    b = _load_bls(vec)
    n = len(b["sig"])
    g, pk = np.tile(b["g"], (n, 1)), np.tile(b["pk"], (n, 1))
    sig = H.element_from_bytes_x_only(1, H.element_to_bytes_x_only(1, b["sig"]))
    sig[11] = sig[12]
    sig[5] = H.element_group_op("neg", 1, b["sig"][5:6])[0]                  # (both signs occur whatever root the x-only format rebuilds)
    sig[6] = b["sig"][6]
    want = H.is_almost_coddh(sig, b["h"], pk, g)
    exact = H.is_almost_coddh(sig, b["h"], pk, g, exact=True)
    assert want[5] == 1 and exact[5] == 0 and exact[6] == 1 and want[11] == 0 and want.sum() == n - 1
    t1, t2 = H.element_pairing(sig, g), H.element_pairing(b["h"], pk)
    c1 = H.element_cmp(3, t1, t2)
    c2 = H.element_cmp(3, H.element_invert_GT(t1), t2)
    assert set(c1) | set(c2) <= {0, 1}
    assert np.array_equal(1 - c1, exact)
    assert np.array_equal(((c1 == 0) | (c2 == 0)).astype(np.uint8), want)
