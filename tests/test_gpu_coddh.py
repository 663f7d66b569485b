"""GPU tests (-m gpu) of is_almost_coddh over a batch (include/pbc_hip.h pbc_hip_is_almost_coddh_batch / _dev): verdicts
known by construction on every curve family, with the five classes mixed inside every wavefront; agreement with the
composition a caller had to write before (two element_pairing, element_mul_GT, comparisons on the host); the _dev form on
a stream of its own with guard bytes behind the result; the x-only BLS verification of example/bls.c:97-110 on d159."""
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT, golden, _param, param_value

pytestmark = pytest.mark.gpu

# family -> (parameter file, its random single-pairing fixture, the key of the group order in the parameter text)
FAMILIES = {"a": ("a", "a_rand32.vec", "r"), "a1": ("a1", "a1_rand6.vec", "n"), "d159": ("d159", "d_rand32.vec", "r"),
            "e": ("e", "e_rand6.vec", "r"), "f": ("f", "f_rand16.vec", "r"), "g149": ("g149", "g149_rand16.vec", "r")}
ALMOST_OF = {"A": 1, "B": 1, "C": 1, "D": 0, "E": 0}
EXACT_OF = {"A": 1, "B": 1, "C": 0, "D": 0, "E": 0}
CLASSES = "ABCDE"


def _be(x, n):
    return np.frombuffer(int(x).to_bytes(n, "big"), np.uint8)


def _route_limit(name):
    """the batch size up to which single pairings take the wave kernels (pbc_amd/csrc/host_params.h)"""
    src = open(os.path.join(ROOT, "pbc_amd", "csrc", "host_params.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


@pytest.fixture(scope="module")
def material(hips):
    """family -> the fixture's units with their multiples, built ONCE with element_mul_zn (pinned to the reference by the
    group tests): P, Q, T and [x]P, [x]Q, [r - x]Q, [x + 1]Q for random odd 64-bit x, one per unit"""
    class Lazy(dict):
        def __missing__(self, family):
            pname, vec, rkey = FAMILIES[family]
            v = golden(vec)
            H = hips[pname]
            r = param_value(pname, rkey)
            lz = H.length_in_bytes_Zr
            rng = np.random.default_rng(2024)
            xs = [int.from_bytes(rng.bytes(8), "big") | 1 for _ in range(v.n)]
            z = lambda f: np.stack([_be(f(x), lz) for x in xs])
            one = np.zeros(v.lenT, np.uint8)
            one[H.length_in_bytes_Fq - 1] = 1                       # GT's 1: the first coordinate is 1, the rest 0
            assert not (v.gt == one).all(axis=1).any()              # T_i != 1: class D is sound
            self[family] = dict(H=H, v=v, one=one, xP=H.element_mul_zn(1, v.g1, z(lambda x: x)),
                                xQ=H.element_mul_zn(2, v.g2, z(lambda x: x)), nxQ=H.element_mul_zn(2, v.g2, z(lambda x: r - x)),
                                x1Q=H.element_mul_zn(2, v.g2, z(lambda x: x + 1)))
            return self[family]
    return Lazy()


def _batch(m, n):
    """n lanes: lane j holds class j mod 5 on unit j mod (units of the fixture) -- every wavefront holds mixed verdicts.
    Returns a, b, c, d and the expected ALMOST / EXACT verdicts."""
    v = m["v"]
    j = np.arange(n)
    i, cls = j % v.n, j % 5
    nx = (i + 1) % v.n
    a = v.g1[i].copy()
    b = np.where((cls == 0)[:, None], v.g1[i], m["xP"][i])
    b[cls == 4] = v.g1[nx][cls == 4]
    c = v.g2[i].copy()
    c[cls == 4] = v.g2[nx][cls == 4]
    d = v.g2[i].copy()
    for k, src in ((1, m["xQ"]), (2, m["nxQ"]), (3, m["x1Q"])):
        d[cls == k] = src[i][cls == k]
    neighbours = (v.gt[i] == v.gt[nx]).all(axis=1).astype(np.uint8)       # class E: what the reference's bytes say (0)
    assert not neighbours.any()
    almost = np.array([ALMOST_OF[CLASSES[k]] for k in cls], np.uint8)
    exact = np.array([EXACT_OF[CLASSES[k]] for k in cls], np.uint8)
    almost[cls == 4] = neighbours[cls == 4]
    exact[cls == 4] = neighbours[cls == 4]
    return tuple(np.ascontiguousarray(x) for x in (a, b, c, d)) + (almost, exact)


SIZES = [(f, n) for f in sorted(FAMILIES) for n in (1, 65, 257)] + [("a", 2600), ("d159", 2600)]


@pytest.mark.parametrize("family,n", SIZES)
def test_verdicts_by_construction(material, family, n):
    """A (P, P, Q, Q) 1/1, B (P, [x]P, Q, [x]Q) 1/1, C (P, [x]P, Q, [r-x]Q) 1/0, D (P, [x]P, Q, [x+1]Q) 0/0,
    E (P_i, P_i+1, Q_i+1, Q_i) 0/0 (ALMOST/EXACT).  n = 1: a single call; 65: one lane past a wavefront; 257: one past a
    256-lane block; 2600: the 2 n = 5200 pairings are past the wave routes of a.param and d159 (5120 each) while n
    alone is not -- the lane kernels run."""
    if n == 2600:
        for lim in ("PBC_A_WAVE_MAX", "PBC_D_WAVE_MAX"):
            assert n <= _route_limit(lim) < 2 * n
    m = material[family]
    a, b, c, d, almost, exact = _batch(m, n)
    got = m["H"].is_almost_coddh(a, b, c, d)
    assert got.dtype == np.uint8 and got.shape == (n,) and np.isin(got, (0, 1)).all()
    assert np.array_equal(got, almost)
    got = m["H"].is_almost_coddh(a, b, c, d, exact=True)
    assert got.dtype == np.uint8 and got.shape == (n,) and np.isin(got, (0, 1)).all()
    assert np.array_equal(got, exact)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_agrees_with_the_composition(material, family):
    """the same inputs, with the identity record in one lane each of a and of b: the verdicts are those computed on the
    host from element_pairing(a, d), element_pairing(b, c) and element_mul_GT of the two"""
    m = material[family]
    H = m["H"]
    n = 257
    a, b, c, d, almost, exact = _batch(m, n)
    a[7] = 0
    b[130] = 0
    T0, T1 = H.element_pairing(a, d), H.element_pairing(b, c)
    same = (T0 == T1).all(axis=1)
    inverse = (H.element_mul_GT(T0, T1) == m["one"]).all(axis=1)
    keep = np.ones(n, bool)
    keep[[7, 130]] = False
    assert np.array_equal(same[keep].astype(np.uint8), exact[keep])           # (the composition itself meets the table)
    assert np.array_equal((same | inverse).astype(np.uint8), H.is_almost_coddh(a, b, c, d))
    assert np.array_equal(same.astype(np.uint8), H.is_almost_coddh(a, b, c, d, exact=True))


@pytest.mark.parametrize("family", ["a", "d159", "f"])
def test_dev_form_on_a_stream_of_its_own(material, family):
    """64 guard bytes behind the n-th result byte stay as they were; the result is the host-buffer form's; two calls back
    to back on one stream with different n (the workspace is reused, first larger then smaller then larger) are both right"""
    import torch
    m = material[family]
    H = m["H"]
    st = torch.cuda.Stream()
    runs = []
    for n, exact in ((257, False), (65, True), (300, False)):
        a, b, c, d, almost, ex = _batch(m, n)
        dev = [torch.from_numpy(x).cuda() for x in (a, b, c, d)]
        res = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        runs.append((n, exact, dev, res, ex if exact else almost, H.is_almost_coddh(a, b, c, d, exact=exact)))
    torch.cuda.synchronize()
    for n, exact, dev, res, want, host in runs:                              # enqueued back to back, no synchronisation between
        H.is_almost_coddh_dev(res.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), n,
                              exact=exact, stream=st.cuda_stream)
    st.synchronize()
    for n, exact, dev, res, want, host in runs:
        got = res.cpu().numpy()
        assert (got[n:] == 0xA5).all()
        assert np.array_equal(got[:n], host) and np.array_equal(got[:n], want)


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


def test_x_only_bls_on_d159(hips):
    """example/bls.c:97-110 as a batch on d159 (q = 1 mod 4: the y that element_from_bytes_x_only rebuilds is the
    signature's up to its sign): signatures and hashes of the reference's own run of the flow (d159_bls32.bin); each
    signature travels as its x alone.  e(sig', g) against e(h, pk): ALMOST accepts every one, EXACT exactly those whose
    rebuilt point is the original; a forged lane (signature j replaced by signature j + 1) is the only 0."""
    H = hips["d159"]
    b = _load_bls("d159_bls32.bin")
    n = len(b["sig"])
    g, pk = np.tile(b["g"], (n, 1)), np.tile(b["pk"], (n, 1))
    assert H.is_almost_coddh(b["sig"], b["h"], pk, g, exact=True).all()      # the plain verification, example/bls.c:70-78
    back = H.element_from_bytes_x_only(1, H.element_to_bytes_x_only(1, b["sig"]))
    kept = (back == b["sig"]).all(axis=1)
    assert np.array_equal(H.is_almost_coddh(back, b["h"], pk, g), np.ones(n, np.uint8))
    assert np.array_equal(H.is_almost_coddh(back, b["h"], pk, g, exact=True), kept.astype(np.uint8))
    j = 11
    forged = back.copy()
    forged[j] = back[j + 1]
    want = np.ones(n, np.uint8)
    want[j] = 0
    assert np.array_equal(H.is_almost_coddh(forged, b["h"], pk, g), want)
