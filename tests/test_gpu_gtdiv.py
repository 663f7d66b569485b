"""GPU tests of pbc_hip_element_invert_GT_batch / div_GT / element_cmp and their _dev forms (include/pbc_hip.h): the
batteries of tests/member_battery.py and tests/cmp_battery.py (expected values: exact integers) through the library on
its default route and with "hip_group_slow 1" (every lane through the subfield inversion / the complete ladder) -- the
two must give identical bytes -- whole and in slices that cross a wavefront and a workgroup with the special unit first,
last and alone; the _dev forms on a stream of their own, in place on either operand."""
import numpy as np
import pytest

import cmp_battery as cb
import intref
import member_battery as mb
import pbc_amd
from conftest import _param

pytestmark = pytest.mark.gpu

SETS = ["a", "a1", "d159", "e", "f", "g149", "d201", "a_160_256"]
WIDE = ("a1", "e")                                               # 33-word fields: one slice length
LENGTHS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def pairings():
    """(name, slow) -> the library's object"""
    class Lazy(dict):
        def __missing__(self, key):
            name, slow = key
            self[key] = pbc_amd.Pairing(_param(name) + ("hip_group_slow 1\n" if slow else ""))
            return self[key]
    objs = Lazy()
    yield objs
    for H in objs.values():
        H.clear()


def _slices(name, plain, special):
    """[(label, row indices)]: the lengths with `special` first, last and alone among the `plain` rows"""
    out = []
    for n in ((65,) if name in WIDE else LENGTHS):
        if n == 1:
            out.append(("alone", [special]))
            continue
        fill = [plain[i % len(plain)] for i in range(n)]
        out.append(("%d first" % n, [special] + fill[1:]))
        out.append(("%d last" % n, fill[:-1] + [special]))
    return out


@pytest.mark.parametrize("name", SETS)
def test_invert_and_div(pairings, name):
    """the whole battery: x * out == 1 and out * b == a in the integer tower, canonical coordinates, 0 -> the zero record;
    the default route and "hip_group_slow 1" agree byte for byte; then the slices, with an element of norm != 1 (the lane
    that runs the inversion) first, last and alone among pairing values, against the rows of the whole-battery result"""
    H, S = pairings[(name, False)], pairings[(name, True)]
    recs, _, labels = mb.gt_battery(name)
    K, decode, _ = mb.gt_field(name)
    F = intref.fam(name)
    inv = H.element_invert_GT(recs)
    assert inv.dtype == np.uint8 and inv.shape == recs.shape
    assert np.array_equal(inv, S.element_invert_GT(recs))
    for i, lab in enumerate(labels):
        if lab == "0":
            assert not inv[i].any()
        else:
            assert K.mul(decode(recs[i].tobytes()), decode(inv[i].tobytes())) == K.one, lab
    assert all(int.from_bytes(row[i:i + F.fb].tobytes(), "big") < F.q for row in inv for i in range(0, inv.shape[1], F.fb))
    ia, ib = cb.div_pairs(name)
    quo = H.element_div_GT(recs[ia], recs[ib])
    assert np.array_equal(quo, S.element_div_GT(recs[ia], recs[ib]))
    for k, (i, j) in enumerate(zip(ia, ib)):
        if labels[j] == "0":
            assert not quo[k].any()
        else:
            assert K.mul(decode(quo[k].tobytes()), decode(recs[j].tobytes())) == decode(recs[i].tobytes()), (labels[i], labels[j])
    plain = [i for i, lab in enumerate(labels) if lab == "pairing value"]
    special = labels.index("random element")
    assert cb.expect_generic(name, "random element")
    one = labels.index("1")
    for lab, rows in _slices(name, plain, special):
        for P in (H, S):
            assert np.array_equal(P.element_invert_GT(recs[rows]), inv[rows]), lab
        ones = [one] * len(rows)                                 # 1 / x = x^-1: the division against the inversion
        assert np.array_equal(H.element_div_GT(recs[ones], recs[rows]), inv[rows]), lab


@pytest.mark.parametrize("group", [0, 1, 2, 3])
@pytest.mark.parametrize("name", SETS)
def test_cmp(pairings, name, group):
    """the battery of (parameter set, group) on both routes; on the twists the slices place a pair whose difference has
    order 3, 4 or 2 -- flagged by the fast lane (asserted on the host mirror) -- first, last and alone among pairs of one
    coset; elsewhere a differing pair among equal ones"""
    H, S = pairings[(name, False)], pairings[(name, True)]
    a, b, want, labels = cb.battery(name, group)
    a0, b0 = a.copy(), b.copy()
    got = H.element_cmp(group, a, b)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = [(i, labels[i], int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad
    assert np.array_equal(S.element_cmp(group, a, b), want)
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    twist = group == 2 and name in cb.TWISTS
    special = cb.flagged_pair(name) if twist else None
    if special is None:
        special = int(np.flatnonzero(want == cb.DIFFER)[0])
    plain = [i for i in range(len(want)) if want[i] == cb.EQUAL and (not twist or labels[i] in ("P / P + [r]X", "P + [r]X / P", "[r]X / [r]Q"))]
    for lab, rows in _slices(name, plain, special):
        for P in (H, S):
            assert np.array_equal(P.element_cmp(group, a[rows], b[rows]), want[rows]), lab


@pytest.mark.parametrize("name", ["a", "d159", "f"])
def test_dev_forms_on_a_stream_of_their_own(pairings, name):
    """invert with out == a, div with out == a and with out == b (exactly), cmp with guard bytes behind the verdicts: the
    host forms' bytes, inputs of cmp unchanged"""
    import torch
    H = pairings[(name, False)]
    recs, _, labels = mb.gt_battery(name)
    n = 257
    ra = np.ascontiguousarray(recs[[i % len(recs) for i in range(n)]])
    rb = np.ascontiguousarray(recs[[(3 * i + 1) % len(recs) for i in range(n)]])
    inv, quo = H.element_invert_GT(ra), H.element_div_GT(ra, rb)
    s = torch.cuda.Stream()
    d = [torch.from_numpy(x.copy()).cuda() for x in (ra, ra, rb, ra, rb)]
    a2, b2, want, _ = cb.battery(name, 2)
    rows = [i % len(want) for i in range(n)]
    ca, cbb = torch.from_numpy(np.ascontiguousarray(a2[rows])).cuda(), torch.from_numpy(np.ascontiguousarray(b2[rows])).cuda()
    res = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    H.element_invert_GT_dev(d[0].data_ptr(), d[0].data_ptr(), n, s.cuda_stream)
    H.element_div_GT_dev(d[1].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, s.cuda_stream)       # out == a
    H.element_div_GT_dev(d[4].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), n, s.cuda_stream)       # out == b
    H.element_cmp_dev(2, res.data_ptr(), ca.data_ptr(), cbb.data_ptr(), n, s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d[0].cpu().numpy(), inv)
    assert np.array_equal(d[1].cpu().numpy(), quo) and np.array_equal(d[2].cpu().numpy(), rb)
    assert np.array_equal(d[4].cpu().numpy(), quo) and np.array_equal(d[3].cpu().numpy(), ra)
    out = res.cpu().numpy()
    assert np.array_equal(out[:n], want[rows]) and (out[n:] == 0xEE).all()
    assert np.array_equal(ca.cpu().numpy(), a2[rows]) and np.array_equal(cbb.cpu().numpy(), b2[rows])


def test_empty_batch_succeeds_and_touches_nothing(pairings):
    import ctypes
    H = pairings[("d159", False)]
    res = np.full(8, 0xEE, np.uint8)
    L = pbc_amd.lib()
    p = ctypes.c_void_p(res.ctypes.data)
    assert L.pbc_hip_element_invert_GT_batch(H._h, p, None, 0) == 0
    assert L.pbc_hip_element_div_GT_batch(H._h, p, None, None, 0) == 0
    for group in (0, 1, 2, 3):
        assert L.pbc_hip_element_cmp_batch(H._h, group, p, None, None, 0) == 0
        assert H.element_cmp(group, np.zeros((0, 1), np.uint8), np.zeros((0, 1), np.uint8)).shape == (0,)
    assert (res == 0xEE).all()
