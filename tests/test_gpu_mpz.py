"""GPU tests of pbc_hip_element_mul_mpz_batch / _dev (include/pbc_hip.h): the batteries of tests/mpz_battery.py (expected
records: exact integers, tests/intref.py) through the host-buffer and the _dev form; slices that cross a wavefront and a
workgroup with a unit the fast lane flags (tests/test_mpz_cpu.py shows it on the host mirror) first, last and alone; the
compiled reference's scalar multiplications (tests/golden/*mul*.vec) unit by unit; byte equality with element_mul_zn /
element_pow_zn_GT on a replicated scalar; stream order of the digits; in place; "hip_group_slow 1"."""
import glob
import os

import numpy as np
import pytest

import intref
import member_battery as mb
import mpz_battery as zb
import pbc_amd
from conftest import GOLDEN, _param, golden, key_of, PARAM_OF

pytestmark = pytest.mark.gpu

SETS = ["a", "a1", "d159", "e", "f", "g149"]
LENGTHS = (1, 63, 64, 65, 193)


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


def _units(name, group):
    """-> records, labels, {scalar label: (rows, expected)} of one (set, group); G2 of the symmetric types is G1's curve"""
    if group == 3:
        recs, labels = zb.gt_units(name)
        return recs, labels, zb.gt_expected(name)
    recs, labels, _ = zb.point_units(name, group)
    return recs, labels, zb.point_expected(name, group)


def _scalars(name, group):
    return zb.scalars(name, group)


def _dev(H, group, recs, k, stream=None):
    """the _dev form: records in a device tensor with a guard behind the output"""
    import torch
    recs = np.ascontiguousarray(recs)
    d_in = torch.from_numpy(recs).cuda()
    d_out = torch.full((recs.size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    H.element_mul_mpz_dev(group, d_out.data_ptr(), d_in.data_ptr(), k, len(recs), stream.cuda_stream if stream else 0)
    (stream.synchronize() if stream else torch.cuda.synchronize())
    out = d_out.cpu().numpy()
    assert (out[recs.size:] == 0xEE).all() and np.array_equal(d_in.cpu().numpy(), recs)
    return out[:recs.size].reshape(recs.shape)


@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("name", SETS)
def test_batteries(pairings, name, group):
    """every unit x scalar of the batteries, host-buffer form and _dev form (on a stream of its own), against intref"""
    import torch
    H = pairings[(name, False)]
    recs, labels, want = _units(name, group)
    L = pbc_amd.lib()
    s = torch.cuda.Stream()
    for lab, k, kb in _scalars(name, group):
        rows, exp = want[lab]
        x = np.ascontiguousarray(recs[rows])
        got = np.full_like(x, 0xEE)
        rc = L.pbc_hip_element_mul_mpz_batch(H._h, group, got.ctypes.data, x.ctypes.data, kb, len(kb), len(x))   # the row's own bytes
        assert rc == 0, L.pbc_hip_last_error()
        bad = [labels[r] for i, r in enumerate(rows) if not np.array_equal(got[i], exp[i])]
        assert not bad, (lab, bad)
        assert np.array_equal(_dev(H, group, x, k, s), exp), lab


def _special(name, group):
    """-> (kind, record): points: member_battery.flagged_unit, a unit of small order, which the fast lane flags at the
    slices' k (tests/test_mpz_cpu.py asserts that on the host mirror), else -- curves of prime order -- an off-curve one;
    GT: a random element, which the Lucas lane of a.param and the cyclotomic lane of f.param report"""
    S = intref.fam(name)
    if group == 3:
        recs, labels = zb.gt_units(name)
        i = labels.index("random element")
        return ("flagged" if name in ("a", "f") else "odd one out"), recs[i]
    g = zb.curve_group(name, group)
    f = mb.flagged_unit(name, g)
    brecs, _, blabels = mb.point_battery(name, g)
    if f is not None:
        return "flagged", brecs[f]
    return "odd one out", brecs[blabels.index("off curve")]


@pytest.mark.parametrize("slow", [False, True], ids=["default", "group_slow"])
@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("name", SETS)
def test_slices(pairings, name, group, slow):
    """n = 1, 63, 64, 65, 193 with the special unit first, last and alone: the partial last wave, two workgroups, and the
    second pass over flagged lanes only; "hip_group_slow 1": one slice, every lane through the complete pass"""
    H = pairings[(name, slow)]
    S = intref.fam(name)
    recs, labels, want = _units(name, group)
    k = dict((lab, k) for lab, k, _ in _scalars(name, group))["random mid"]
    rows, exp = want["random mid"]
    plain = [i for i, lab in enumerate(labels) if lab in ("subgroup", "pairing value")]
    kind, srec = _special(name, group)
    if group == 3:
        sexp = zb.gt_pow(name, srec[None, :], k)[0]
    else:
        g = zb.curve_group(name, group)
        C, lay = (S.g1, S.lay1) if g == 1 else (S.g2, S.lay2)
        sexp = lay.pack([C.mul(k, lay.decode(srec.tobytes()), reduce=False)])[0]
    for n in ((65,) if slow else LENGTHS):
        fill = [plain[i % len(plain)] for i in range(n)]
        for where in (("alone",) if n == 1 else ("first",) if slow else ("first", "last")):
            x, e = recs[fill].copy(), exp[fill].copy()
            at = 0 if where in ("alone", "first") else n - 1
            x[at], e[at] = srec, sexp
            got = H.element_mul_mpz(group, x, k)
            assert np.array_equal(got, e), (n, where, kind, [i for i in range(n) if not np.array_equal(got[i], e[i])][:8])


ANCHORS = {"a_g1mulfull6.vec": ("a", 1), "a_g2mulfull6.vec": ("a", 2), "d159_g1mulfull6.vec": ("d159", 1), "d159_g2mul6.vec": ("d159", 2),
           "d201_g2mul6.vec": ("d201", 2), "d224_g1mul6.vec": ("d224", 1), "e_g1mul3.vec": ("e", 1), "e_g1mulfull6.vec": ("e", 1),
           "f_g2mul6.vec": ("f", 2), "g149_g1mulfull6.vec": ("g149", 1), "g149_g2mul6.vec": ("g149", 2)}


def test_anchor_list_is_every_mul_fixture():
    assert sorted(ANCHORS) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "*mul*.vec")))


@pytest.mark.parametrize("vec", sorted(ANCHORS))
def test_reference_anchor(pairings, vec):
    """the compiled reference's own results: the first 8 units of every scalar-multiplication fixture, one call of n = 1
    per unit with that unit's scalar; the bytes are the fixture's"""
    name, group = ANCHORS[vec]
    H = pairings[(name, False)]
    v = golden(vec)
    for i in range(min(8, v.n)):
        k = int.from_bytes(v.g2[i].tobytes(), "big")
        got = H.element_mul_mpz(group, v.g1[i:i + 1], k)
        assert np.array_equal(got[0], v.gt[i]), (vec, i)


@pytest.mark.parametrize("name", SETS)
def test_equals_the_zr_record_route(pairings, name):
    """4096 units, a random k < r replicated: G1, G2 and GT on pairing values give element_mul_zn's / element_pow_zn_GT's bytes"""
    H = pairings[(name, False)]
    S = intref.fam(name)
    n = 4096
    rng = intref._rng(name, 77)
    k = 1 + intref._rand_below(rng, S.r - 1)
    Z = np.tile(np.frombuffer(k.to_bytes(S.zl, "big"), np.uint8), (n, 1))
    for group in (1, 2, 3):
        recs, labels, _ = _units(name, group)
        plain = [i for i, lab in enumerate(labels) if lab in ("subgroup", "neg subgroup", "pairing value")]
        x = np.ascontiguousarray(recs[[plain[i % len(plain)] for i in range(n)]])
        ref = H.element_pow_zn_GT(x, Z) if group == 3 else H.element_mul_zn(group, x, Z)
        assert np.array_equal(H.element_mul_mpz(group, x, k), ref), group


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("name", ["a", "d159", "f"])
def test_stream_order_and_in_place(pairings, name, group):
    """two _dev calls on ONE stream with different k and nothing between them, a third on a second stream: each result is
    its own k's (the digits travel in stream order; a later call does not overwrite an earlier one's); then out == in"""
    import torch
    H = pairings[(name, False)]
    recs, labels, want = _units(name, group)
    ks = dict((lab, k) for lab, k, _ in _scalars(name, group))
    labs = ("random mid", "random 8 zl + 1 bits", "r - 1")
    n = 193
    rows = [i % len(recs) for i in range(n)]
    x = torch.from_numpy(np.ascontiguousarray(recs[rows])).cuda()
    outs = [torch.full((n, recs.shape[1]), 0xEE, dtype=torch.uint8, device="cuda") for _ in labs]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    H.element_mul_mpz_dev(group, outs[0].data_ptr(), x.data_ptr(), ks[labs[0]], n, s1.cuda_stream)
    H.element_mul_mpz_dev(group, outs[1].data_ptr(), x.data_ptr(), ks[labs[1]], n, s1.cuda_stream)
    H.element_mul_mpz_dev(group, outs[2].data_ptr(), x.data_ptr(), ks[labs[2]], n, s2.cuda_stream)
    torch.cuda.synchronize()
    for lab, o in zip(labs, outs):
        assert want[lab][0] == list(range(len(recs)))
        assert np.array_equal(o.cpu().numpy(), want[lab][1][rows]), lab
    H.element_mul_mpz_dev(group, x.data_ptr(), x.data_ptr(), ks[labs[0]], n, s1.cuda_stream)      # in place
    s1.synchronize()
    assert np.array_equal(x.cpu().numpy(), want[labs[0]][1][rows])
    y = np.ascontiguousarray(recs[rows])
    L = pbc_amd.lib()
    kb = ks[labs[1]].to_bytes((ks[labs[1]].bit_length() + 7) // 8, "big")
    assert L.pbc_hip_element_mul_mpz_batch(H._h, group, y.ctypes.data, y.ctypes.data, kb, len(kb), n) == 0    # host form, in place
    assert np.array_equal(y, want[labs[1]][1][rows])


def test_empty_batch_succeeds_and_touches_nothing(pairings):
    import ctypes
    H = pairings[("d159", False)]
    out = np.full(8, 0xEE, np.uint8)
    L = pbc_amd.lib()
    for group in (1, 2, 3):
        assert L.pbc_hip_element_mul_mpz_batch(H._h, group, ctypes.c_void_p(out.ctypes.data), None, b"\x07", 1, 0) == 0
        assert L.pbc_hip_element_mul_mpz_batch_dev(H._h, group, None, None, None, 0, 0, None) == 0
        assert H.element_mul_mpz(group, np.zeros((0, 1), np.uint8), 7).shape[0] == 0
    assert (out == 0xEE).all()
