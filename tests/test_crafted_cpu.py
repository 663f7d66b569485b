"""CPU half of the crafted-operand battery (tests/intref.py: exact Python integers; tests/test_gpu_crafted.py: the GPU half).

First the integer reference is pinned to the reference library: it must reproduce, byte for byte, the fixtures the
reference wrote (group law *_gops{1,2}.rec, Z_r *_zrops.rec, scalar multiplications *_g1mulfull6 / *_g2mul6 / *_g2mulfull6.vec,
the G1 / G2 arrays of *_pow23g{1,2}.rec), and every G2 record of those files must satisfy the twist equation derived
from the parameter text -- a wrong twist constant or coefficient order fails here.

Then every batch of the GPU battery runs through the kernel source compiled for the host (tests/hostsim): fq_op, zr_op,
affine_op, group (element_mul_zn on G1, element_pow_zn on GT), g2_mul, multi.  Exact byte equality of whole batches.
What the host build does not expose: the launch side -- the two-pass orchestration on the device (flag words, the
compaction of the reported lanes; the host mirror calls the complete routine for a reported lane directly), the staging
of host buffers, and the limb-image entry points; element_mul_zn on G2 of the symmetric types goes through `group`."""
import math
import os

import numpy as np
import pytest

import hostsim
import intref
import oracle
from conftest import GOLDEN, PARAM_OF, _param, golden


@pytest.fixture(scope="module")
def sims():
    class Lazy(dict):
        def __missing__(self, t):
            self[t] = hostsim.HostSim(_param(PARAM_OF.get(t, t)))
            return self[t]
    return Lazy()


def rec(name):
    return oracle.Rec(os.path.join(GOLDEN, name)).arrays


GOPS = [("a", 1), ("a1", 1), ("e", 1), ("d159", 1), ("d159", 2), ("f", 1), ("f", 2), ("g149", 2), ("d201", 2), ("f_256", 2)]
ZROPS = ["a", "a1", "d159", "d224", "f", "f_256", "g149"]
MULS = [("a", 1, "a_g1mulfull6.vec"), ("a", 2, "a_g2mulfull6.vec"), ("d159", 1, "d159_g1mulfull6.vec"), ("g149", 1, "g149_g1mulfull6.vec"),
        ("e", 1, "e_g1mulfull6.vec"), ("d159", 2, "d159_g2mul6.vec"), ("d201", 2, "d201_g2mul6.vec"), ("g149", 2, "g149_g2mul6.vec"),
        ("f", 2, "f_g2mul6.vec")]
POW23 = [("a", 1), ("e", 1), ("d159", 1), ("d159", 2), ("f", 1), ("f", 2)]
ZR_FILE = {1: 2, 2: 3, 0: 4, 3: 5, 4: 6, 6: 7, 5: 8, 7: 9}       # op code -> array of the fixture that holds its result


def _side(name, group):
    S = intref.fam(name)
    return (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)


def _on_curve(lay, recs):
    """every record is O (zero bytes) or satisfies the curve equation with coordinates below q"""
    for r in recs:
        if r.any():
            raw = r.tobytes()
            P = (lay.elem(raw[:lay.length // 2]), lay.elem(raw[lay.length // 2:]))
            assert lay.encode(P) == raw and lay.C.on_curve(P)


# ---- the reference is pinned to PBC before it judges anything -------------------------------------------------------------
def test_op_numbering_is_the_library_s():
    import pbc_amd
    assert intref.ZR_OPS == pbc_amd.ZR_OPS
    assert {k: v for k, v in intref.ZR_OPS.items() if v < 7} == intref.FQ_OPS


@pytest.mark.parametrize("name,group", GOPS)
def test_integer_group_law_reproduces_the_fixtures(name, group):
    A, B, ADD, SUB, NEG, DBL = rec("%s_gops%d.rec" % (name, group))
    C, lay = _side(name, group)
    for arr in (A, B, ADD, SUB, NEG, DBL):
        _on_curve(lay, arr)
    a, b = lay.unpack(A), lay.unpack(B)
    assert np.array_equal(lay.pack([C.add(x, y) for x, y in zip(a, b)]), ADD)
    assert np.array_equal(lay.pack([C.sub(x, y) for x, y in zip(a, b)]), SUB)
    assert np.array_equal(lay.pack([C.neg(x) for x in a]), NEG)
    assert np.array_equal(lay.pack([C.dbl(x) for x in a]), DBL)


@pytest.mark.parametrize("name", ZROPS)
def test_integer_zr_reproduces_the_fixtures(name):
    R = rec(name + "_zrops.rec")
    S = intref.fam(name)
    a = [int.from_bytes(x.tobytes(), "big") for x in R[0]]
    b = [int.from_bytes(x.tobytes(), "big") for x in R[1]]
    for op, idx in ZR_FILE.items():
        want = [int.from_bytes(x.tobytes(), "big") for x in R[idx]]
        assert [S.zr.op(op, x, y) for x, y in zip(a, b)] == want, op


@pytest.mark.parametrize("name,group,file", MULS)
def test_integer_scalar_multiplication_reproduces_the_fixtures(name, group, file):
    v = golden(file)
    C, lay = _side(name, group)
    if group == 2:
        _on_curve(lay, v.g1)
        _on_curve(lay, v.gt)
    ks = [int.from_bytes(z.tobytes(), "big") for z in v.g2]
    pts = lay.unpack(v.g1, zero_is_O=False)
    assert np.array_equal(lay.pack([C.mul(k, P) for k, P in zip(ks, pts)]), v.gt)
    assert np.array_equal(lay.pack([C.mul_many([k], P)[0] for k, P in zip(ks, pts)]), v.gt)


@pytest.mark.parametrize("name,group", POW23)
def test_integer_multi_exponentiation_reproduces_the_fixtures(name, group):
    A1, A2, A3, N1, N2, N3, P2, P3 = rec("%s_pow23g%d.rec" % (name, group))
    C, lay = _side(name, group)
    if group == 2:
        for arr in (A1, A2, A3, P2, P3):
            _on_curve(lay, arr)
    a = [lay.unpack(x) for x in (A1, A2, A3)]
    n = [[int.from_bytes(z.tobytes(), "big") for z in x] for x in (N1, N2, N3)]
    m = [[C.mul(k, P) for k, P in zip(n[j], a[j])] for j in range(3)]
    p2 = [C.add(x, y) for x, y in zip(m[0], m[1])]
    assert np.array_equal(lay.pack(p2), P2)
    assert np.array_equal(lay.pack([C.add(x, y) for x, y in zip(p2, m[2])]), P3)


def test_extension_field_inverse_and_square_root():
    for name in ("d159", "f", "g149", "f_256"):
        F = intref.fam(name).g2.F
        rng = np.random.default_rng(5)
        for _ in range(4):
            x = F.from_coeffs([int.from_bytes(rng.bytes(40), "big") for _ in range(F.d)])
            assert F.mul(x, F.inv(x)) == F.one
            y = F.from_coeffs([int.from_bytes(rng.bytes(40), "big") for _ in range(F.d)])
            assert F.mul(x, y) == F.mul_schoolbook(x, y) and F.mul(x, x) == F.mul_schoolbook(x, x)
            assert F.mul(x, F.one) == x and F.mul(F.neg(F.one), y) == F.neg(y)
            s = F.mul(x, x)
            y = intref.sqrt(F, s)
            assert y in (x, F.neg(x))


# ---- the crafted operands themselves ------------------------------------------------------------------------------------------
def test_patterns_restate_the_soak_generator():
    """spot values of soak_pattern for a.param's q (18 limbs of 29 bits) and a1.param's p (38 limbs of 28 bits)"""
    q = intref.fam("a").q
    assert intref.rbits_of(64) == 522 and intref.rbits_of(20) == 174 and intref.rbits_of(130) == 28 * 38
    assert intref.soak_pattern(0, q, 522) == q - 1 and intref.soak_pattern(5, q, 522) == (q + 1) // 2
    assert intref.soak_pattern(8, q, 522) == (1 << (q.bit_length() - 1)) - 1            # cut below q
    assert intref.soak_pattern(10, q, 522) == ((1 << 29) - 1) << (29 * 9)
    assert intref.soak_pattern(13, q, 522) == sum(((1 << 29) - 1) << (29 * i) for i in range(1, 18, 2)) & ((1 << 511) - 1)
    assert intref.soak_pattern(15, q, 522) == 1 << (29 * 9)
    assert intref.soak_pattern(19, q, 522) == (1 << 256) - 1
    p = intref.fam("a1").q
    assert intref.soak_pattern(14, p, 28 * 38) == 1 << 28 and intref.soak_pattern(16, p, 28 * 38) == 1 << (28 * 36)
    rows = intref.patterns(q, 522)
    labels = [r[0] for r in rows]
    assert len(set(labels)) == len(labels) and {"p0", "p8/R", "2^58", "m-2^493", "2^493/R"} <= set(labels)
    R = 1 << 522
    for lab, t, mont, v in rows:
        x = intref.operand(v, mont, q, 522)
        assert 0 <= x < q and (x * R % q if mont else x) == v
    assert intref.noncanonical(5, q, 64) % q == 5 and intref.noncanonical(5, q, 64) + q >= 1 << 512 > intref.noncanonical(5, q, 64)


def test_deep_divstep_operands_are_as_deep_as_recorded():
    """the named inversion operands: well above a uniform operand's count, and present in the F_q battery"""
    for name, (count, g) in intref.DEEP_DIVSTEPS.items():
        S = intref.fam(name)
        assert 0 < g < S.q and intref.divsteps(S.q, g) == count and count > 2.04 * S.q.bit_length()
        a = intref.operand(g, True, S.q, intref.rbits_of(S.fb))
        assert a * (1 << intref.rbits_of(S.fb)) % S.q == g
    A = intref.battery_fq("d159")[0]
    a = intref.operand(intref.DEEP_DIVSTEPS["d159"][1], True, intref.fam("d159").q, intref.rbits_of(20))
    assert any(int.from_bytes(x.tobytes(), "big") == a for x in A)


def test_scalars_hold_the_structured_rows():
    S = intref.fam("a")
    rows = intref.scalars(S.r, S.zl)
    ks = [k for _, k in rows]
    assert ks[:12] == [0, 1, 2, 3, S.r - 1, S.r - 2, S.r, 2 ** 160 - 1, 2 ** 160 - 2, 15, 16, 17]
    assert len(set(ks)) == len(ks) and all(0 <= k < 2 ** 160 for k in ks)
    for nib in range(1, 16):
        v = int("%x" % nib * 40, 16)
        assert v in ks and v % S.r in ks and (v ^ 1) in ks
    for k in (int("0f" * 20, 16), int("f0" * 20, 16), 2 ** 159 - 1, 2 ** 159, 2 ** 159 + 1, S.r + 1, S.r + 2, (S.r - 1) // 2, (S.r + 1) // 2,
              2 ** 157, 2 ** 157 - 1, 2 ** 156 + 1, 2 ** 4 + 1, 2 ** 5 - 1):
        assert k in ks and (k ^ 1) in ks, hex(k)
    # the reduced list keeps every nibble pattern
    red = [k for _, k in intref.scalars(S.r, S.zl, pow2_rows=False)]
    assert all(int("%x" % nib * 40, 16) in red for nib in range(1, 16)) and 2 ** 100 not in red
    assert len(intref.whole_curve_scalars("a")) == 16


def test_a1_operands_that_share_a_factor_with_n_are_few():
    for name in ("a1",):
        A, B, cases, dropped, total = intref.battery_zr(name)
        assert dropped < 0.05 * total, (dropped, total)
        n = intref.fam(name).r
        assert all(math.gcd(int.from_bytes(x.tobytes(), "big"), n) == 1 for x in A)


# ---- the battery of tests/test_gpu_crafted.py on the kernel source compiled for the host ---------------------------------------
FQ_SETS = ["a", "d159", "d278027-190-181", "d201", "f_256", "a_160_256", "a_160_500", "a_224_768", "a1", "e", "a_160_1024", "g149"]
ZR_SETS = ["a", "a1", "d159", "f", "g149", "e", "a_150_300_mm"]
LAW_SETS = ["a", "d159", "f", "g149", "d201", "e", "a1_200"]
MUL_SETS = ["a", "d159", "f", "g149", "d201", "f_256", "a_160_256", "e", "a1"]
MULTI_SETS = ["a", "d159", "f", "g149"]
GT_SETS = ["a", "d159", "f", "g149", "e"]
TWISTED = ("d159", "f", "g149", "d201", "f_256")
KEY = intref.HIP_KEY


def _host_group(name, group):
    return group if name in TWISTED else 1            # (symmetric types: G2 is G1, the host mirror has one set of routines)


@pytest.mark.parametrize("name", FQ_SETS)
def test_fq_on_crafted_operands_on_host(sims, name):
    A, B, cases, NA, nc_cases = intref.battery_fq(name)
    assert len(A) % 64 == 1
    S = sims[KEY.get(name, name)]
    for op, rows, want in cases:
        got = S.fq_op(op, A, B)
        assert np.array_equal(got[rows], want), (op, np.nonzero((got[rows] != want).any(axis=1))[0][:8])
    for op, rows, want in nc_cases:
        assert np.array_equal(S.fq_op(op, NA, NA)[rows], want), ("non-canonical", op)


@pytest.mark.parametrize("name", ZR_SETS)
def test_zr_on_crafted_operands_on_host(sims, name):
    A, B, cases, dropped, total = intref.battery_zr(name)
    assert len(A) % 64 == 1
    S = sims[KEY.get(name, name)]
    for op, rows, want in cases:
        got = S.zr_op(op, A, B if op in (0, 1, 2, 7) else None)
        assert np.array_equal(got[rows], want), (op, np.nonzero((got[rows] != want).any(axis=1))[0][:8])


@pytest.mark.parametrize("name,group", [(n, g) for n in LAW_SETS for g in intref.GROUPS])
def test_group_law_on_crafted_points_on_host(sims, name, group):
    A, B, want = intref.battery_law(name, group)
    assert len(A) % 64 == 1
    S = sims[KEY.get(name, name)]
    hg = _host_group(name, group)
    for op, what in enumerate(("add", "sub", "neg", "double")):
        got = S.affine_op(op, hg, A, B if op < 2 else None)
        assert np.array_equal(got, want[what]), (what, np.nonzero((got != want[what]).any(axis=1))[0][:8])


@pytest.mark.parametrize("name,group", [(n, g) for n in MUL_SETS for g in intref.GROUPS])
def test_scalar_multiplication_on_structured_scalars_on_host(sims, name, group):
    P, Z, want = intref.battery_mul(name, group, intref.POW2_EVERY.get((name, group), 1))
    assert len(P) % 64 == 1
    S = sims[KEY.get(name, name)]
    S.fallbacks()
    got = S.g2_mul(P, Z) if _host_group(name, group) == 2 else S.group(0, P, Z)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (bad[:8], [Z[i].tobytes().hex() for i in bad[:4]])
    assert 0 < S.fallbacks() < len(P)                 # both passes ran: the fast ladder and the complete routine


@pytest.mark.parametrize("name,group", [(n, g) for n in MULTI_SETS for g in intref.GROUPS])
def test_multi_exponentiation_on_structured_scalars_on_host(sims, name, group):
    bases, zs, p2, p3 = intref.battery_multi(name, group)
    assert len(p2) % 64 == 1
    S = sims[KEY.get(name, name)]
    hg = _host_group(name, group)
    got = S.multi(hg, bases[:2], zs[:2])
    assert np.array_equal(got, p2), np.nonzero((got != p2).any(axis=1))[0][:8]
    got = S.multi(hg, bases, zs)
    assert np.array_equal(got, p3), np.nonzero((got != p3).any(axis=1))[0][:8]


@pytest.mark.parametrize("name", GT_SETS)
def test_gt_powers_on_structured_scalars_on_host(sims, oracles, name):
    G, Z = intref.battery_gt(name)
    key = KEY.get(name, name)
    assert np.array_equal(sims[key].group(2, G, Z), oracles[key].gt_pow(G, Z))
