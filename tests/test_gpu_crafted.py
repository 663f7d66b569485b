"""GPU half (-m gpu) of the crafted-operand battery: the field, Z_r and curve kernels through the C-ABI against exact Python
integers (tests/intref.py, pinned to the reference's fixtures by tests/test_crafted_cpu.py, which also runs every batch
below through the kernel source compiled for the host).  Every comparison is byte equality of a whole batch; batch
lengths are of the form 64 k + 1.

  F_q     every limb pattern of ref_harness.c soak_pattern as a value and as a Montgomery residue, 2^j and q - 2^j on every
          limb boundary, each against a 12-element subset, itself and its negative: all seven ops (op 3 not on 0); the
          records v + t q through ops 0 and 3.  One parameter set per arithmetic width.
  Z_r     the same on the modulus r (a1: n, operands sharing a factor with n left out), every op of zr_op
  G1/G2   element_add / sub / neg / double: points of the whole curve whose x follows the patterns (on the twists in
          every coefficient, or in the first alone), with a fixture point, themselves, their negatives and O
  mul_zn  the default route (fast signed-window ladder + complete pass): every scalar of intref.scalars on a fixture point,
          16 scalars below r on every crafted whole-curve point, the two interleaved
  pow2/3  structured scalars on every base; A2 = A1, A2 = -A1 with equal scalars, a base O
  GT      element_pow_zn on pairing values with the structured scalars against the C oracle

Sizing -- CPU seconds of the integer reference per test (process time, each battery computed once per session and shared with
its CPU twin; the GPU calls of a test take well under a second):
  F_q          0.0 - 0.1; the 1000-bit fields a1 0.3, e 0.2, a_160_1024 0.3
  Z_r          0.0; a1 0.4
  group law    G1 0.0 - 0.2; G2 a 0.2, d159 0.5, f 0.3, g149 1.1, d201 0.8, a1_200 0.0; e 2.6 / 2.4 (square roots mod a 1020-bit q)
  pow2 / pow3  G1 / G2: a 0.3 / 0.3, d159 0.1 / 0.7, f 0.1 / 0.3, g149 0.1 / 0.9
  mul_zn       G1 / G2: a 0.9 / 1.2, d159 0.4 / 3.0, f 0.3 / 1.6, g149 0.2 / 3.6, d201 0.3 / 3.3, f_256 0.6 / 3.3,
               a_160_256 0.3 / 0.3, e 2.7 / 0.0, a1 21.7 / 0.0
What was cut for size, and nothing else: d201's G2 keeps every third 2^j row of the scalar list; the 1000-bit sets e and a1 run
the list without its 2^j rows.  On e and a1 G2 is G1 (one curve, the same fixture points), so group 2 sends group 1's batch
through its own entry point and costs no second reference.  Every crafted whole-curve point meets all 16 scalars on every
set.  a1 stays above ten seconds (21.7) with no 2^j row or padding left to drop: 176 crafted points times ten 1022-bit
scalars over a 1033-bit field.

Scalars >= r: the reference library reads a Z_r record mod r; this library multiplies by the integer as it stands
(include/pbc_hip.h: "scalars may exceed r"; pinned on points of small order by tests/test_hostsim.py).  The two agree on
the order-r subgroup.  Off it -- the fixture points of G2 on types d, f, g, whose twists carry no cofactor in the reference --
the rows with a scalar >= r are judged by the header's reading (intref.Curve.mul reduce=False); the reference's reading
(reduce=True) is what the fixture pinning of tests/test_crafted_cpu.py exercises."""
import numpy as np
import pytest

import intref
pytestmark = pytest.mark.gpu

FQ_SETS = ["a", "d159", "d278027-190-181", "d201", "f_256", "a_160_256", "a_160_500", "a_224_768", "a1", "e", "a_160_1024", "g149"]
ZR_SETS = ["a", "a1", "d159", "f", "g149", "e", "a_150_300_mm"]
LAW_SETS = ["a", "d159", "f", "g149", "d201", "e", "a1_200"]
MUL_SETS = ["a", "d159", "f", "g149", "d201", "f_256", "a_160_256", "e", "a1"]
MULTI_SETS = ["a", "d159", "f", "g149"]
GT_SETS = ["a", "d159", "f", "g149", "e"]
KEY = intref.HIP_KEY
POW2_EVERY = intref.POW2_EVERY


def _bad(got, want):
    return np.nonzero((got != want).any(axis=1))[0]


@pytest.mark.parametrize("name", FQ_SETS)
def test_fq_on_crafted_operands(hips, name):
    A, B, cases, NA, nc_cases = intref.battery_fq(name)
    assert len(A) % 64 == 1
    H = hips[KEY.get(name, name)]
    assert intref.rbits_of(H.length_in_bytes_Fq) == intref.rbits_of(intref.fam(name).fb)
    for op, rows, want in cases:
        got = H.fq_op(op, A, B)
        bad = _bad(got[rows], want)
        assert len(bad) == 0, (op, [(A[rows[i]].tobytes().hex(), B[rows[i]].tobytes().hex()) for i in bad[:3]])
    for op, rows, want in nc_cases:
        got = H.fq_op(op, NA, NA)
        bad = _bad(got[rows], want)
        assert len(bad) == 0, ("non-canonical", op, [NA[rows[i]].tobytes().hex() for i in bad[:3]])


@pytest.mark.parametrize("name", ZR_SETS)
def test_zr_on_crafted_operands(hips, name):
    A, B, cases, dropped, total = intref.battery_zr(name)
    assert len(A) % 64 == 1 and dropped < 0.05 * total
    H = hips[KEY.get(name, name)]
    what = {v: k for k, v in intref.ZR_OPS.items()}
    for op, rows, want in cases:
        got = H.zr_op(what[op], A, B if op in (0, 1, 2, 7) else None)
        bad = _bad(got[rows], want)
        assert len(bad) == 0, (what[op], [(A[rows[i]].tobytes().hex(), B[rows[i]].tobytes().hex()) for i in bad[:3]])


@pytest.mark.parametrize("name,group", [(n, g) for n in LAW_SETS for g in intref.GROUPS])
def test_group_law_on_crafted_points(hips, name, group):
    A, B, want = intref.battery_law(name, group)
    assert len(A) % 64 == 1
    H = hips[KEY.get(name, name)]
    for what in ("add", "sub", "neg", "double"):
        got = H.element_group_op(what, group, A, B if what in ("add", "sub") else None)
        bad = _bad(got, want[what])
        assert len(bad) == 0, (what, [(A[i].tobytes().hex(), B[i].tobytes().hex()) for i in bad[:2]])


@pytest.mark.parametrize("name,group", [(n, g) for n in MUL_SETS for g in intref.GROUPS])
def test_scalar_multiplication_on_structured_scalars(hips, name, group):
    P, Z, want = intref.battery_mul(name, group, POW2_EVERY.get((name, group), 1))
    assert len(P) % 64 == 1
    got = hips[KEY.get(name, name)].element_mul_zn(group, P, Z)
    bad = _bad(got, want)
    assert len(bad) == 0, [(P[i].tobytes().hex(), Z[i].tobytes().hex()) for i in bad[:3]]


@pytest.mark.parametrize("name,group", [(n, g) for n in MULTI_SETS for g in intref.GROUPS])
def test_multi_exponentiation_on_structured_scalars(hips, name, group):
    bases, zs, p2, p3 = intref.battery_multi(name, group)
    assert len(p2) % 64 == 1
    H = hips[KEY.get(name, name)]
    bad = _bad(H.element_pow_multi(group, bases[:2], zs[:2]), p2)
    assert len(bad) == 0, ("pow2", [[x[i].tobytes().hex() for x in bases[:2] + zs[:2]] for i in bad[:2]])
    bad = _bad(H.element_pow_multi(group, bases, zs), p3)
    assert len(bad) == 0, ("pow3", [[x[i].tobytes().hex() for x in bases + zs] for i in bad[:2]])


@pytest.mark.parametrize("name", GT_SETS)
def test_gt_powers_on_structured_scalars(hips, oracles, name):
    G, Z = intref.battery_gt(name)
    assert len(G) % 64 == 1
    key = KEY.get(name, name)
    bad = _bad(hips[key].element_pow_zn_GT(G, Z), oracles[key].gt_pow(G, Z))
    assert len(bad) == 0, [Z[i].tobytes().hex() for i in bad[:4]]
