"""CPU tests of GT inversion / division (include/pbc_hip.h: pbc_hip_element_invert_GT_batch, pbc_hip_element_div_GT_batch):
the lane bodies of the kernels (group_gtdiv.cuh) compiled for the host next to the host mirror
(tests/hostsim/hostsim_gtdiv.cpp) on the GT battery of tests/member_battery.py, judged in the exact-integer towers of
member_battery.gt_field; the inverse the reference's side supplies; the C entry points and Python wrappers without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import cmp_battery as cb
import intref
import member_battery as mb
import pbc_amd
from conftest import ROOT, _param, golden, param_value

FAMILIES = ["a", "a1", "d159", "e", "f", "g149"]
RKEY = {"a1": "n"}


def _canonical(name, recs):
    S = intref.fam(name)
    return all(int.from_bytes(row[i:i + S.fb].tobytes(), "big") < S.q for row in recs for i in range(0, recs.shape[1], S.fb))


@pytest.mark.parametrize("generic", [False, True], ids=["default", "group_slow"])
@pytest.mark.parametrize("name", FAMILIES)
def test_invert_lane_on_host(name, generic):
    """x * out == 1 in the integer tower for every unit but 0, 0 gives the zero record, every coordinate is canonical; the
    lane that ran is the unitary one for pairing values, 1 and their other byte images, the generic one for 2 x a pairing
    value and random elements (cmp_battery.expect_generic: type e has no conjugation, everything but 1 is inverted)"""
    recs, _, labels = mb.gt_battery(name)
    K, decode, _ = mb.gt_field(name)
    out, lanes = cb.mirror(name).gtdiv(recs, generic=generic)
    assert _canonical(name, out)
    for i, lab in enumerate(labels):
        x, y = decode(recs[i].tobytes()), decode(out[i].tobytes())
        if lab == "0":
            assert not out[i].any()
        else:
            assert K.mul(x, y) == K.one, lab
        assert lanes[i] == (1 if generic else int(cb.expect_generic(name, lab))), (lab, int(lanes[i]))
    assert {"pairing value", "1", "0", "2 x pairing value", "random element", "coordinates >= q", "1 as 1 + q"} <= set(labels)


@pytest.mark.parametrize("name", FAMILIES)
def test_default_and_generic_lanes_agree_on_host(name):
    recs = mb.gt_battery(name)[0]
    ia, ib = cb.div_pairs(name)
    M = cb.mirror(name)
    assert np.array_equal(M.gtdiv(recs)[0], M.gtdiv(recs, generic=True)[0])
    assert np.array_equal(M.gtdiv(recs[ia], recs[ib])[0], M.gtdiv(recs[ia], recs[ib], generic=True)[0])


@pytest.mark.parametrize("name", FAMILIES)
def test_div_lane_on_host(name):
    """out * b == a over pairs of the battery; a division by 0 gives the zero record; the lane follows the DIVISOR"""
    recs, _, labels = mb.gt_battery(name)
    K, decode, _ = mb.gt_field(name)
    ia, ib = cb.div_pairs(name)
    out, lanes = cb.mirror(name).gtdiv(recs[ia], recs[ib])
    assert _canonical(name, out)
    for k, (i, j) in enumerate(zip(ia, ib)):
        a, b, o = (decode(x.tobytes()) for x in (recs[i], recs[j], out[k]))
        if labels[j] == "0":
            assert not out[k].any()
        else:
            assert K.mul(o, b) == a, (labels[i], labels[j])
        assert lanes[k] == int(cb.expect_generic(name, labels[j])), (labels[i], labels[j])


@pytest.mark.parametrize("name", FAMILIES)
def test_inverse_of_a_pairing_value_is_the_reference_sides(oracles, name):
    """T^(r-1) from the oracle, obtained as tests/test_coddh_cpu.py obtains it, is the mirror's inverse byte for byte"""
    T = golden(intref.FIXTURE_OF[name]).gt
    r = param_value(name, RKEY.get(name, "r"))
    elen = (r.bit_length() + 7) // 8
    e_inv = np.tile(np.frombuffer((r - 1).to_bytes(elen, "big"), np.uint8), (len(T), 1))
    Tinv = oracles[name].gt_pow(T, e_inv)
    out, lanes = cb.mirror(name).gtdiv(T)
    assert np.array_equal(out, Tinv)
    if name != "e":
        assert not lanes.any()


# ---- the C-ABI and the Python wrappers -----------------------------------------------------------------------------------
SYMS = ("pbc_hip_element_invert_GT_batch", "pbc_hip_element_invert_GT_batch_dev", "pbc_hip_element_div_GT_batch",
        "pbc_hip_element_div_GT_batch_dev", "pbc_hip_element_cmp_batch", "pbc_hip_element_cmp_batch_dev", "pbc_hip_diag_quotient_cmp")


def test_exports_and_header_agree():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(pbc_amd.LIB_PATH)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, code) and sym in pbc_amd.EXPORTS and hasattr(L, sym), sym


def test_header_cites_the_reference():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    block = hdr[hdr.index("Inversion and division on GT"):hdr.index("pbc_hip_diag_quotient_cmp(pbc_hip_pairing_t")]
    for ref in ("include/pbc_field.h:394", ":324",
                "ecc/pairing.c:203-209", "arith/montfp.c:400", "include/pbc_field.h:424", "ecc/curve.c:29-33", "ecc/curve.c:375-391",
                "ecc/d_param.c:1060-1069", "ecc/g_param.c:1336", "ecc/f_param.c:388-398", "example/bls.c:104-105",
                "if (!element_cmp(a, b))", "pbc_hip_is_almost_coddh_batch", "zero record"):
        assert ref in block, ref


def test_null_arguments_are_rejected_without_a_device():
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    L = pbc_amd.lib()
    out = np.zeros_like(v.gt)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    for args in ((None, ptr(v.gt)), (ptr(out), None)):
        assert L.pbc_hip_element_invert_GT_batch(H._h, args[0], args[1], v.n) != 0
        assert b"null argument" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_invert_GT_batch_dev(H._h, args[0], args[1], v.n, None) != 0
        assert b"null argument" in L.pbc_hip_last_error()
    for args in ((None, ptr(v.gt), ptr(v.gt)), (ptr(out), None, ptr(v.gt)), (ptr(out), ptr(v.gt), None)):
        assert L.pbc_hip_element_div_GT_batch(H._h, *args, v.n) != 0
        assert b"null argument" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_div_GT_batch_dev(H._h, *args, v.n, None) != 0
        assert b"null argument" in L.pbc_hip_last_error()
    assert L.pbc_hip_element_invert_GT_batch(None, ptr(out), ptr(v.gt), v.n) != 0
    assert b"null pairing" in L.pbc_hip_last_error()
    assert L.pbc_hip_element_invert_GT_batch(H._h, None, None, 0) == 0         # n == 0: nothing is looked at
    assert L.pbc_hip_element_div_GT_batch_dev(H._h, None, None, None, 0, None) == 0
    assert not out.any()
    with pytest.raises(ValueError):
        H.element_invert_GT(v.g1)                                  # 40-byte records where 120-byte records belong
    with pytest.raises(ValueError):
        H.element_div_GT(v.gt, v.gt[:-1])
    H.clear()


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    """as tests/test_ppset_cpu.py: every form gets as far as the library and comes back with its 'no HIP device' error"""
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    calls = [lambda: H.element_invert_GT(v.gt), lambda: H.element_div_GT(v.gt, v.gt),
             lambda: H.element_invert_GT_dev(0x1000, 0x1000, 4, stream=0), lambda: H.element_div_GT_dev(0x1000, 0x1000, 0x1000, 4, stream=0)]
    for f in calls:
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            f()
    H.clear()
