"""CPU tests of element_cmp (include/pbc_hip.h: pbc_hip_element_cmp_batch): the lane bodies of the kernels
(group_gtdiv.cuh) compiled for the host next to the host mirror (tests/hostsim/hostsim_gtdiv.cpp) on the pairs of
tests/cmp_battery.py, whose expected bytes are exact-integer results; the integer behind the coset compare
(pbc_amd/csrc/cmp_plan.h) against the trace recurrence in Python integers for every shipped type d / f / g file, through
pbc_hip_diag_quotient_cmp and through a stand-alone program built with the address and undefined-behaviour sanitizers;
the order of the errors; the Python wrappers as far as the C entry points."""
import ctypes
import glob
import math
import os
import subprocess

import numpy as np
import pytest

import cmp_battery as cb
import intref
import pbc_amd
from conftest import ROOT, _param, golden

PARAM_DIR = os.path.join(ROOT, "pbc_amd", "param")
ALL_PARAMS = sorted(os.path.basename(p)[:-6] for p in glob.glob(os.path.join(PARAM_DIR, "*.param")))
TWIST_PARAMS = [n for n in ALL_PARAMS if intref.param_dict(_param(n)).get("type") in ("d", "g", "f")]
PLAIN_SETS = ["a", "a1", "d159", "e", "f", "g149", "a_160_256"]


def _mismatches(got, want, labels):
    return [(i, labels[i], int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]


PLAIN_CASES = [(n, g) for n in PLAIN_SETS for g in (0, 1, 2, 3) if not (g == 2 and n in cb.TWISTS)]      # (the twists: below)


@pytest.mark.parametrize("name,group", PLAIN_CASES)
def test_plain_compare_on_host(name, group):
    """Z_r, G1, GT, and G2 of the symmetric types: equality of the reduced values; O == O; O != a finite point; an
    off-curve record reads as O; on a.param the zero record equals (q, q)"""
    a, b, want, labels = cb.battery(name, group)
    assert set(want) == {cb.EQUAL, cb.DIFFER}
    a0, b0 = a.copy(), b.copy()
    got, flags = cb.mirror(name).cmp(group, 0, a, b)
    assert not _mismatches(got, want, labels) and not flags.any()
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    if group in (1, 2):
        for lab in ("P / P, coordinates >= q", "O / O", "O / off curve", "off curve / off curve", "zero record / zero as q"):
            assert want[labels.index(lab)] == cb.EQUAL, lab
        for lab in ("P / -P", "P / O", "O / P", "P / Q", "P / off curve"):
            assert want[labels.index(lab)] == cb.DIFFER, lab


@pytest.mark.parametrize("name", cb.TWISTS)
def test_coset_compare_on_host(name):
    """G2 of types d, g, f.  Expected: [quotient_cmp](a - b) is O with the REFERENCE's integer; the mirror walks the
    shorter gcd(quotient_cmp, #twist).  The library's route, the complete lane alone and -- wherever it did not raise its
    flag -- the fast lane alone give that byte.  The fast lane raises its flag for a difference of order 2, 3 or 4 (the
    doubling of a point with y = 0, the table's 3P = O, two doublings in a row: exceptional whatever the digits are) and
    for no pair whose difference is O or lies outside the small torsion.  (A difference of order 6 can pass the incomplete
    steps untouched -- odd digits are only added to even multiples -- so its verdict is asserted, its flag is not.)"""
    a, b, want, labels = cb.point_battery(name, 2)
    assert want[labels.index("P / P + [r]X")] == cb.EQUAL and want[labels.index("O / [r]X")] == cb.EQUAL
    assert want[labels.index("P / P + X")] == cb.DIFFER and want[labels.index("P / -P")] == cb.DIFFER
    if "P / P + [N/r]X" in labels:
        assert want[labels.index("P / P + [N/r]X")] == cb.DIFFER
    M = cb.mirror(name)
    got, flags = M.cmp(2, 0, a, b)
    assert not _mismatches(got, want, labels)
    slow, none = M.cmp(2, 1, a, b)
    assert not _mismatches(slow, want, labels) and not none.any()
    fast, flags2 = M.cmp(2, 2, a, b)
    assert np.array_equal(flags, flags2) and set(flags) <= {0, 1}
    keep = flags == 0
    assert not _mismatches(fast[keep], want[keep], [l for l, k in zip(labels, keep) if k])
    for i, lab in enumerate(labels):
        torsion = lab.startswith(("difference of order ", "order "))
        if torsion and lab.replace("difference of ", "").split()[1] in ("2", "3", "4"):
            assert flags[i] == 1, lab
        elif not torsion:
            assert flags[i] == 0, lab
    f = cb.flagged_pair(name)
    if name in ("d159", "d201"):
        assert f is not None                                     # (their twists have even order)
    if f is not None:
        assert flags[f] == 1


def test_twist_batteries_hold_small_torsion():
    """at least one shipped twist has the differences the fast lane must flag"""
    assert any(cb.flagged_pair(name) is not None for name in cb.TWISTS)


# ---- the integer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_PARAMS)
def test_diag_quotient_cmp_matches_the_trace_recurrence(name):
    """which = 0: quotient_cmp from the recurrence in Python integers; which = 1: gcd(quotient_cmp, twist order); nothing
    for groups 1 and 3 and for the symmetric types.  No device is needed."""
    H = pbc_amd.Pairing(_param(name))
    ref = cb.quotient_cmp_of_text(_param(name))
    assert (ref is not None) == (name in TWIST_PARAMS)
    for group in (0, 1, 3, 4):
        assert H.quotient_cmp(group, 0) is None and H.quotient_cmp(group, 1) is None
    assert H.quotient_cmp(2, 2) is None and H.quotient_cmp(2, -1) is None
    if ref is None:
        assert H.quotient_cmp(2, 0) is None and H.quotient_cmp(2, 1) is None
    else:
        c, N = ref
        r = intref.fam(name).r
        assert H.quotient_cmp(2, 0) == c
        assert H.quotient_cmp(2, 1) == math.gcd(c, N)
        assert c % r and (c.bit_length() + 7) // 8 <= pbc_amd.MPZ_MAX_BYTES
        if intref.fam(name).type == "f":
            assert math.gcd(c, N) == 2 * intref.fam(name).q - r
        else:
            assert math.gcd(c, N) == c
    H.clear()


def test_eleven_twist_files_are_shipped():
    assert len(TWIST_PARAMS) == 11, TWIST_PARAMS


def test_cmp_plan_under_the_sanitizers(tmp_path):
    """tests/hostsim/cmp_plan_check.cpp: its own main around cmp_plan.h, built with -fsanitize=address,undefined, run on
    every shipped parameter text; a plain executable, nothing is loaded into this interpreter"""
    exe = str(tmp_path / "cmp_plan_check")
    build = subprocess.run([cb.CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(cb.HOSTSIM, "cmp_plan_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and any(w in build.stderr.lower() for w in ("asan", "ubsan", "sanitizer", "clang_rt")):
        pytest.skip("this toolchain cannot link the sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    files = [os.path.join(PARAM_DIR, n + ".param") for n in ALL_PARAMS]
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    rows = [line.split() for line in run.stdout.splitlines()]
    assert [r[0] for r in rows] == files
    for name, (_, h0, h1) in zip(ALL_PARAMS, rows):
        ref = cb.quotient_cmp_of_text(_param(name))
        if ref is None:
            assert (h0, h1) == ("-", "-"), name
        else:
            assert int(h0, 16) == ref[0] and int(h1, 16) == math.gcd(*ref), name


# ---- the C-ABI and the Python wrappers -----------------------------------------------------------------------------------
def test_errors_come_in_the_stated_order_without_a_device():
    """null arguments with n > 0, then the group, both before a device is looked for; n == 0 returns 0 and touches nothing"""
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    L = pbc_amd.lib()
    res = np.zeros(v.n, np.uint8)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    for group in (1, 7):                                         # a null argument is reported whatever the group is
        for args in ((None, ptr(v.g1), ptr(v.g1)), (ptr(res), None, ptr(v.g1)), (ptr(res), ptr(v.g1), None)):
            assert L.pbc_hip_element_cmp_batch(H._h, group, *args, v.n) != 0
            assert b"null argument" in L.pbc_hip_last_error()
            assert L.pbc_hip_element_cmp_batch_dev(H._h, group, *args, v.n, None) != 0
            assert b"null argument" in L.pbc_hip_last_error()
    for group in (4, -1):
        assert L.pbc_hip_element_cmp_batch(H._h, group, ptr(res), ptr(v.g1), ptr(v.g1), v.n) != 0
        assert b"group" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_cmp_batch_dev(H._h, group, 0x1000, 0x1000, 0x1000, v.n, None) != 0
        assert b"group" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_cmp_batch(H._h, group, None, None, None, 0) != 0      # (the group is checked for n == 0 too)
    assert L.pbc_hip_element_cmp_batch(None, 1, ptr(res), ptr(v.g1), ptr(v.g1), v.n) != 0
    assert b"null pairing" in L.pbc_hip_last_error()
    for group in (0, 1, 2, 3):
        assert L.pbc_hip_element_cmp_batch(H._h, group, None, None, None, 0) == 0
        assert L.pbc_hip_element_cmp_batch_dev(H._h, group, None, None, None, 0, None) == 0
    assert not res.any()
    with pytest.raises(pbc_amd.PbcHipError, match="group"):
        H.element_cmp(4, v.g1, v.g1)
    with pytest.raises(ValueError):
        H.element_cmp(2, v.g1, v.g1)                             # G1 records where G2 records belong (40 / 120 bytes)
    with pytest.raises(ValueError):
        H.element_cmp(1, v.g1, v.g1[:-1])
    H.clear()


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    zr = np.zeros((4, H.length_in_bytes_Zr), np.uint8)
    for group, recs in ((0, zr), (1, v.g1), (2, v.g2), (3, v.gt)):
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_cmp(group, recs, recs)
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_cmp_dev(group, 0x1000, 0x1000, 0x1000, 4, stream=0)
    H.clear()
