"""CPU tests of the membership verdicts (include/pbc_hip.h: pbc_hip_element_membership_batch): the lane bodies of the
kernels (group_member.cuh) compiled for the host next to the host mirror (tests/hostsim/hostsim_member.cpp) -- the fast
lane with its flag, the complete lane, the GT lanes -- on the batteries of tests/member_battery.py, whose expected classes
are exact-integer results of tests/intref.py; the Python wrappers as far as the C entry points; the header's citations."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import intref
import member_battery as mb
import pbc_amd
from conftest import ROOT, _param, golden

HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SETS = ["a", "a1", "d159", "e", "f", "g149", "a_160_256"]


@pytest.fixture(scope="module")
def member_sim():
    """tests/hostsim/hostsim_member.cpp built as tests/hostsim/__init__.py builds hostsim.cpp"""
    lib = os.path.join(HOSTSIM, "libhostsim_member.so")
    csrc = os.path.join(ROOT, "pbc_amd", "csrc")
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim_member.cpp", "hostsim.cpp", "hostsim_shim.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if (not os.path.exists(lib)) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([CLANG, "-O1", "-Wno-psabi", "-std=c++17", "-fPIC", "-shared", "-I", HOSTSIM, "-o", lib,
                               os.path.join(HOSTSIM, "hostsim_member.cpp")])
    L = ctypes.CDLL(lib)
    L.hostsim_init.restype = ctypes.c_void_p
    L.hostsim_init.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.hostsim_member_points.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t]
    L.hostsim_member_gt.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t]
    handles = {}

    def run(name, group, mode, recs):
        """-> verdicts, flags of the fast lane.  group 3: GT"""
        if name not in handles:
            text = _param(name).encode()
            handles[name] = L.hostsim_init(text, len(text))
            assert handles[name]
        recs = np.ascontiguousarray(recs, np.uint8)
        res, flags = np.full(len(recs), 0xee, np.uint8), np.full(len(recs), 0xee, np.uint8)
        if group == 3:
            rc = L.hostsim_member_gt(handles[name], mode, res.ctypes.data, flags.ctypes.data, recs.ctypes.data, len(recs))
        else:
            rc = L.hostsim_member_points(handles[name], group, mode, res.ctypes.data, flags.ctypes.data, recs.ctypes.data, len(recs))
        assert rc == 0
        return res, flags
    return run


def _mismatches(got, want, labels):
    return [(i, labels[i], int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", SETS)
def test_point_lanes_on_host(member_sim, name, group):
    """the library's route (fast lane, complete lane where it raised its flag) and the complete lane alone give intref's
    class for every unit; the fast lane's own verdict is already right wherever it did not raise its flag; it raises the
    flag for a point of small order and for no point of the order-r subgroup"""
    recs, want, labels = mb.point_battery(name, group)
    whole = {mb.OUTSIDE} if mb.curve_order(name, group) != intref.fam(name).r else set()      # (f, g149 G1: E(F_q) has r points)
    assert set(want) >= {mb.INVALID, mb.INSIDE, mb.IDENTITY} | whole, sorted(set(want))
    got, flags = member_sim(name, group, 0, recs)
    assert not _mismatches(got, want, labels)
    slow, none = member_sim(name, group, 1, recs)
    assert not _mismatches(slow, want, labels) and not none.any()
    fast, flags2 = member_sim(name, group, 2, recs)
    assert np.array_equal(flags, flags2) and set(flags) <= {0, 1}
    keep = flags == 0
    assert not _mismatches(fast[keep], want[keep], [l for l, k in zip(labels, keep) if k])
    for i, lab in enumerate(labels):
        if lab in ("subgroup", "neg subgroup", "O", "off curve", "coordinates >= q"):
            assert not flags[i], lab
    small = [i for i, lab in enumerate(labels) if lab.startswith("order ") and want[i] == mb.OUTSIDE]
    if intref.fam(name).type in ("a", "a1", "e"):
        assert small                                             # #E = q + 1 (a, a1), q - 1 = h r^2 (e): even
    if small:
        assert flags[small].any(), [labels[i] for i in small]
    f = mb.flagged_unit(name, group)                             # the unit the GPU slices place first, last and alone
    assert (f is not None) == bool(small)
    if f is not None:
        assert flags[f] == 1 and want[f] == mb.OUTSIDE and got[f] == mb.OUTSIDE and slow[f] == mb.OUTSIDE, labels[f]
    for i, lab in enumerate(labels):                             # a doubling chain from a point with y = 0, or through one
        if lab in ("order 2", "order 4") and want[i] == mb.OUTSIDE:
            assert flags[i], lab
    assert (want[flags == 1] == mb.OUTSIDE).all()                # a flagged lane holds a finite point outside the subgroup


def test_two_torsion_shift_is_outside_on_host(member_sim):
    """[r] (P + T) = T for a 2-torsion T: a test of the x-coordinate alone would pass, the class is OUTSIDE.  Every family
    with an even curve order: types a, a1 (T = (0, 0)), type e (#E = h r^2, h even: its own digit source, r in binary, on
    the 33-word field), and the twist of d159"""
    for name, group in (("a", 1), ("a_160_256", 1), ("a1", 1), ("e", 1), ("d159", 2)):
        recs, want, labels = mb.point_battery(name, group)
        rows = [i for i, lab in enumerate(labels) if lab.startswith("subgroup + ")]
        assert rows and (want[rows] == mb.OUTSIDE).all(), name
        for mode in (0, 1, 2):
            got, flags = member_sim(name, group, mode, recs[rows])
            assert (got == mb.OUTSIDE).all() and not flags.any(), (name, mode)


@pytest.mark.parametrize("name", ["a", "a1", "d159", "e", "f", "g149", "a_160_256"])
def test_gt_lanes_on_host(member_sim, name):
    """GT: the library's route and the generic power alone; on the 512-bit type a field the Lucas lane decides the
    elements of norm 1 and raises its flag for exactly the others (0 and 1 are decided before the power)"""
    recs, want, labels = mb.gt_battery(name)
    assert set(want) == {mb.INVALID, mb.OUTSIDE, mb.INSIDE, mb.IDENTITY}
    assert all(w == mb.INSIDE for w, lab in zip(want, labels) if lab in ("pairing value", "coordinates >= q"))
    got, flags = member_sim(name, 3, 0, recs)
    assert not _mismatches(got, want, labels)
    slow, _ = member_sim(name, 3, 1, recs)
    assert not _mismatches(slow, want, labels)
    if name == "a":
        fast, flags2 = member_sim(name, 3, 2, recs)
        assert np.array_equal(flags, flags2)
        assert [lab for lab, f in zip(labels, flags) if f] == [lab for lab in labels if lab in ("2 x pairing value", "random element")]
        keep = flags == 0
        assert np.array_equal(fast[keep], want[keep])
    else:
        assert not flags.any()


# ---- the C-ABI and the Python wrappers -----------------------------------------------------------------------------------
def test_exports_and_header_agree():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(pbc_amd.LIB_PATH)
    for sym in ("pbc_hip_element_membership_batch", "pbc_hip_element_membership_batch_dev"):
        assert re.search(r"\b%s\s*\(" % sym, code) and sym in pbc_amd.EXPORTS and hasattr(L, sym), sym
    for k, v in (("INVALID", 0), ("OUTSIDE", 1), ("INSIDE", 2), ("IDENTITY", 3)):
        assert re.search(r"#define PBC_HIP_MEMBER_%s\s+%d\b" % (k, v), hdr) and getattr(pbc_amd, "MEMBER_" + k) == v
    assert (mb.INVALID, mb.OUTSIDE, mb.INSIDE, mb.IDENTITY) == (0, 1, 2, 3)


def test_header_cites_the_reference_for_membership():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    block = hdr[hdr.index("Membership verdicts"):hdr.index("pbc_hip_element_membership_batch_dev")]
    for ref in ("ecc/curve.c:57-77", "ecc/curve.c:609-623", "pairing->r", "element_mul_mpz", "element_pow_mpz", "element_is0",
                "element_is1", "include/pbc_pairing.h"):
        assert ref in block, ref
    classes = hdr[hdr.index("Input classes"):hdr.index("#ifndef PBC_HIP_H")]
    assert "pbc_hip_element_membership_batch" in classes


def test_bad_group_and_null_arguments_are_rejected_without_a_device():
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    L = pbc_amd.lib()
    res = np.zeros(v.n, np.uint8)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    for group in (0, 4, -1):
        assert L.pbc_hip_element_membership_batch(H._h, group, ptr(res), ptr(v.g1), v.n) != 0
        assert b"group" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_membership_batch_dev(H._h, group, 0x1000, 0x1000, v.n, None) != 0
        assert b"group" in L.pbc_hip_last_error()
    for args in ((None, ptr(v.g1)), (ptr(res), None)):
        assert L.pbc_hip_element_membership_batch(H._h, 1, args[0], args[1], v.n) != 0
        assert b"null argument" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_membership_batch_dev(H._h, 1, args[0], args[1], v.n, None) != 0
        assert b"null argument" in L.pbc_hip_last_error()
    assert L.pbc_hip_element_membership_batch(None, 1, ptr(res), ptr(v.g1), v.n) != 0
    assert b"null pairing" in L.pbc_hip_last_error()
    assert not res.any()
    with pytest.raises(pbc_amd.PbcHipError, match="group"):
        H.element_membership(0, v.g1)
    with pytest.raises(ValueError):
        H.element_membership(2, v.g1)                            # G1 records where G2 records belong (40 / 120 bytes)
    H.clear()


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    """as test_abi.py test_python_wrappers_reach_the_c_abi_and_fail_loudly_without_a_device"""
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    for group, recs in ((1, v.g1), (2, v.g2), (3, v.gt)):
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_membership(group, recs)
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_membership_dev(group, 0x1000, 0x1000, 4, stream=0)
    H.clear()
