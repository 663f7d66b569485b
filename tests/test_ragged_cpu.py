"""CPU tests of the ragged products of pairings (include/pbc_hip.h pbc_hip_element_prod_pairing_ragged_batch): the planner
through pbc_hip_diag_ragged_plan; the lane bodies of the fold and finish kernels compiled for the host next to the host
mirror (tests/hostsim/hostsim_ragged.cpp) against the oracle, product by product; the argument errors, which the library
reports before it looks for a device; the header's citations."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbc_amd
from conftest import ROOT, _param, golden

HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


# ---- the planner ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3, 16])
def test_plan_levels(F):
    """level i + 1 holds ceil(c / F) records per product of c; the last level has every count <= F; empty products stay
    empty at every level; the first array is the caller's"""
    lengths = [0, 1, 2, F - 1, F, F + 1, F * F, F * F + 1, 0]
    H = pbc_amd.Pairing(_param("a") + "hip_ragged_fold %d\n" % F)
    off = _offsets(lengths)
    levels = H.ragged_plan(off)
    assert np.array_equal(levels[0], off)
    counts = [np.diff(lv).astype(np.int64) for lv in levels]
    for lv in levels:
        assert lv[0] == 0 and len(lv) == len(lengths) + 1
    for a, b in zip(counts, counts[1:]):
        assert np.array_equal(b, -(-a // F))
        assert a.max() > F                                  # a level is only folded while some product needs it
    assert counts[-1].max() <= F
    for c in counts:
        assert c[0] == 0 and c[-1] == 0 and c[1] == 1
    # F*F + 1 records: F + 1 after one level, 2 after two
    assert len(levels) == 3 and counts[1][7] == F + 1 and counts[2][7] == 2
    H.clear()


@pytest.mark.parametrize("F", [2, 3, 16])
def test_plan_of_short_products_has_no_fold_level(F):
    H = pbc_amd.Pairing(_param("d159") + "hip_ragged_fold %d\n" % F)
    off = _offsets([F, 0, 1, F, F - 1])
    levels = H.ragged_plan(off)
    assert len(levels) == 1 and np.array_equal(levels[0], off)
    assert len(H.ragged_plan(_offsets([]))) == 1            # n == 0: the one-element array
    H.clear()


def test_fold_factor_is_a_checked_parameter_key():
    assert pbc_amd.Pairing(_param("a")).ragged_plan(_offsets([17]))[-1][-1] == 2          # the default: 16
    assert pbc_amd.Pairing(_param("a") + "hip_ragged_fold 64\n").ragged_plan(_offsets([65]))[-1][-1] == 2
    for bad in (1, 0, 65):
        with pytest.raises(pbc_amd.PbcHipError, match="hip_ragged_fold"):
            pbc_amd.Pairing(_param("a") + "hip_ragged_fold %d\n" % bad)


# ---- the lane bodies on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_sim():
    """tests/hostsim/hostsim_ragged.cpp built as tests/test_coddh_cpu.py builds its mirror"""
    lib = os.path.join(HOSTSIM, "libhostsim_ragged.so")
    csrc = os.path.join(ROOT, "pbc_amd", "csrc")
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim_ragged.cpp", "hostsim.cpp", "hostsim_shim.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if (not os.path.exists(lib)) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([CLANG, "-O1", "-Wno-psabi", "-std=c++17", "-fPIC", "-shared", "-I", HOSTSIM, "-o", lib,
                               os.path.join(HOSTSIM, "hostsim_ragged.cpp")])
    L = ctypes.CDLL(lib)
    L.hostsim_init.restype = ctypes.c_void_p
    L.hostsim_init.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.hostsim_ragged.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def run(pname, g1, g2, off, F):
        text = _param(pname).encode()
        h = L.hostsim_init(text, len(text))
        assert h
        g1, g2 = np.ascontiguousarray(g1, np.uint8), np.ascontiguousarray(g2, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        lens = [ctypes.c_int() for _ in range(3)]
        assert L.hostsim_lens(ctypes.c_void_p(h), *[ctypes.byref(x) for x in lens]) == 0
        gt = np.full((n, lens[2].value), 0xee, np.uint8)
        levels = ctypes.c_int(-1)
        assert L.hostsim_ragged(h, gt.ctypes.data, g1.ctypes.data, g2.ctypes.data, off.ctypes.data, n, F, ctypes.byref(levels)) == 0
        return gt, levels.value
    return run


def _identity(O, some_gt):
    return O.gt_pow(some_gt[:1], np.zeros((1, 4), np.uint8))[0]


@pytest.mark.parametrize("pname,vec", [("a", "a_prod16x4.vec"), ("d159", "d_prod16x4.vec"), ("f", "f_prod4x3.vec")])
def test_lane_bodies_on_host(ragged_sim, oracles, pname, vec):
    """lengths [3, 0, 1, 5, 2] with hip_ragged_fold 2: the product of 5 terms crosses two fold levels (5 -> 3 -> 2), the
    one of 3 one, the others none.  a.param: the record route (Miller records folded, one final exponentiation per
    product); d159, f: the GT route.  Expected: the oracle's element_prod_pairing per product, the identity for the
    empty one."""
    v = golden(vec)
    lengths = [3, 0, 1, 5, 2]
    off = _offsets(lengths)
    T = int(off[-1])
    assert T <= len(v.g1)
    g1, g2 = v.g1[:T], v.g2[:T]
    O = oracles[pname]
    one = _identity(O, v.gt)
    got, levels = ragged_sim(pname, g1, g2, off, 2)
    assert levels == 2
    for u, c in enumerate(lengths):
        a, b = int(off[u]), int(off[u + 1])
        want = O.prod_pairing_batch(g1[a:b], g2[a:b], c)[0] if c else one
        assert np.array_equal(got[u], want), (u, c)
    assert not np.array_equal(got[0], one) and np.array_equal(got[1], one)


def test_lane_bodies_carry_validity_apart_from_values(ragged_sim, oracles):
    """d159, fold 2, products [5, 3]: an all-zero G1 record as the LAST term of the first product (it travels through two
    levels as a one-record block whose value is the identity's bytes) makes that product the identity; its
    neighbour keeps the oracle's value"""
    v = golden("d_prod16x4.vec")
    off = _offsets([5, 3])
    g1, g2 = v.g1[:8].copy(), v.g2[:8].copy()
    g1[4] = 0
    O = oracles["d159"]
    got, _ = ragged_sim("d159", g1, g2, off, 2)
    assert np.array_equal(got[0], _identity(O, v.gt))
    assert np.array_equal(got[1], O.prod_pairing_batch(g1[5:8], g2[5:8], 3)[0])


def test_all_zero_g2_record_on_type_a_makes_its_product_the_identity(ragged_sim, oracles):
    """a.param, the record route: (0, 0) is a finite point of y^2 = x^3 + x, which the Miller kernel accepts (its pairing
    value is 1), but the all-zero record is O to every entry point: the product that holds it is the identity, its
    neighbour is not.  Also as the all-zero G1 record and as off-curve records on either side."""
    v = golden("a_prod16x4.vec")
    O = oracles["a"]
    one = _identity(O, v.gt)
    off = _offsets([3, 2])
    want1 = O.prod_pairing_batch(v.g1[3:5], v.g2[3:5], 2)[0]
    for group, zero in ((2, True), (1, True), (2, False), (1, False)):
        g1, g2 = v.g1[:5].copy(), v.g2[:5].copy()
        rec = (g1 if group == 1 else g2)[1]
        if zero:
            rec[:] = 0
        else:
            rec[-1] ^= 1
        got, _ = ragged_sim("a", g1, g2, off, 2)
        assert np.array_equal(got[0], one), (group, zero)
        assert np.array_equal(got[1], want1) and not np.array_equal(want1, one)


# ---- errors, without a device -----------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device_check():
    H = pbc_amd.Pairing(_param("a"))
    L = pbc_amd.lib()
    v = golden("a_rand32.vec")
    gt = np.zeros((4, 128), np.uint8)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    host = lambda off, g=gt, a=v.g1, b=v.g2, h=H._h, n=None: L.pbc_hip_element_prod_pairing_ragged_batch(
        h, None if g is None else ptr(g), None if a is None else ptr(a), None if b is None else ptr(b),
        None if off is None else ptr(off), len(off) - 1 if n is None else n)
    dev = lambda off, g=0x1000, h=H._h, n=None: L.pbc_hip_element_prod_pairing_ragged_batch_dev(
        h, g, 0x1000, 0x1000, None if off is None else ptr(off), len(off) - 1 if n is None else n, None)
    err = lambda: L.pbc_hip_last_error()
    good = _offsets([1, 2, 0, 3])
    for call in (host, dev):
        assert call(good, h=None) != 0 and b"null pairing" in err()
        assert call(None, n=4) != 0 and b"null argument" in err()
        assert call(good, g=None) != 0 and b"null argument" in err()
        assert call(np.array([1, 2, 3], np.uint64)) != 0 and b"offsets[0] must be 0" in err()
        assert call(np.array([0, 5, 3, 6], np.uint64)) != 0 and b"decrease at index 1" in err()
        assert call(np.array([0, 1, (1 << 22) + 2], np.uint64)) != 0 and b"more than 2^22" in err()
        assert call(np.array([0], np.uint64)) == 0                              # n == 0
    assert host(good, a=None) != 0 and b"null argument" in err()
    assert host(good, b=None) != 0 and b"null argument" in err()
    assert len(H.ragged_plan(np.array([0, 1 << 22, 1 << 23], np.uint64))) > 1                 # 2^22 terms in a product are allowed
    assert not gt.any()
    with pytest.raises(ValueError):
        H.element_prod_pairing_ragged(v.g1[:5], v.g2[:6], good)
    with pytest.raises(ValueError):
        H.element_prod_pairing_ragged(v.g1[:6], v.g2[:6], [])
    H.clear()


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
        H.element_prod_pairing_ragged(v.g1[:6], v.g2[:6], _offsets([1, 2, 0, 3]))
    with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
        H.element_prod_pairing_ragged_dev(0x1000, 0x1000, 0x1000, _offsets([1, 2, 0, 3]), stream=0)
    assert H.element_prod_pairing_ragged(v.g1[:0], v.g2[:0], [0]).shape == (0, v.lenT)
    H.clear()


def test_header_cites_the_reference_for_the_ragged_products():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    block = hdr[hdr.index("Ragged products"):hdr.index("pbc_hip_element_prod_pairing_ragged_batch_dev")]
    for ref in ("include/pbc_pairing.h:153-171", "include/pbc_pairing.h:161-168", "ecc/a_param.c:1283", "ecc/pairing.c:35-46", "hip_ragged_fold"):
        assert ref in block, ref
    plan = hdr[hdr.index("pbc_hip_element_prod_pairing_ragged_batch_dev"):hdr.index("pbc_hip_diag_ragged_plan")]
    assert "ecc/pairing.c:35-46" in plan
