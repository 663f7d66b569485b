"""CPU tests of is_almost_coddh (include/pbc_hip.h: pbc_hip_is_almost_coddh_batch): the lane body of
coddh_verdict_kernel (group_more.cuh coddh_verdict_lane) compiled for the host next to the host mirror
(tests/hostsim/hostsim_coddh.cpp), on GT values of the reference's fixtures and their inverses from the oracle; the
Python wrappers as far as the C entry points; the header's citations."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbc_amd
from conftest import ROOT, _param, golden, param_value

HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
# family -> (parameter file, its random single-pairing fixture, the key of the group order in the parameter text)
FAMILIES = {"a": ("a", "a_rand32.vec", "r"), "a1": ("a1", "a1_rand6.vec", "n"), "d159": ("d159", "d_rand32.vec", "r"),
            "e": ("e", "e_rand6.vec", "r"), "f": ("f", "f_rand16.vec", "r"), "g149": ("g149", "g149_rand16.vec", "r")}


@pytest.fixture(scope="module")
def coddh_sim():
    """tests/hostsim/hostsim_coddh.cpp built as tests/hostsim/__init__.py builds hostsim.cpp"""
    lib = os.path.join(HOSTSIM, "libhostsim_coddh.so")
    csrc = os.path.join(ROOT, "pbc_amd", "csrc")
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim_coddh.cpp", "hostsim.cpp", "hostsim_shim.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if (not os.path.exists(lib)) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([CLANG, "-O1", "-Wno-psabi", "-std=c++17", "-fPIC", "-shared", "-I", HOSTSIM, "-o", lib,
                               os.path.join(HOSTSIM, "hostsim_coddh.cpp")])
    L = ctypes.CDLL(lib)
    L.hostsim_init.restype = ctypes.c_void_p
    L.hostsim_init.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.hostsim_coddh.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_int]
    handles = {}

    def verdicts(family, t0, t1, almost):
        if family not in handles:
            text = _param(FAMILIES[family][0]).encode()
            handles[family] = L.hostsim_init(text, len(text))
            assert handles[family]
        t0 = np.ascontiguousarray(t0, np.uint8)
        t1 = np.ascontiguousarray(t1, np.uint8)
        assert t0.shape == t1.shape
        res = np.full(len(t0), 0xee, np.uint8)
        assert L.hostsim_coddh(handles[family], res.ctypes.data, t0.ctypes.data, t1.ctypes.data, len(t0), 1 if almost else 0) == 0
        return res
    return verdicts


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_verdict_lane_on_host(coddh_sim, oracles, family):
    """the table of the definition on the reference's GT values T_i: (T, T) 1/1; (T, T^(r-1)) 1/0 (ALMOST/EXACT);
    (T_i, T_i+1) what the bytes say (0); (1, 1) 1/1; (T, 1) 0/0.  Expected values: the fixture's bytes and the oracle."""
    pname, vec, rkey = FAMILIES[family]
    T = golden(vec).gt
    n, lt = T.shape
    r = param_value(pname, rkey)
    elen = (r.bit_length() + 7) // 8
    O = oracles[pname]
    e_inv = np.tile(np.frombuffer((r - 1).to_bytes(elen, "big"), np.uint8), (n, 1))
    Tinv = O.gt_pow(T, e_inv)
    one = O.gt_pow(T[:1], np.zeros((1, elen), np.uint8))
    ones = np.tile(one, (n, 1))
    assert np.array_equal(O.gt_mul(T, Tinv), ones)                 # T^(r-1) is the inverse, 1 is the identity
    assert not (T == ones).all(axis=1).any()                       # T_i != 1
    assert not (T == Tinv).all(axis=1).any()                       # (r odd: T_i != T_i^-1)
    nxt = np.roll(T, -1, axis=0)
    neighbours = (T == nxt).all(axis=1).astype(np.uint8)
    assert not neighbours.any()
    for almost in (True, False):
        assert np.array_equal(coddh_sim(family, T, T, almost), np.ones(n, np.uint8))
        assert np.array_equal(coddh_sim(family, T, Tinv, almost), np.full(n, 1 if almost else 0, np.uint8))
        assert np.array_equal(coddh_sim(family, Tinv, T, almost), np.full(n, 1 if almost else 0, np.uint8))
        assert np.array_equal(coddh_sim(family, T, nxt, almost), neighbours)
        assert np.array_equal(coddh_sim(family, ones, ones, almost), np.ones(n, np.uint8))
        assert np.array_equal(coddh_sim(family, T, ones, almost), np.zeros(n, np.uint8))
        assert np.array_equal(coddh_sim(family, ones, T, almost), np.zeros(n, np.uint8))


def test_verdict_lane_compares_values_not_images(coddh_sim, oracles):
    """two byte images of one field element (a coordinate x and x + q, which fits the record of a.param) are equal"""
    T = golden("a_rand32.vec").gt
    q = param_value("a", "q")
    fb = T.shape[1] // 2
    alt = T.copy()
    changed = 0
    for i in range(len(T)):
        x = int.from_bytes(T[i, :fb].tobytes(), "big")
        if x + q < 1 << (8 * fb):
            alt[i, :fb] = np.frombuffer((x + q).to_bytes(fb, "big"), np.uint8)
            changed += 1
    assert changed and not np.array_equal(alt, T)
    for almost in (True, False):
        assert np.array_equal(coddh_sim("a", T, alt, almost), np.ones(len(T), np.uint8))


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    """as test_abi.py test_python_wrappers_reach_the_c_abi_and_fail_loudly_without_a_device: both forms get as far as the
    library and come back with its 'no HIP device' error"""
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    for exact in (False, True):
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.is_almost_coddh(v.g1, v.g1, v.g2, v.g2, exact=exact)
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.is_almost_coddh_dev(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 4, exact=exact, stream=0)
    with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
        H.is_almost_coddh(v.g1[:0], v.g1[:0], v.g2[:0], v.g2[:0])      # n == 0: as element_pairing_batch, the device check first
    H.clear()


def test_bad_mode_and_mismatched_lengths_are_rejected():
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    L = pbc_amd.lib()
    res = np.zeros(v.n, np.uint8)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    for mode in (2, -1, 7):
        assert L.pbc_hip_is_almost_coddh_batch(H._h, ptr(res), ptr(v.g1), ptr(v.g1), ptr(v.g2), ptr(v.g2), v.n, mode) != 0
        assert b"mode" in L.pbc_hip_last_error()
        assert L.pbc_hip_is_almost_coddh_batch_dev(H._h, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, v.n, mode, None) != 0
        assert b"mode" in L.pbc_hip_last_error()
    assert L.pbc_hip_is_almost_coddh_batch(None, ptr(res), ptr(v.g1), ptr(v.g1), ptr(v.g2), ptr(v.g2), v.n, 0) != 0
    assert b"null pairing" in L.pbc_hip_last_error()
    assert not res.any()
    with pytest.raises(ValueError):
        H.is_almost_coddh(v.g1, v.g1[:-1], v.g2, v.g2)
    with pytest.raises(ValueError):
        H.is_almost_coddh(v.g1, v.g1, v.g2[:-1], v.g2)
    with pytest.raises(ValueError):
        H.is_almost_coddh(v.g1, v.g1, v.g2, v.g1)                      # G1 records where G2 records belong (40 / 120 bytes)
    H.clear()


def test_header_cites_the_reference_for_is_almost_coddh():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    at = hdr.index("is_almost_coddh")
    block = hdr[at:hdr.index("pbc_hip_is_almost_coddh_batch_dev")]
    for ref in ("include/pbc_pairing.h:240", "ecc/pairing.c:15", "ecc/d_param.c:739", "example/bls.c:97"):
        assert ref in block, ref
    assert pbc_amd.CODDH_ALMOST == 0 and pbc_amd.CODDH_EXACT == 1
    assert "#define PBC_HIP_CODDH_ALMOST 0" in hdr and "#define PBC_HIP_CODDH_EXACT  1" in hdr
