"""CPU tests of the table sets (include/pbc_hip.h pbc_hip_pairing_pp_set_*): the wave planner through
pbc_hip_diag_pp_set_plan; the argument errors of the entry points, which the library reports before it looks for a device;
the lane bodies of the set-init and product kernels compiled for the host next to the host mirror
(tests/hostsim/hostsim_ppset.cpp) against the oracle; the header's citations."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbc_amd
from conftest import ROOT, _param, golden

HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
COUNTS = [0, 1, 63, 64, 65, 0, 130]


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def _plan(H, off):
    off = np.ascontiguousarray(off, np.uint64)
    m = len(off) - 1
    L = pbc_amd.lib()
    need = L.pbc_hip_diag_pp_set_plan(H._h, ctypes.c_void_p(off.ctypes.data), m, None, 0)
    out = np.zeros(need, np.uint64)
    assert L.pbc_hip_diag_pp_set_plan(H._h, ctypes.c_void_p(off.ctypes.data), m, ctypes.c_void_p(out.ctypes.data), need) == need
    return out.reshape(-1, 3)


# ---- the planner ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["a", "d159"])
def test_plan_covers_every_unit_once_in_order(pname):
    """counts [0, 1, 63, 64, 65, 0, 130]: the slots cover every unit exactly once, in order; no slot spans two tables;
    every count is in 1..64; ceil(c / 64) slots per table, none for an empty one"""
    H = pbc_amd.Pairing(_param(pname))
    off = _offsets(COUNTS)
    slots = _plan(H, off)
    assert len(slots) == sum(-(-c // 64) for c in COUNTS) == 8
    nxt = 0
    for table, first, count in slots.astype(np.int64):
        assert 1 <= count <= 64
        assert first == nxt                                              # in order, nothing skipped, nothing twice
        assert off[table] <= first and first + count <= off[table + 1]  # inside ONE table's range
        nxt = first + count
    assert nxt == off[-1]
    assert [int(t) for t in slots[:, 0]] == [1, 2, 3, 4, 4, 6, 6, 6]
    assert [int(c) for c in slots[:, 2]] == [1, 63, 64, 64, 1, 64, 64, 2]
    assert not {0, 5} & set(int(t) for t in slots[:, 0])                 # empty tables get no slot
    H.clear()


def test_plan_refuses_bad_offsets():
    H = pbc_amd.Pairing(_param("a"))
    L = pbc_amd.lib()
    out = np.zeros(64, np.uint64)
    call = lambda off: L.pbc_hip_diag_pp_set_plan(H._h, ctypes.c_void_p(off.ctypes.data), len(off) - 1, ctypes.c_void_p(out.ctypes.data), 64)
    assert call(np.array([1, 2, 3], np.uint64)) == 0                    # offsets[0] != 0
    assert call(np.array([0, 5, 3, 6], np.uint64)) == 0                 # a decreasing pair
    assert not out.any()
    assert call(np.array([0, 5, 5, 6], np.uint64)) == 6                 # two slots; the empty table has none
    assert call(np.array([0, 0, 0], np.uint64)) == 0                    # nothing to do: no slot
    H.clear()


# ---- errors, without a device -----------------------------------------------------------------------------------------
def test_init_errors_come_before_the_device_check():
    L = pbc_amd.lib()
    err = lambda: L.pbc_hip_last_error()
    v = golden("a_rand32.vec")
    H = pbc_amd.Pairing(_param("a"))
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    h = ctypes.c_void_p()
    for init in (lambda o, p, g, m: L.pbc_hip_pairing_pp_set_init(o, p, g, m),
                 lambda o, p, g, m: L.pbc_hip_pairing_pp_set_init_dev(o, p, g, m, None)):
        assert init(None, H._h, ptr(v.g1), 4) != 0 and b"null argument" in err()
        assert init(ctypes.byref(h), None, ptr(v.g1), 4) != 0 and b"null argument" in err()
        assert init(ctypes.byref(h), H._h, None, 4) != 0 and b"null argument" in err()
        assert init(ctypes.byref(h), H._h, ptr(v.g1), 0) != 0 and b"m == 0" in err()
        assert init(ctypes.byref(h), H._h, ptr(v.g1), 1 << 60) != 0 and b"overflow size_t" in err()
        for other in ("e", "f"):
            E = pbc_amd.Pairing(_param(other))
            assert init(ctypes.byref(h), E._h, ptr(v.g1), 2) != 0
            assert b"pairing_pp is built for types a, a1, d and g (other types: use element_pairing)" in err()
            E.clear()
        assert not h.value
    assert L.pbc_hip_pairing_pp_set_count(None) == 0
    L.pbc_hip_pairing_pp_set_clear(None)
    # calls on a set: the null set is refused first
    off = _offsets([1, 2])
    assert L.pbc_hip_pairing_pp_set_apply_batch(None, 1, 1, ptr(off)) != 0 and b"null pp set" in err()
    assert L.pbc_hip_pairing_pp_set_apply_batch_dev(None, 1, 1, ptr(off), None) != 0 and b"null pp set" in err()
    assert L.pbc_hip_pairing_pp_set_prod_batch(None, 1, 1, 1) != 0 and b"null pp set" in err()
    assert L.pbc_hip_pairing_pp_set_prod_batch_dev(None, 1, 1, 1, None) != 0 and b"null pp set" in err()
    H.clear()


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    v = golden("d_rand32.vec")
    H = pbc_amd.Pairing(_param("d159"))
    with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
        H.pp_set_init(v.g1[:3])
    with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
        H.pp_set_init_dev(0x1000, 3)
    with pytest.raises(pbc_amd.PbcHipError, match="m == 0"):
        H.pp_set_init(v.g1[:0])
    H.clear()


# ---- the lane bodies on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ppset_sim():
    """tests/hostsim/hostsim_ppset.cpp built as tests/test_ragged_cpu.py builds its mirror; bound to a.param"""
    lib = os.path.join(HOSTSIM, "libhostsim_ppset.so")
    csrc = os.path.join(ROOT, "pbc_amd", "csrc")
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim_ppset.cpp", "hostsim.cpp", "hostsim_shim.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if (not os.path.exists(lib)) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([CLANG, "-O1", "-Wno-psabi", "-std=c++17", "-fPIC", "-shared", "-I", HOSTSIM, "-o", lib,
                               os.path.join(HOSTSIM, "hostsim_ppset.cpp")])
    L = ctypes.CDLL(lib)
    L.hostsim_init.restype = ctypes.c_void_p
    L.hostsim_init.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.hostsim_ppset_table_words.restype = ctypes.c_size_t
    L.hostsim_ppset_table_words.argtypes = [ctypes.c_void_p]
    L.hostsim_ppset_init.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t]
    L.hostsim_ppset_single_table.argtypes = [ctypes.c_void_p] * 4
    L.hostsim_ppset_prod.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_size_t]
    text = _param("a").encode()
    h = L.hostsim_init(text, len(text))
    assert h
    tw = L.hostsim_ppset_table_words(h)
    assert tw == (159 + 1) * 3 * 16                                     # a.param: exp2 = 159

    class Sim:
        table_words = tw

        @staticmethod
        def init(g1):
            g1 = np.ascontiguousarray(g1, np.uint8)
            m = len(g1)
            tabs, flags = np.full((m, tw), 0xeeeeeeee, np.uint32), np.full(m, 0xee, np.uint32)
            assert L.hostsim_ppset_init(h, tabs.ctypes.data, flags.ctypes.data, g1.ctypes.data, m) == 0
            return tabs, flags

        @staticmethod
        def single(g1):
            g1 = np.ascontiguousarray(g1, np.uint8)
            tab, flag = np.zeros(tw, np.uint32), np.zeros(1, np.uint32)
            assert L.hostsim_ppset_single_table(h, tab.ctypes.data, flag.ctypes.data, g1.ctypes.data) == 0
            return tab, int(flag[0])

        @staticmethod
        def prod(tabs, flags, g2, n):
            g2 = np.ascontiguousarray(g2, np.uint8)
            m = len(tabs)
            assert len(g2) == n * m
            gt = np.full((n, 128), 0xee, np.uint8)
            assert L.hostsim_ppset_prod(h, gt.ctypes.data, tabs.ctypes.data, flags.ctypes.data, g2.ctypes.data, m, n) == 0
            return gt
    return Sim


def test_a_table_of_the_set_is_the_single_table(ppset_sim):
    """the set-init lane writes table after table: table t holds a_pp_init_lane's words for g1[t], flag t its validity
    (an off-curve and an all-zero record among them)"""
    v = golden("a_prod3x10_edge.vec")
    g1 = v.g1[:5].copy()
    g1[1, -1] ^= 1                                                       # off the curve
    g1[3] = 0                                                            # the all-zero record
    tabs, flags = ppset_sim.init(g1)
    assert [int(f) for f in flags] == [1, 0, 1, 0, 1]
    for t in range(len(g1)):
        tab, flag = ppset_sim.single(g1[t])
        assert np.array_equal(tabs[t], tab), t
        assert flag == int(flags[t])
    assert not np.array_equal(tabs[0], tabs[2])


@pytest.mark.parametrize("vec", ["a_prod3x10_edge.vec", "a_prod2x8.vec"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_pp_miller_records_and_finish_against_the_oracle(ppset_sim, oracles, vec, k):
    """pp_miller_record_lane over k consecutive terms of the fixture (tables of the set-init lane), then
    prod_finish_lane: the oracle's element_prod_pairing bytes of the same k terms -- the edge fixture's off-curve and
    all-zero G1 terms included, which make their product the identity.  A window that holds the all-zero G2 record is
    left out: (0, 0) is a finite point to this route as to the uniform entry point (include/pbc_hip.h), and the
    reference divides by zero there."""
    v = golden(vec)
    O = oracles["a"]
    one = O.gt_pow(v.gt[:1], np.zeros((1, 4), np.uint8))[0]
    checked = identities = 0
    for s in range(0, min(len(v.g1) - k + 1, 12), k):
        g1, g2 = v.g1[s:s + k], v.g2[s:s + k]
        if not g2.any(axis=1).all():
            continue
        tabs, flags = ppset_sim.init(g1)
        got = ppset_sim.prod(tabs, flags, g2, 1)
        want = O.prod_pairing_batch(g1, g2, k)[0]
        assert np.array_equal(got[0], want), (vec, s, k)
        if k == v.k and s % v.k == 0:
            assert np.array_equal(got[0], v.gt[s // v.k])
        checked += 1
        identities += np.array_equal(want, one)
    assert checked >= 3 and identities < checked


def test_products_over_one_set_run_term_major(ppset_sim, oracles):
    """n = 3 products over one set of m = 2 tables: unit u of table j reads term record u m + j"""
    v = golden("a_prod2x8.vec")
    O = oracles["a"]
    g1 = v.g1[:2]
    g2 = v.g2[:6]
    tabs, flags = ppset_sim.init(g1)
    got = ppset_sim.prod(tabs, flags, g2, 3)
    want = O.prod_pairing_batch(np.tile(g1, (3, 1)), g2, 2)
    assert np.array_equal(got, want)
    assert len({bytes(r) for r in got}) == 3


# ---- the header -------------------------------------------------------------------------------------------------------------
def test_header_cites_the_reference_for_the_table_sets():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    block = hdr[hdr.index("Table sets:"):hdr.index("pbc_hip_pairing_pp_set_prod_batch_dev")]
    for ref in ("include/pbc_pairing.h:54-89", "ecc/a_param.c:149-220", "ecc/a_param.c:317-360", "ecc/a_param.c:1632-1818",
                "ecc/d_param.c:794-966", "ecc/g_param.c:619-787", "include/pbc_pairing.h:153-171", "example/bls.c:70-78"):
        assert ref in block, ref
    for name in pbc_amd.EXPORTS:
        if "pp_set" in name:
            assert name + "(" in block or name + "(" in hdr[hdr.index("Table sets:"):], name
