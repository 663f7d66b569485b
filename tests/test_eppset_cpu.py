"""CPU tests of the fixed-base table sets (include/pbc_hip.h pbc_hip_element_pp_set_*): the argument errors of the entry
points, which the library reports before it looks for a device; the lane bodies of the kernels (group_ppset.cuh) compiled
for the host next to the host mirror (tests/hostsim/hostsim_eppset.cpp) -- the set's entry lane, the segmented power, the
fast and the complete multi-base lane, the GT lanes -- on the batteries of tests/eppset_battery.py, whose expected records
are exact-integer results of tests/intref.py; the battery's own claims about the rows that cancel and meet."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import eppset_battery as eb
import intref
import pbc_amd
from conftest import ROOT, _param, golden

HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
# (parameter set, group): G2 of the symmetric types is G1's curve and runs the same lanes
POINT_SETS = [("a", 1), ("d159", 1), ("d159", 2), ("f", 1), ("f", 2), ("g149", 1), ("e", 1), ("a_160_256", 1), ("a1", 1)]
GT_SETS = ["a", "d159", "f", "g149", "e", "a_160_256", "a1"]


def m_of(name, group):
    """bases of the sets the mirror runs: a1 at most 2 (an entry of its table is a 1032-bit ladder on 33 words); the other
    33-word set and the twists 3"""
    if name == "a1":
        return 2
    return 3 if eb._thin(name, group) else 5


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/hostsim_eppset.cpp built as tests/test_mpz_cpu.py builds hostsim_mpz.cpp"""
    lib = os.path.join(HOSTSIM, "libhostsim_eppset.so")
    csrc = os.path.join(ROOT, "pbc_amd", "csrc")
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim_eppset.cpp", "hostsim.cpp", "hostsim_shim.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if (not os.path.exists(lib)) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([CLANG, "-O1", "-Wno-psabi", "-std=c++17", "-fPIC", "-shared", "-I", HOSTSIM, "-o", lib,
                               os.path.join(HOSTSIM, "hostsim_eppset.cpp")])
    L = ctypes.CDLL(lib)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.hostsim_init.restype = vp
    L.hostsim_init.argtypes = [ctypes.c_char_p, sz]
    L.hostsim_eppset_entries.restype = sz
    L.hostsim_eppset_entries.argtypes = [vp, ci]
    L.hostsim_eppset_table_words.restype = sz
    L.hostsim_eppset_table_words.argtypes = [vp, ci]
    L.hostsim_eppset_tables.argtypes = [vp, ci, vp, vp, vp, sz, vp, sz]
    L.hostsim_eppset_single_table.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.hostsim_eppset_prod.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, sz, vp, sz]
    L.hostsim_eppset_pow.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, sz, vp, vp]
    handles = {}

    class Sim:
        @staticmethod
        def handle(name):
            if name not in handles:
                text = _param(name).encode()
                handles[name] = L.hostsim_init(text, len(text))
                assert handles[name]
            return handles[name]

        @staticmethod
        def shape(name, group):
            h = Sim.handle(name)
            return L.hostsim_eppset_entries(h, group), L.hostsim_eppset_table_words(h, group)

        @staticmethod
        def units_of(name, group, zr, m, table=None):
            """the table entries the scalars of `zr` ((n, m' * zl) bytes) select: unit numbers of the set.  table: the rows
            hold ONE scalar each, all for that table (a segment)"""
            zl = intref.fam(name).zl
            per, _ = Sim.shape(name, group)
            want = set()
            if not len(zr):
                return want
            z = np.ascontiguousarray(zr, np.uint8).reshape(len(zr), -1, zl)
            for j in range(z.shape[1]):
                t = j if table is None else table
                for row in range(zl):
                    ws = np.unique(z[:, j, zl - 1 - row])
                    for w in ws:
                        if group == 3:
                            want.add(t * per + row * 256 + int(w))
                        elif w:
                            want.add(t * per + row * 255 + int(w) - 1)
            return want

        @staticmethod
        def tables(name, group, bases, units=None):
            """-> tabs (m, words) uint32, entry flags (m, entries) uint8 (0xEE where no entry was built); units: the entries
            to build (None: all of them)"""
            h = Sim.handle(name)
            bases = np.ascontiguousarray(bases, np.uint8)
            m = len(bases)
            per, tw = Sim.shape(name, group)
            tabs, ef = np.zeros((m, tw), np.uint32), np.full((m, per), 0xEE, np.uint8)
            if units is None:
                assert L.hostsim_eppset_tables(h, group, tabs.ctypes.data, ef.ctypes.data, bases.ctypes.data, m, None, 0) == 0
            else:
                u = np.array(sorted(units), np.uint64)
                assert L.hostsim_eppset_tables(h, group, tabs.ctypes.data, ef.ctypes.data, bases.ctypes.data, m, u.ctypes.data, len(u)) == 0
            return tabs, ef

        @staticmethod
        def single_table(name, group, base, units):
            """the entries `units` (numbers within the table) of the single-base object's table, the rest zero / 0xEE"""
            h = Sim.handle(name)
            base = np.ascontiguousarray(base, np.uint8)
            per, tw = Sim.shape(name, group)
            tab, ef = np.zeros(tw, np.uint32), np.full(per, 0xEE, np.uint8)
            u = np.array(sorted(units), np.uint64)
            assert L.hostsim_eppset_single_table(h, group, tab.ctypes.data, ef.ctypes.data, base.ctypes.data, u.ctypes.data, len(u)) == 0
            return tab, ef

        @staticmethod
        def prod(name, group, mode, complete_only, tabs, bases, zr):
            """-> records (0xEE where a lane wrote nothing), the fast lane's flags"""
            h = Sim.handle(name)
            bases, zr = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(zr, np.uint8)
            m, n = len(bases), len(zr)
            assert zr.shape[1] == m * intref.fam(name).zl
            out, flags = np.full((n, bases.shape[1]), 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
            assert L.hostsim_eppset_prod(h, group, mode, int(complete_only), out.ctypes.data, flags.ctypes.data, tabs.ctypes.data, bases.ctypes.data, m,
                                         zr.ctypes.data, n) == 0
            return out, flags

        @staticmethod
        def pow(name, group, mode, tabs, tflags, bases, zr, offsets):
            h = Sim.handle(name)
            bases, zr = np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(zr, np.uint8)
            off, tf = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(tflags, np.uint8)
            n = int(off[-1])
            out, flags = np.full((n, bases.shape[1]), 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
            assert L.hostsim_eppset_pow(h, group, mode, out.ctypes.data, flags.ctypes.data, tabs.ctypes.data, tf.ctypes.data, bases.ctypes.data, len(bases),
                                        zr.ctypes.data, off.ctypes.data) == 0
            return out, flags
    return Sim


def _bad(got, want, labels):
    return [(labels[i], got[i].tobytes().hex()[:16], want[i].tobytes().hex()[:16]) for i in range(len(want)) if not np.array_equal(got[i], want[i])]


# ---- the battery's own claims, intref alone --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", [("a", 1), ("d159", 1), ("f", 1), ("f", 2)])
def test_battery_rows_cancel_and_meet_where_they_say(name, group):
    """the cancelling rows sum to O, the meeting rows do not all; every one of them reaches an equal or opposite step of
    the fast lane's walk over the exact table entries, the all-zero row and the uniformly random rows on distinct fixture
    bases reach none"""
    m = m_of(name, group)
    labels = [lab for lab, _ in eb.rows(name, group, "related")]
    hit = eb.exceptional(name, group, "related", m)
    want = eb.expected(name, group, "related", m)
    seen = {"cancel": 0, "meet": 0}
    for i, lab in enumerate(labels):
        if lab.startswith("cancel"):
            assert hit[i] and not want[i].any(), lab
            seen["cancel"] += 1
        elif lab.startswith("meet"):
            assert hit[i], lab
            seen["meet"] += 1
        elif lab == "all zero" or lab.startswith("byte "):
            assert not hit[i], lab
    assert seen["cancel"] >= 3 and seen["meet"] >= 3
    assert any(want[labels.index(lab)].any() for lab in labels if lab.startswith("meet"))     # a met step is not a sum of O
    dl = [lab for lab, _ in eb.rows(name, group, "distinct")]
    dh = eb.exceptional(name, group, "distinct", m)
    rnd = [i for i, lab in enumerate(dl) if lab.startswith("random")]
    assert len(rnd) >= 3 and not dh[rnd].any()
    assert not dh[dl.index("all zero")]


# ---- the lanes on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", POINT_SETS)
def test_multi_base_lanes_on_host(sim, name, group):
    """kinds "distinct" and "related": the library's route and the complete lane alone give intref's record for every row;
    the fast lane flags EXACTLY the rows intref's walk says meet an equal or opposite step (a sum of O with a non-zero
    scalar byte among them), writes nothing for them (the record stays 0xEE), is right wherever it raised no flag, and
    flags none of the random rows on distinct bases.  The all-zero row is O without a flag: no step is taken"""
    m = m_of(name, group)
    for kind in ("distinct", "related"):
        bases = eb.base_set(name, group, kind)[0][:m]
        labels = [lab for lab, _ in eb.rows(name, group, kind)]
        zr = eb.zr_bytes(name, group, kind, m)
        want = eb.expected(name, group, kind, m)
        tabs, ef = sim.tables(name, group, bases, sim.units_of(name, group, zr, m))
        assert not (ef == 1).any()                               # no entry is O: no table is "complete only"
        got, flags = sim.prod(name, group, 0, False, tabs, bases, zr)
        assert not _bad(got, want, labels), kind
        slow, none = sim.prod(name, group, 1, False, tabs, bases, zr)
        assert not _bad(slow, want, labels) and not none.any(), kind
        fast, flags2 = sim.prod(name, group, 2, False, tabs, bases, zr)
        assert np.array_equal(flags, flags2) and set(flags) <= {0, 1}
        hit = eb.exceptional(name, group, kind, m)
        assert np.array_equal(flags == 1, hit), (kind, [labels[i] for i in np.nonzero((flags == 1) != hit)[0]])
        assert np.array_equal(fast[~hit], want[~hit]) and (fast[hit] == 0xEE).all(), kind
        zero = labels.index("all zero")
        assert not want[zero].any() and not hit[zero]
        if kind == "distinct":
            assert not any(hit[i] for i, lab in enumerate(labels) if "random" in lab)
        elif m >= 2:
            assert hit.any()


@pytest.mark.parametrize("name,group", POINT_SETS)
def test_crafted_bases_take_the_complete_lane_on_host(sim, name, group):
    """kinds "crafted" and "complete": O, an off-curve record and a point of small order raise an entry flag, the set is
    "complete only", and the complete lane gives intref's record for every row -- the library's route is that lane"""
    for kind in ("crafted", "complete"):
        recs, blabels, pts = eb.base_set(name, group, kind)
        m = min(len(recs), m_of(name, group) if name != "a1" else 2)
        bases = recs[:m]
        labels = [lab for lab, _ in eb.rows(name, group, kind)]
        zr = eb.zr_bytes(name, group, kind, m)
        want = eb.expected(name, group, kind, m)
        got, flags = sim.prod(name, group, 0, True, np.zeros((m, 1), np.uint32), bases, zr)
        assert not _bad(got, want, labels), kind
        assert not flags.any()
        if eb._thin(name, group) or name == "a":
            continue                                             # (an entry of these tables costs milliseconds: the flags are shown on the narrow sets)
        per, _ = sim.shape(name, group)
        # the entries of row 0 and of the top row: a base that is O or off the curve flags every one of them, a point of
        # order k every k-th of a row
        units = [t * per + e for t in range(m) for e in list(range(255)) + list(range(per - 255, per))]
        _, ef = sim.tables(name, group, bases, units)
        for t in range(m):
            built = ef[t][ef[t] != 0xEE]
            if blabels[t] in ("O", "off curve"):
                assert (built == 1).all(), blabels[t]
            elif blabels[t].startswith("order "):
                k = int(blabels[t].split()[1])
                assert (ef[t][:255] == [1 if (w + 1) % k == 0 else 0 for w in range(255)]).all(), blabels[t]
            else:
                assert not built.any(), blabels[t]


@pytest.mark.parametrize("name", GT_SETS)
def test_gt_lanes_on_host(sim, name):
    """GT: the plain product of the selected entries is intref's product of powers, a repeated base, a record with
    coordinates >= q, the identity and an element outside the subgroup included"""
    m = m_of(name, 3)
    for kind in ("distinct", "related"):
        bases = eb.base_set(name, 3, kind)[0][:m]
        labels = [lab for lab, _ in eb.rows(name, 3, kind)]
        zr = eb.zr_bytes(name, 3, kind, m)
        tabs, _ = sim.tables(name, 3, bases, sim.units_of(name, 3, zr, m))
        got, flags = sim.prod(name, 3, 0, False, tabs, bases, zr)
        assert not _bad(got, eb.expected(name, 3, kind, m), labels), kind
        assert not flags.any()
        one = sim.prod(name, 3, 0, False, tabs, bases[:1], zr[:, :intref.fam(name).zl])[0]
        assert not _bad(one, eb.single(name, 3, kind, 0), labels), kind


@pytest.mark.parametrize("name,group", [("a", 1), ("d159", 1), ("d159", 2), ("f", 2), ("a", 3), ("d159", 3), ("e", 1)])
def test_segmented_power_on_host(sim, name, group):
    """segments over the bases of kind "crafted" (GT: "related") with an empty table in front and in the middle: every
    unit finds its table, a "complete only" table's units go to the complete ladder, and segment t equals [z] B_t"""
    kind = "related" if group == 3 else "crafted"
    recs = eb.base_set(name, group, kind)[0]
    m = len(recs) if not eb._thin(name, group) else 3
    zl = intref.fam(name).zl
    zall = eb.zr_bytes(name, group, kind, len(recs))
    rows_n = len(zall)
    # table t serves counts[t] units: the t-th scalars of the LAST counts[t] rows (the random rows are among them)
    counts = [4, 0, 4][:m] if eb._thin(name, group) else [0, rows_n, 0, 2, rows_n][:m]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    seg = lambda a, t, c: a[len(a) - c:, t * zl:(t + 1) * zl] if a is zall else a[len(a) - c:]
    zr = np.concatenate([seg(zall, t, c) for t, c in enumerate(counts)])
    want = np.concatenate([seg(eb.single(name, group, kind, t), t, c) for t, c in enumerate(counts)])
    labels = ["table %d unit %d" % (t, i) for t, c in enumerate(counts) for i in range(c)]
    bases = recs[:m]
    if group == 3:
        units = set()
        for t, c in enumerate(counts):
            units |= sim.units_of(name, 3, seg(zall, t, c), 1, table=t)
        tabs, _ = sim.tables(name, 3, bases, units)
        got, _ = sim.pow(name, 3, 0, tabs, np.zeros(m, np.uint8), bases, zr, off)
        assert not _bad(got, want, labels)
        return
    blabels = eb.base_set(name, group, kind)[1][:m]
    tflags = np.array([0 if lab.startswith("fixture") else 1 for lab in blabels], np.uint8)
    units = set()
    for t, c in enumerate(counts):
        if not tflags[t]:
            units |= sim.units_of(name, group, seg(zall, t, c), 1, table=t)
    tabs, ef = sim.tables(name, group, bases, units)
    assert not (ef == 1).any()
    got, flags = sim.pow(name, group, 0, tabs, tflags, bases, zr, off)
    assert not _bad(got, want, labels)
    slow, none = sim.pow(name, group, 1, tabs, tflags, bases, zr, off)
    assert not _bad(slow, want, labels) and not none.any()
    fast, flags2 = sim.pow(name, group, 2, tabs, tflags, bases, zr, off)
    assert np.array_equal(flags, flags2)
    t_of = np.repeat(np.arange(m), counts)
    assert flags[tflags[t_of] == 1].all()                        # a "complete only" table: every unit reported
    assert np.array_equal(fast[flags == 0], want[flags == 0]) and (fast[flags == 1] == 0xEE).all()


@pytest.mark.parametrize("name,group", [("d159", 1), ("f", 2), ("d159", 3)])
def test_a_table_of_the_set_is_the_single_base_table(sim, name, group):
    """m = 3: table t of the set equals, word for word, the table the single-base object's entry lane derives from
    bases[t], entry flags included (bases: a fixture point, O, an off-curve record; GT: a repeated base among them) --
    on row 0 and every 8th entry of the top row, the entries the mirror builds in seconds"""
    kind = "related" if group == 3 else "crafted"
    bases = eb.base_set(name, group, kind)[0][:3]
    per, tw = sim.shape(name, group)
    rl = per // intref.fam(name).zl                             # entries of a row: 255, GT 256
    ent = list(range(rl)) + list(range(per - rl, per, 8))        # row 0, and every 8th entry of the top row
    tabs, ef = sim.tables(name, group, bases, [t * per + e for t in range(3) for e in ent])
    we = tw // per
    for t in range(3):
        one, of = sim.single_table(name, group, bases[t], ent)
        assert np.array_equal(tabs[t], one), t
        if group != 3:
            assert np.array_equal(ef[t], of), t
    top = tabs[0][(per - rl) * we:(per - rl + 1) * we]          # the first entry of the top row
    assert tabs[0][:rl * we].any() and top.any() and not np.array_equal(tabs[0], tabs[2])


# ---- the C-ABI and the Python wrappers -----------------------------------------------------------------------------------
NAMES = ("pbc_hip_element_pp_set_init", "pbc_hip_element_pp_set_init_dev", "pbc_hip_element_pp_set_clear", "pbc_hip_element_pp_set_count",
         "pbc_hip_element_pp_set_pow_zn_batch", "pbc_hip_element_pp_set_pow_zn_batch_dev", "pbc_hip_element_pp_set_prod_batch",
         "pbc_hip_element_pp_set_prod_batch_dev", "pbc_hip_diag_element_pp_set_offsets")


def test_exports_and_header_agree():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(pbc_amd.LIB_PATH)
    for sym in NAMES:
        assert re.search(r"\b%s\s*\(" % sym, code) and sym in pbc_amd.EXPORTS and hasattr(L, sym), sym
    block = hdr[hdr.index("Sets of fixed-base tables"):hdr.index("typedef struct pbc_hip_element_pp_set_s")]
    for ref in ("include/pbc_field.h:591-625", "arith/field.c:243-323", "include/pbc_field.h:280", "element_build_base_table", "HOST memory",
                "offsets[0] == 0", "complete only", "may not alias", "pbc_hip_element_pow2_zn_batch"):
        assert ref in block, ref
    for cls in ("ElementPPSet",):
        for meth in ("pow_zn", "pow_zn_dev", "prod", "prod_dev", "count", "clear"):
            assert callable(getattr(getattr(pbc_amd, cls), meth))
    assert callable(pbc_amd.Pairing.element_pp_set_init)


def test_bad_arguments_are_rejected_without_a_device():
    """null arguments, group outside 1..3, m == 0, table bytes that overflow size_t, offsets[0] != 0, a decreasing pair of
    offsets: non-zero with the message, before a device is looked for"""
    L = pbc_amd.lib()
    err = lambda: L.pbc_hip_last_error()
    v = golden("d_rand32.vec")
    H = pbc_amd.Pairing(_param("d159"))
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    h = ctypes.c_void_p()
    for init in (lambda o, p, g, b, m: L.pbc_hip_element_pp_set_init(o, p, g, b, m),
                 lambda o, p, g, b, m: L.pbc_hip_element_pp_set_init_dev(o, p, g, b, m, None)):
        assert init(None, H._h, 1, ptr(v.g1), 4) != 0 and b"null argument" in err()
        assert init(ctypes.byref(h), None, 1, ptr(v.g1), 4) != 0 and b"null argument" in err()
        assert init(ctypes.byref(h), H._h, 1, None, 4) != 0 and b"null argument" in err()
        for group in (0, 4, -1):
            assert init(ctypes.byref(h), H._h, group, ptr(v.g1), 4) != 0 and b"group must be 1, 2 or 3" in err()
        for group in (1, 2, 3):
            assert init(ctypes.byref(h), H._h, group, ptr(v.g1), 0) != 0 and b"m == 0" in err()
            assert init(ctypes.byref(h), H._h, group, ptr(v.g1), 1 << 60) != 0 and b"overflow size_t" in err()
        assert not h.value
    assert L.pbc_hip_element_pp_set_count(None) == 0
    L.pbc_hip_element_pp_set_clear(None)
    off = np.array([0, 1, 3], np.uint64)
    assert L.pbc_hip_element_pp_set_pow_zn_batch(None, 1, 1, ptr(off)) != 0 and b"null element_pp set" in err()
    assert L.pbc_hip_element_pp_set_pow_zn_batch_dev(None, 1, 1, ptr(off), None) != 0 and b"null element_pp set" in err()
    assert L.pbc_hip_element_pp_set_prod_batch(None, 1, 1, 1) != 0 and b"null element_pp set" in err()
    assert L.pbc_hip_element_pp_set_prod_batch_dev(None, 1, 1, 1, None) != 0 and b"null element_pp set" in err()
    # the offsets of a call, as the two pow_zn entry points check them
    chk = lambda o, m: L.pbc_hip_diag_element_pp_set_offsets(ptr(o), m)
    assert chk(np.array([1, 2, 3], np.uint64), 2) != 0 and b"offsets[0] must be 0 (got 1)" in err()
    assert chk(np.array([0, 5, 3, 6], np.uint64), 3) != 0 and b"offsets decrease at index 1 (5 > 3)" in err()
    assert chk(np.array([0, 5, 5, 6], np.uint64), 3) == 0
    assert chk(np.array([0, 0, 0], np.uint64), 2) == 0
    assert L.pbc_hip_diag_element_pp_set_offsets(None, 2) != 0 and b"null argument" in err()
    assert chk(off, 0) != 0 and b"m == 0" in err()
    H.clear()


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        return                                                   # (with a device the calls succeed: tests/test_gpu_eppset.py)
    v = golden("d_rand32.vec")
    H = pbc_amd.Pairing(_param("d159"))
    for group, recs in ((1, v.g1), (2, v.g2), (3, v.gt)):
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_pp_set_init(group, recs[:3])
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_pp_set_init_dev(group, 0x1000, 3)
        with pytest.raises(pbc_amd.PbcHipError, match="m == 0"):
            H.element_pp_set_init(group, recs[:0])
    with pytest.raises(pbc_amd.PbcHipError, match="group must be 1, 2 or 3"):
        H.element_pp_set_init(0, v.g1[:3])
    with pytest.raises(ValueError):
        H.element_pp_set_init(2, v.g1[:1])                       # G1 records where G2 records belong (40 / 120 bytes)
    H.clear()
