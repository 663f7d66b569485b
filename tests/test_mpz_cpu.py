"""CPU tests of element_mul_mpz / element_pow_mpz with one integer for the batch (include/pbc_hip.h
pbc_hip_element_mul_mpz_batch): the host recoding (mpz_plan.h) through pbc_hip_diag_mpz_digits; the lane bodies of the
kernels (group_mpz.cuh) compiled for the host next to the host mirror (tests/hostsim/hostsim_mpz.cpp) -- the fast lane
with its flags, the complete lane, the GT lanes -- on the batteries of tests/mpz_battery.py, whose expected records are
exact-integer results of tests/intref.py; the entry points and the Python wrappers as far as they go without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import intref
import member_battery as mb
import mpz_battery as zb
import pbc_amd
from conftest import ROOT, _param, golden

HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SETS = ["a", "a1", "d159", "e", "f", "g149", "a_160_256"]
WIDTHS = (1, 2, 4)                                               # what the library runs: bits on GT; the plain or the width-4 NAF on points
THIN_FULL_ROWS = ("0", "3", "r", "N", "2^64", "random mid", "512 bytes of ones")
OTHER_WIDTH_ROWS = ("3", "r", "N", "2^64", "long zero run", "random mid", "three leading zero bytes")
MORE_WIDTHS = (3, 5)                                             # the recoding is general; the contract is checked for these too


@pytest.fixture(scope="module")
def mpz_sim():
    """tests/hostsim/hostsim_mpz.cpp built as tests/hostsim/__init__.py builds hostsim.cpp"""
    lib = os.path.join(HOSTSIM, "libhostsim_mpz.so")
    csrc = os.path.join(ROOT, "pbc_amd", "csrc")
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim_mpz.cpp", "hostsim.cpp", "hostsim_shim.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if (not os.path.exists(lib)) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([CLANG, "-O1", "-Wno-psabi", "-std=c++17", "-fPIC", "-shared", "-I", HOSTSIM, "-o", lib,
                               os.path.join(HOSTSIM, "hostsim_mpz.cpp")])
    L = ctypes.CDLL(lib)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.hostsim_init.restype = vp
    L.hostsim_init.argtypes = [ctypes.c_char_p, sz]
    L.hostsim_mpz_points.argtypes = [vp, ci, ci, ci, vp, vp, vp, sz, ctypes.c_char_p, sz]
    L.hostsim_mpz_gt.argtypes = [vp, ci, vp, vp, vp, sz, ctypes.c_char_p, sz]
    L.hostsim_mpz_digits.restype = sz
    L.hostsim_mpz_digits.argtypes = [ctypes.c_char_p, sz, ci, vp, sz]
    handles = {}

    def run(name, group, mode, recs, kb, w=0):
        """-> result records (0xEE where a lane wrote nothing), flags of the fast lane.  group 3: GT.  w: 0 = the digit
        width the library takes for this k (left in run.width), 2 / 4 = that width"""
        if name not in handles:
            text = _param(name).encode()
            handles[name] = L.hostsim_init(text, len(text))
            assert handles[name]
        recs = np.ascontiguousarray(recs, np.uint8)
        out, flags = np.full(recs.shape, 0xEE, np.uint8), np.full(len(recs), 0xEE, np.uint8)
        if group == 3:
            assert L.hostsim_mpz_gt(handles[name], mode, out.ctypes.data, flags.ctypes.data, recs.ctypes.data, len(recs), kb, len(kb)) == 0
        else:
            run.width = L.hostsim_mpz_points(handles[name], group, mode, w, out.ctypes.data, flags.ctypes.data, recs.ctypes.data, len(recs), kb, len(kb))
            assert run.width in (2, 4) and w in (0, run.width)
        return out, flags
    run.lib = L
    return run


# ---- the digits ---------------------------------------------------------------------------------------------------------------
def _check_digits(d, k, klen, w):
    d = [int(x) for x in d]
    assert sum(x << i for i, x in enumerate(d)) == k
    assert len(d) <= 8 * klen + 1
    if k == 0:
        assert d == []
        return
    assert d[-1] > 0                                             # no padding above the top digit, and it is positive
    if w == 1:
        assert set(d) <= {0, 1}
        return
    assert all(x == 0 or (x % 2 == 1 and abs(x) < (1 << (w - 1))) for x in d)
    nz = [i for i, x in enumerate(d) if x]
    assert all(b - a >= w for a, b in zip(nz, nz[1:]))           # a non-zero digit is followed by at least w - 1 zeros


@pytest.mark.parametrize("name", SETS + ["a_160_1024"])
def test_digits_of_the_battery_scalars(mpz_sim, name):
    """sum d_i 2^i == k; digits zero or odd, |d| < 2^(w-1); no two non-zero digits within w positions; at most 8 klen + 1
    digits; k = 0: the empty string -- for every battery scalar and every width, through the library's diagnostic entry
    point and through the header the host mirror compiles, which agree"""
    L = mpz_sim.lib
    for group in (1, 2):
        for lab, k, kb in zb.scalars(name, group):
            for w in WIDTHS + MORE_WIDTHS:
                d = pbc_amd.Pairing.mpz_digits(k, w)
                _check_digits(d, k, len(kb), w)
                buf = np.zeros(8 * len(kb) + 2, np.int8)
                n = L.hostsim_mpz_digits(kb, len(kb), w, buf.ctypes.data, buf.size)      # the row's own bytes: leading zeros included
                assert np.array_equal(buf[:n], d), (lab, w)
                raw = np.zeros(8 * len(kb) + 2, np.int8)
                n2 = pbc_amd.lib().pbc_hip_diag_mpz_digits(kb, len(kb), w, ctypes.c_void_p(raw.ctypes.data), raw.size)
                assert n2 == n and np.array_equal(raw[:n], d), (lab, w)
            own = pbc_amd.Pairing.mpz_digits(k, 0)               # the library's own choice for points: one of its two widths
            assert any(np.array_equal(own, pbc_amd.Pairing.mpz_digits(k, w)) for w in (2, 4)), lab


def test_digits_edge_cases():
    D = pbc_amd.Pairing.mpz_digits
    assert D(0, 2).size == 0 and D(0, 1).size == 0
    assert list(D(1, 2)) == [1] and list(D(3, 2)) == [-1, 0, 1] and list(D(7, 2)) == [-1, 0, 0, 1]
    assert list(D(7, 4)) == [7] and list(D(9, 4)) == [-7, 0, 0, 0, 1] and list(D(5, 1)) == [1, 0, 1]
    assert list(D((1 << 70) + 3, 2)) == [-1, 0, 1] + [0] * 67 + [1]
    ones = (1 << 4096) - 1
    d = D(ones, 2)
    assert d.size == 4097 and d[0] == -1 and d[-1] == 1 and not d[1:-1].any()
    L = pbc_amd.lib()
    buf = np.zeros(8, np.int8)
    assert L.pbc_hip_diag_mpz_digits(b"\x00\x00\x00", 3, 2, ctypes.c_void_p(buf.ctypes.data), 8) == 0      # zero bytes only: k = 0
    assert L.pbc_hip_diag_mpz_digits(None, 0, 2, ctypes.c_void_p(buf.ctypes.data), 8) == 0
    assert L.pbc_hip_diag_mpz_digits(b"\x05", 1, 2, None, 0) == 3                                          # the count alone
    assert L.pbc_hip_diag_mpz_digits(b"\x0b", 1, 2, ctypes.c_void_p(buf.ctypes.data), 2) == 5 and list(buf[:3]) == [-1, 0, 0]   # cap
    rng = np.random.default_rng(5)
    for _ in range(200):
        nb = int(rng.integers(1, 40))
        kb = rng.bytes(nb)
        for w in WIDTHS + MORE_WIDTHS:
            _check_digits(D(int.from_bytes(kb, "big"), w), int.from_bytes(kb, "big"), nb, w)


# ---- the point lanes ---------------------------------------------------------------------------------------------------------
def _bad(got, want, labels, rows):
    return [(labels[r], got[i].tobytes().hex()[:16], want[i].tobytes().hex()[:16]) for i, r in enumerate(rows) if not np.array_equal(got[i], want[i])]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", SETS)
def test_point_lanes_on_host(mpz_sim, name, group):
    """the library's route and the complete lane alone equal intref for every unit x scalar, the complete lane raising no
    flag; the fast lane's result is already right wherever it raised no flag, and it wrote nothing where it did; it flags
    a unit of small order wherever the curve order is even, every subgroup point at k = r, and no subgroup point at the
    random k with 2^16 < k < r - 2^16.  For OTHER_WIDTH_ROWS the same with the digit width the library did not choose.
    Thinned where the mirror is slow -- the 33-word sets (a1, e: ~40 ms per unit and 1000-bit scalar) and the twists of
    types d and g (F_q^3, F_q^5): there THIN_FULL_ROWS run as everywhere, every other scalar runs the library's route (both
    lanes' code) on the four units of mpz_battery.long_rows (a subgroup point, a whole-curve point, an off-curve record, a
    small order), and the other digit width on "r" and "random mid"."""
    recs, labels, _ = zb.point_units(name, group)                # (G2 of the symmetric types: G1's curve, G1's battery)
    want = zb.point_expected(name, group)
    sub = zb.subgroup_rows(name, group)
    assert len(sub) >= 2
    flagged_small, widths = False, set()
    thin = name in zb.WIDE or (group == 2 and intref.fam(name).type in ("d", "g"))
    few = zb.long_rows(name, group)
    for lab, k, kb in zb.scalars(name, group):
        rows, exp = want[lab]
        full = not thin or lab in THIN_FULL_ROWS
        if not full:
            exp, rows = exp[[rows.index(r) for r in few]], few
        got, flags = mpz_sim(name, group, 0, recs[rows], kb)
        assert not _bad(got, exp, labels, rows), lab
        widths.add(mpz_sim.width)
        if lab in (OTHER_WIDTH_ROWS if not thin else ("r", "random mid")):       # the width the library did not take for this k: the same results
            other = 6 - mpz_sim.width
            got2, flags_o = mpz_sim(name, group, 0, recs[rows], kb, other)
            assert not _bad(got2, exp, labels, rows), (lab, other)
            fast_o, _ = mpz_sim(name, group, 2, recs[rows], kb, other)
            assert np.array_equal(fast_o[flags_o == 0], exp[flags_o == 0]) and (fast_o[flags_o == 1] == 0xEE).all(), (lab, other)
        if full:
            slow, none = mpz_sim(name, group, 1, recs[rows], kb)
            assert not _bad(slow, exp, labels, rows) and not none.any(), lab
            fast, flags2 = mpz_sim(name, group, 2, recs[rows], kb)
            assert np.array_equal(flags, flags2) and set(flags) <= {0, 1}
            keep = flags == 0
            assert np.array_equal(fast[keep], exp[keep]), lab
            assert (fast[~keep] == 0xEE).all(), lab              # a flagged lane leaves its record alone (out == in is allowed)
        pos = {r: i for i, r in enumerate(rows)}
        if lab == "r":
            assert all(flags[pos[r]] == 1 and not exp[pos[r]].any() for r in sub if r in pos)
        if lab == "random mid":
            assert not any(flags[pos[r]] for r in sub if r in pos)
            f = mb.flagged_unit(name, zb.curve_group(name, group))       # the unit the GPU slices place first, last and alone
            if f is not None:
                frec = mb.point_battery(name, zb.curve_group(name, group))[0][f:f + 1]
                assert mpz_sim(name, group, 2, frec, kb)[1][0] == 1
        if lab in ("0",):
            assert not exp.any()
        flagged_small |= any(flags[pos[r]] for r in rows if labels[r].startswith("order ") and k > 3)
    assert widths == {2, 4}                                      # dense scalars take the table, sparse ones do not
    if mb.curve_order(name, zb.curve_group(name, group)) % 2 == 0:
        assert any(l.startswith("order ") for l in labels)
        assert flagged_small
    if intref.fam(name).type in ("a", "a1", "e"):
        assert mb.curve_order(name, 1) % 2 == 0


def test_results_equal_the_zr_record_route_on_host(mpz_sim):
    """whenever k fits a Z_r record the bytes are those of element_mul_zn with that record: the host mirror's
    element_mul_zn lanes (tests/hostsim) on the same points"""
    import hostsim
    for name in ("a", "d159", "f"):
        S = intref.fam(name)
        H = hostsim.HostSim(_param(name))
        recs, labels, _ = zb.point_units(name, 1)
        for lab, k, kb in zb.scalars(name, 1):
            if k >= 1 << (8 * S.zl):
                continue
            z = np.tile(np.frombuffer(int(k).to_bytes(S.zl, "big"), np.uint8), (len(recs), 1))
            ref = H.group(0, recs, z)
            got, _ = mpz_sim(name, 1, 0, recs, kb)
            assert np.array_equal(got, ref), (name, lab)


# ---- GT -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_gt_lanes_on_host(mpz_sim, name):
    """every record x scalar against the exact power: x^0 = 1 (0^0 too), 0^k = 0, members, non-members; the generic lane
    alone; on the 512-bit type a field the Lucas lane serves exactly the elements of norm 1 -- -1 and x^(q - 1), which
    are no members of the order-r subgroup, among them -- and writes nothing else; on f.param the cyclotomic lane serves
    the cyclotomic subgroup, an element of another order and a k > r included, where the exponent is dense"""
    recs, labels = zb.gt_units(name)
    want = zb.gt_expected(name)
    K, decode, nco = mb.gt_field(name)
    zero, one = labels.index("0"), labels.index("1")
    routed = False
    for lab, k, kb in zb.scalars(name, 3):
        rows, exp = want[lab]
        got, flags = mpz_sim(name, 3, 0, recs[rows], kb)
        assert not _bad(got, exp, labels, rows), lab
        slow, none = mpz_sim(name, 3, 1, recs[rows], kb)
        assert not _bad(slow, exp, labels, rows) and not none.any(), lab
        if zero in rows:
            i = rows.index(zero)
            assert np.array_equal(got[i], recs[one] if k == 0 else recs[zero]), lab      # 0^0 = 1, 0^k = 0
        if name == "a":
            fast, flags2 = mpz_sim(name, 3, 2, recs[rows], kb)
            assert np.array_equal(flags, flags2)
            norm1 = np.array([labels[r] in ("pairing value", "1", "coordinates >= q", "1 as 1 + q", "-1", "norm 1, outside") for r in rows])
            assert np.array_equal(flags == 0, norm1), lab
            assert np.array_equal(fast[norm1], exp[norm1]) and (fast[~norm1] == 0xEE).all(), lab
        elif name == "f":                                        # the cyclotomic lane of element_pow_zn serves dense k that fit a Z_r record
            cyc = np.array([labels[r] in ("pairing value", "1", "coordinates >= q", "1 as 1 + q", "cyclotomic, outside") for r in rows])
            assert not flags[cyc].any() and (not flags.any() or flags[~cyc].all()), lab
            routed |= bool(flags.any())
        else:
            assert not flags.any()
    assert routed == (name == "f")
    if name == "f":                                              # a k >= r that fits the record, on a cyclotomic element of another order
        k = dict((lab, k) for lab, k, _ in zb.scalars(name, 3))["random 8 zl bits"]
        assert k > intref.fam(name).r and "cyclotomic, outside" in labels


@pytest.mark.parametrize("name", ["d159", "f"])
def test_gt_unit_group_order_on_host(mpz_sim, name):
    """x^N' = 1 for every x != 0 and 0^N' = 0, N' = q^k - 1 the order of the field's unit group: an exponent of 954 / 1899
    bits on elements outside every subgroup the pairing kernels' shortcuts assume"""
    recs, labels = zb.gt_units(name)
    Np = zb.gt_unit_order(name)
    kb = Np.to_bytes((Np.bit_length() + 7) // 8, "big")
    assert len(kb) <= zb.MAX_BYTES
    got, _ = mpz_sim(name, 3, 0, recs, kb)
    one, zero = recs[labels.index("1")], recs[labels.index("0")]
    for i, lab in enumerate(labels):
        assert np.array_equal(got[i], zero if lab == "0" else one), lab
    r = labels.index("random element")
    assert np.array_equal(zb.gt_pow(name, recs[r:r + 1], Np)[0], one)        # ... and the exact integers say so too
    got1, _ = mpz_sim(name, 3, 0, recs, (Np + 1).to_bytes(len(kb), "big"))   # x^(N' + 1) = x, reduced
    assert np.array_equal(got1, zb.gt_pow(name, recs, 1))


# ---- the C-ABI and the Python wrappers -----------------------------------------------------------------------------------
def test_exports_and_header_agree():
    hdr = open(os.path.join(ROOT, "include", "pbc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(pbc_amd.LIB_PATH)
    for sym in ("pbc_hip_element_mul_mpz_batch", "pbc_hip_element_mul_mpz_batch_dev", "pbc_hip_diag_mpz_digits"):
        assert re.search(r"\b%s\s*\(" % sym, code) and sym in pbc_amd.EXPORTS and hasattr(L, sym), sym
    assert re.search(r"#define PBC_HIP_MPZ_MAX_BYTES\s+512\b", hdr) and pbc_amd.MPZ_MAX_BYTES == 512 == zb.MAX_BYTES
    block = hdr[hdr.index("One integer of any length"):hdr.index("#define PBC_HIP_MPZ_MAX_BYTES")]
    for ref in ("include/pbc_field.h:292", ":365", "curve.c:713", "ecc/pairing.c:215,266,274", "arith/field.c:117", "mpz_tstbit",
                "Negative integers are not part of", "NOT reduced mod r", "HOST memory"):
        assert ref in block, ref


def test_bad_arguments_are_rejected_without_a_device():
    """klen = 513, NULL k with klen > 0, group 0 or 4, null records: non-zero with a message, before a device is looked
    for; n == 0 returns 0; a negative Python int raises"""
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    L = pbc_amd.lib()
    out = np.full_like(v.g1, 0xEE)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    k = b"\x05"
    for group in (0, 4, -1):
        assert L.pbc_hip_element_mul_mpz_batch(H._h, group, ptr(out), ptr(v.g1), k, 1, v.n) != 0
        assert b"group" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_mul_mpz_batch_dev(H._h, group, 0x1000, 0x1000, k, 1, v.n, None) != 0
        assert b"group" in L.pbc_hip_last_error()
    big = b"\x01" * 513
    assert L.pbc_hip_element_mul_mpz_batch(H._h, 1, ptr(out), ptr(v.g1), big, 513, v.n) != 0
    assert b"PBC_HIP_MPZ_MAX_BYTES" in L.pbc_hip_last_error()
    assert L.pbc_hip_element_mul_mpz_batch_dev(H._h, 1, 0x1000, 0x1000, big, 513, v.n, None) != 0
    assert b"PBC_HIP_MPZ_MAX_BYTES" in L.pbc_hip_last_error()
    assert L.pbc_hip_element_mul_mpz_batch(H._h, 1, ptr(out), ptr(v.g1), None, 1, v.n) != 0
    assert b"null argument" in L.pbc_hip_last_error()
    assert L.pbc_hip_element_mul_mpz_batch_dev(H._h, 1, 0x1000, 0x1000, None, 1, v.n, None) != 0
    assert b"null argument" in L.pbc_hip_last_error()
    for args in ((None, ptr(v.g1)), (ptr(out), None)):
        assert L.pbc_hip_element_mul_mpz_batch(H._h, 1, args[0], args[1], k, 1, v.n) != 0
        assert b"null argument" in L.pbc_hip_last_error()
        assert L.pbc_hip_element_mul_mpz_batch_dev(H._h, 1, args[0], args[1], k, 1, v.n, None) != 0
        assert b"null argument" in L.pbc_hip_last_error()
    assert L.pbc_hip_element_mul_mpz_batch(None, 1, ptr(out), ptr(v.g1), k, 1, v.n) != 0
    assert b"null pairing" in L.pbc_hip_last_error()
    for group in (1, 2, 3):                                      # n == 0: nothing to do, with or without k, with or without a device
        assert L.pbc_hip_element_mul_mpz_batch(H._h, group, ptr(out), None, None, 0, 0) == 0
        assert L.pbc_hip_element_mul_mpz_batch(H._h, group, None, None, k, 1, 0) == 0
        assert L.pbc_hip_element_mul_mpz_batch_dev(H._h, group, None, None, None, 0, 0, None) == 0
    assert (out == 0xEE).all()
    with pytest.raises(ValueError, match="non-negative"):
        H.element_mul_mpz(1, v.g1, -1)
    with pytest.raises(ValueError, match="non-negative"):
        H.element_mul_mpz_dev(1, 0x1000, 0x1000, -5, 4)
    with pytest.raises(ValueError, match="non-negative"):
        pbc_amd.Pairing.mpz_digits(-1, 2)
    with pytest.raises(pbc_amd.PbcHipError, match="group"):
        H.element_mul_mpz(0, v.g1, 5)
    with pytest.raises(ValueError):
        H.element_mul_mpz(2, v.g1, 5)                            # G1 records where G2 records belong (40 / 120 bytes)
    with pytest.raises(pbc_amd.PbcHipError, match="PBC_HIP_MPZ_MAX_BYTES"):
        H.element_mul_mpz(1, v.g1, 1 << 4096)                    # 513 bytes
    H.clear()


def test_python_wrappers_reach_the_c_entry_points_without_a_device():
    """as test_abi.py test_python_wrappers_reach_the_c_abi_and_fail_loudly_without_a_device"""
    if pbc_amd.lib().pbc_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    H = pbc_amd.Pairing(_param("d159"))
    v = golden("d_rand32.vec")
    for group, recs in ((1, v.g1), (2, v.g2), (3, v.gt)):
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_mul_mpz(group, recs, 12345)
        with pytest.raises(pbc_amd.PbcHipError, match="no HIP device"):
            H.element_mul_mpz_dev(group, 0x1000, 0x1000, 12345, 4, stream=0)
    H.clear()
