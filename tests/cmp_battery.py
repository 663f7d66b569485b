"""Batteries of element_cmp and of GT inversion / division (include/pbc_hip.h pbc_hip_element_cmp_batch,
pbc_hip_element_invert_GT_batch), shared by tests/test_cmp_cpu.py, tests/test_gtdiv_cpu.py (host mirror) and
tests/test_gpu_gtdiv.py, tests/test_gpu_cmp.py (the library).  Every expected byte is computed with the exact integers of
tests/intref.py and the towers of tests/member_battery.py -- never with the code under test:
  plain groups: equality of the reduced values; for points, a record off the curve or all zero is O, O == O, O != finite;
  twists:       Curve.mul(quotient_cmp, a - b, reduce=False) is None, with the REFERENCE's quotient_cmp (the trace
                recurrence of pbc_mpz_curve_order_extn), not the shorter integer the kernels walk."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import intref
import member_battery as mb
from conftest import ROOT, _param

EQUAL, DIFFER = 0, 1
TWISTS = ("d159", "d201", "f", "g149")


def curve_order_extn(q, t, k):
    """#E(F_q^k) for a curve over F_q of trace t: t_0 = 2, t_1 = t, t_(j+1) = t t_j - q t_(j-1)"""
    tj, tprev = t, 2
    for _ in range(k - 1):
        tj, tprev = t * tj - q * tprev, tj
    return q ** k + 1 - tj


def quotient_cmp_of_text(text):
    """-> (the reference's quotient_cmp, the twist's order) for a type d / g / f parameter text, None for another type:
    #E'(F_q^d) / r (ecc/d_param.c:1060-1069, ecc/g_param.c:1336), #E(F_q^12) / r^2 (ecc/f_param.c:388-398)"""
    p = intref.param_dict(text)
    if p["type"] in ("d", "g"):
        q, r = p["q"], p["r"]
        N = curve_order_extn(q, -(q + 1 - p["n"]), p["k"] // 2)
        assert N % r == 0
        return N // r, N
    if p["type"] == "f":
        q, r = p["q"], p["r"]
        N = curve_order_extn(q, q - r + 1, 12)
        assert N % (r * r) == 0
        return N // (r * r), r * (2 * q - r)
    return None


def _is_twist(name, group):
    return group == 2 and intref.fam(name).type in ("d", "g", "f")


def _nc_point(S, F, P):
    return b"".join(int(intref.noncanonical(c, S.q, S.fb)).to_bytes(S.fb, "big") for v in P for c in F.coeffs(v))


@functools.lru_cache(maxsize=None)
def point_pairs(name, group):
    """-> [(label, a record, b record)] of one (parameter set, group)"""
    S = intref.fam(name)
    C, lay = (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)
    F = C.F
    fix = lay.unpack(intref._fixture_points(name, group))
    P, Q = fix[0], fix[1]
    enc = lay.encode
    O = bytes(lay.length)
    off = enc((P[0], F.add(P[1], F.embed(1))))
    pairs = [("P / P", enc(P), enc(P)), ("Q / Q", enc(Q), enc(Q)),
             ("P / P, coordinates >= q", enc(P), _nc_point(S, F, P)),
             ("P / Q", enc(P), enc(Q)), ("P / -P", enc(P), enc(C.neg(P))),
             ("O / O", O, O), ("O / off curve", O, off), ("off curve / off curve", off, enc((Q[0], F.add(Q[1], F.embed(1))))),
             ("P / O", enc(P), O), ("O / P", O, enc(P)), ("P / off curve", enc(P), off)]
    pairs.append(("zero record / zero as q", O, b"".join(int(S.q).to_bytes(S.fb, "big") for _ in range(2 * F.d))))
    if _is_twist(name, group):
        N, r = mb.curve_order(name, 2), S.r
        X = fix[2]
        rX, hX = C.mul(r, X, reduce=False), C.mul(N // r, X, reduce=False)
        assert rX is not None
        pairs += [("P / P + [r]X", enc(P), enc(C.add(P, rX))), ("P + [r]X / P", enc(C.add(P, rX)), enc(P)),
                  ("P / P + X", enc(P), enc(C.add(P, X))), ("O / [r]X", O, enc(rX)), ("[r]X / O", enc(rX), O),
                  ("[r]X / [r]Q", enc(rX), enc(C.mul(r, Q, reduce=False)))]
        if hX is not None:
            pairs.append(("P / P + [N/r]X", enc(P), enc(C.add(P, hX))))
        for order in (2, 3, 4, 6):
            T = mb._torsion(name, 2, order)
            if T is not None:
                pairs.append(("difference of order %d" % order, enc(C.add(P, T)), enc(P)))
                pairs.append(("order %d / O" % order, enc(T), O))
    return pairs


@functools.lru_cache(maxsize=None)
def point_battery(name, group):
    """-> a records, b records, expected bytes, labels (G2 of the symmetric types is G1: one curve, one battery)"""
    S = intref.fam(name)
    if S.type in ("a", "a1", "e"):
        group = 1
    C, lay = (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)
    pairs = point_pairs(name, group)
    c = quotient_cmp_of_text(_param(name))[0] if _is_twist(name, group) else None
    half, zero = lay.length // 2, C.F.zero

    def read(raw):                                               # the header's reading: reduced mod q, then (0, 0) / off curve -> O
        P = (lay.elem(raw[:half]), lay.elem(raw[half:]))
        return None if P == (zero, zero) or not C.on_curve(P) else P
    ops = [(read(ra), read(rb)) for _, ra, rb in pairs]
    if c is None:
        want = [EQUAL if A == B else DIFFER for A, B in ops]
    else:
        diffs = [C.sub(A, B) for A, B in ops]
        finite = [i for i, D in enumerate(diffs) if D is not None]
        want = [EQUAL] * len(ops)
        for i, R in zip(finite, C.mul_batch([(c, diffs[i]) for i in finite], reduce=False)):
            want[i] = EQUAL if R is None else DIFFER
    pack = lambda k: np.frombuffer(b"".join(u[k] for u in pairs), np.uint8).reshape(len(pairs), lay.length).copy()
    return pack(1), pack(2), np.array(want, np.uint8), [u[0] for u in pairs]


def flagged_pair(name):
    """the index of a twist pair the fast lane cannot finish (a difference of order 2, 3 or 4: the table or the doubling
    chain meets an exceptional step whatever the digits are), or None where the twist has no such point"""
    labels = point_battery(name, 2)[3]
    for order in (3, 4, 2):
        if "difference of order %d" % order in labels:
            return labels.index("difference of order %d" % order)
    return None


@functools.lru_cache(maxsize=None)
def zr_battery(name):
    S = intref.fam(name)
    r, zl = S.r, S.zl
    rng = intref._rng(name, 57)
    x, y = intref._rand_below(rng, r), intref._rand_below(rng, r)
    rec = lambda v: int(v).to_bytes(zl, "big")
    pairs = [("x / x", rec(x), rec(x)), ("x / y", rec(x), rec(y)), ("x / -x", rec(x), rec(r - x)), ("0 / 0", rec(0), rec(0)),
             ("0 / 1", rec(0), rec(1)), ("x / x + 1", rec(x), rec((x + 1) % r))]
    if intref.noncanonical(x, r, zl) != x:
        pairs += [("x / x, >= r", rec(x), rec(intref.noncanonical(x, r, zl))), ("0 / r", rec(0), rec(intref.noncanonical(0, r, zl)))]
    want = [EQUAL if int.from_bytes(a, "big") % r == int.from_bytes(b, "big") % r else DIFFER for _, a, b in pairs]
    pack = lambda k: np.frombuffer(b"".join(u[k] for u in pairs), np.uint8).reshape(len(pairs), zl).copy()
    return pack(1), pack(2), np.array(want, np.uint8), [u[0] for u in pairs]


@functools.lru_cache(maxsize=None)
def gt_cmp_battery(name):
    """pairs over member_battery.gt_battery: every unit with itself, with its neighbour, and the two images of one element"""
    recs, _, labels = mb.gt_battery(name)
    K, decode, _ = mb.gt_field(name)
    n = len(recs)
    ia = list(range(n)) + list(range(n)) + [labels.index("pairing value"), labels.index("1")]
    ib = list(range(n)) + [(i + 1) % n for i in range(n)] + [labels.index("coordinates >= q"), labels.index("1 as 1 + q")]
    want = [EQUAL if decode(recs[i].tobytes()) == decode(recs[j].tobytes()) else DIFFER for i, j in zip(ia, ib)]
    return recs[ia].copy(), recs[ib].copy(), np.array(want, np.uint8), ["%s / %s" % (labels[i], labels[j]) for i, j in zip(ia, ib)]


def battery(name, group):
    return zr_battery(name) if group == 0 else gt_cmp_battery(name) if group == 3 else point_battery(name, group)


# ---- GT inversion / division ---------------------------------------------------------------------------------------------
GENERIC = ("2 x pairing value", "random element", "0")


def expect_generic(name, label):
    """does the lane run the inversion in the subfield for this unit of member_battery.gt_battery?  Elements of norm 1 down
    to the half-degree subfield -- pairing values, 1, their other byte images -- do not.  Type e has GT = F_q and no such
    subfield (no conjugation inverts a pairing value there): only 1 is served without fp_inv."""
    if intref.fam(name).type == "e":
        return label not in ("1", "1 as 1 + q")
    return label in GENERIC


def div_pairs(name):
    """index pairs (a, b) over the battery: every unit over its neighbour and over itself"""
    n = len(mb.gt_battery(name)[0])
    return list(range(n)) * 2, [(i + 1) % n for i in range(n)] + list(range(n))


# ---- the host mirror (tests/hostsim/hostsim_gtdiv.cpp), built as tests/test_member_cpu.py builds its own ---------------------
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@functools.lru_cache(maxsize=None)
def host_mirror():
    lib = os.path.join(HOSTSIM, "libhostsim_gtdiv.so")
    csrc = os.path.join(ROOT, "pbc_amd", "csrc")
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim_gtdiv.cpp", "hostsim.cpp", "hostsim_shim.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if (not os.path.exists(lib)) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call([CLANG, "-O1", "-Wno-psabi", "-std=c++17", "-fPIC", "-shared", "-I", HOSTSIM, "-o", lib,
                               os.path.join(HOSTSIM, "hostsim_gtdiv.cpp")])
    L = ctypes.CDLL(lib)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.hostsim_init.restype = vp
    L.hostsim_init.argtypes = [ctypes.c_char_p, sz]
    L.hostsim_gtdiv.argtypes = [vp, ci, vp, vp, vp, vp, sz]
    L.hostsim_cmp.argtypes = [vp, ci, ci, vp, vp, vp, vp, sz, ctypes.c_char_p, sz]
    return L


class Mirror:
    """one parameter set on the host mirror"""

    def __init__(self, name):
        self.L, self.text = host_mirror(), _param(name).encode()
        self.h = self.L.hostsim_init(self.text, len(self.text))
        assert self.h

    def gtdiv(self, a, b=None, generic=False):
        """-> out records, lanes (1: the lane ran the subfield inversion)"""
        a = np.ascontiguousarray(a, np.uint8)
        b = None if b is None else np.ascontiguousarray(b, np.uint8)
        out, lanes = np.full_like(a, 0xee), np.full(len(a), 0xee, np.uint8)
        assert self.L.hostsim_gtdiv(self.h, 1 if generic else 0, out.ctypes.data, lanes.ctypes.data, a.ctypes.data,
                                    None if b is None else b.ctypes.data, len(a)) == 0
        return out, lanes

    def cmp(self, group, mode, a, b):
        """-> verdict bytes, flags of the fast lane"""
        a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        res, flags = np.full(len(a), 0xee, np.uint8), np.full(len(a), 0xee, np.uint8)
        assert self.L.hostsim_cmp(self.h, group, mode, res.ctypes.data, flags.ctypes.data, a.ctypes.data, b.ctypes.data, len(a),
                                  self.text, len(self.text)) == 0
        return res, flags


@functools.lru_cache(maxsize=None)
def mirror(name):
    return Mirror(name)
