"""Batteries of the membership verdicts (include/pbc_hip.h pbc_hip_element_membership_batch), shared by
tests/test_member_cpu.py (host mirror) and tests/test_gpu_member.py (the library).  Every expected class is computed
with the exact integers of tests/intref.py -- never with the code under test:
  points: all reduced coordinates zero -> IDENTITY (the header's reading of a record); off the curve -> INVALID;
          otherwise Curve.mul(r, P, reduce=False) is None -> INSIDE, else OUTSIDE;
  GT:     0 -> INVALID, 1 -> IDENTITY, x^r == 1 -> INSIDE, else OUTSIDE (x^r in intref's fields and a binomial tower on them)."""
import functools

import numpy as np

import intref
from conftest import _param

INVALID, OUTSIDE, INSIDE, IDENTITY = 0, 1, 2, 3


# ---- the group orders the constructions below need -----------------------------------------------------------------------
def _params(name):
    return intref.param_dict(_param(name))


def curve_order(name, group):
    """#E(F_q) for G1 (and the symmetric G2), the order of the twist for G2 of types d, f, g"""
    S, p = intref.fam(name), _params(name)
    q = S.q
    if S.type in ("a", "a1"):
        return q + 1                                             # supersingular: trace 0
    if S.type == "e":
        assert p["h"] * S.r * S.r + 1 == q                       # ecc/e_param.c:20, :967-969: q = h r^2 + 1, #E = h r^2
        return q - 1
    if S.type in ("d", "g"):
        n = p["n"]
        if group == 1:
            return n
        d, t = p["k"] // 2, q + 1 - n
        tj, tprev = t, 2                                         # t_{j+1} = t t_j - q t_{j-1}
        for _ in range(d - 1):
            tj, tprev = t * tj - q * tprev, tj
        return q ** d + 1 + tj                                   # the twist: trace -t_d
    assert S.type == "f"
    return S.r if group == 1 else S.r * (2 * q - S.r)            # tests/golden/gen_bn_param.py


def _curve(name, group):
    S = intref.fam(name)
    return (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)


@functools.lru_cache(maxsize=None)
def _sylow_chains(name, group):
    """{2: [Q, 2 Q, 4 Q, ...], 3: [Q, 3 Q, ...]}: for l = 2, 3 the non-O multiples of Q = [N / l^s] P (l^s the full power of l
    in the curve order N), for the first crafted P whose Q is not O: the last entry has order l, the one before it l^2"""
    N = curve_order(name, group)
    C, _ = _curve(name, group)
    cands = [P for _, P in intref.crafted_points(name, group)][:12]
    out = {}
    for l in (2, 3):
        m = N
        while m % l == 0:
            m //= l
        if m == N:
            continue
        for Q in C.mul_batch([(m, P) for P in cands], reduce=False):
            if Q is None:
                continue
            chain = []
            while Q is not None:
                chain.append(Q)
                Q = C.mul(l, Q, reduce=False)
            out[l] = chain
            break
    return out


def _torsion(name, group, order):
    """a point of exact order `order` (2, 3, 4 or 6) from the chains above, or None where the curve has none"""
    C, _ = _curve(name, group)
    ch = _sylow_chains(name, group)
    T2 = ch[2][-1] if 2 in ch else None
    T4 = ch[2][-2] if 2 in ch and len(ch[2]) > 1 else None
    T3 = ch[3][-1] if 3 in ch else None
    T = {2: T2, 3: T3, 4: T4, 6: C.add(T2, T3) if T2 is not None and T3 is not None else None}[order]
    if T is not None:
        assert C.mul(order, T, reduce=False) is None
        assert all(C.mul(order // f, T, reduce=False) is not None for f in (2, 3) if order % f == 0)
    return T


@functools.lru_cache(maxsize=None)
def point_units(name, group):
    """-> [(label, record bytes)]: the battery of one (parameter set, group)"""
    S = intref.fam(name)
    C, lay = _curve(name, group)
    F = C.F
    fix = lay.unpack(intref._fixture_points(name, group))
    twist = group == 2 and S.type in ("d", "g", "f")
    units = [("crafted " + lab, lay.encode(P)) for lab, P in intref.crafted_points(name, group)]
    if twist:
        N = curve_order(name, group)
        assert N % S.r == 0
        sub = C.mul_batch([(N // S.r, P) for P in fix[:4]], reduce=False)     # INSIDE on the twist
        assert all(P is not None for P in sub)
        units += [("fixture", lay.encode(P)) for P in fix[:4]]                # (whole-twist points as the reference draws them)
        fix = sub
    units += [("subgroup", lay.encode(P)) for P in fix]
    units += [("neg subgroup", lay.encode(C.neg(P))) for P in fix[:2]]
    units.append(("O", bytes(lay.length)))
    P = fix[0]
    one = F.embed(1)
    units.append(("off curve", lay.encode((P[0], F.add(P[1], one)))))
    nc = b"".join(int(intref.noncanonical(c, S.q, S.fb)).to_bytes(S.fb, "big") for v in fix[1 % len(fix)] for c in F.coeffs(v))
    units.append(("coordinates >= q", nc))
    units.append(("zero as q", b"".join(int(S.q).to_bytes(S.fb, "big") for _ in range(2 * F.d))))
    for order in (2, 3, 4, 6):
        T = _torsion(name, group, order)
        if T is None:
            continue
        units.append(("order %d" % order, lay.encode(T)))
        if order == 2:                                           # [r] (P + T) = T != O: catches an x-only or Z-only end test
            units += [("subgroup + 2-torsion", lay.encode(C.add(Q, T))) for Q in fix[:2]]
    if S.type in ("a", "a1"):
        units += [("subgroup + (0, 0)", lay.encode(C.add(Q, (0, 0)))) for Q in fix[2:4]]
    return units


def point_battery(name, group):
    """-> records (n, L) uint8, expected classes (n,) uint8, labels (G2 of the symmetric types is G1: one curve, one battery)"""
    return _point_battery(name, 1 if intref.fam(name).type in ("a", "a1", "e") else group)


@functools.lru_cache(maxsize=None)
def _point_battery(name, group):
    S = intref.fam(name)
    C, lay = _curve(name, group)
    units = point_units(name, group)
    half = lay.length // 2
    want, todo = [None] * len(units), []
    for i, (_, raw) in enumerate(units):
        x, y = lay.elem(raw[:half]), lay.elem(raw[half:])
        if x == C.F.zero and y == C.F.zero:
            want[i] = IDENTITY
        elif not C.on_curve((x, y)):
            want[i] = INVALID
        else:
            todo.append((i, (x, y)))
    for (i, _), R in zip(todo, C.mul_batch([(S.r, P) for _, P in todo], reduce=False)):
        want[i] = INSIDE if R is None else OUTSIDE
    recs = np.frombuffer(b"".join(raw for _, raw in units), np.uint8).reshape(len(units), lay.length).copy()
    return recs, np.array(want, np.uint8), [lab for lab, _ in units]


def flagged_unit(name, group):
    """the index of a unit the fast lane cannot finish -- a finite point of order 3, 4, 6 or 2 (in that order of
    preference; on types a / a1 the point of order 2 is (0, 0), the zero record: O, never flagged) whose class is OUTSIDE
    -- or None where the curve has no such point (f, g149 G1: prime order).  tests/test_member_cpu.py asserts that the
    host mirror's fast lane raises its flag for exactly this unit; tests/test_gpu_member.py places it first, last and alone"""
    _, want, labels = point_battery(name, group)
    for lab in ("order 3", "order 4", "order 6", "order 2"):
        if lab in labels and want[labels.index(lab)] == OUTSIDE:
            return labels.index(lab)
    return None


# ---- GT -------------------------------------------------------------------------------------------------------------------
class Tower:
    """base[X] / (X^d - c) over one of intref's fields; elements are tuples of d base elements, coefficient 0 first"""

    def __init__(self, base, d, c):
        self.B, self.d, self.c = base, d, c
        self.zero = (base.zero,) * d
        self.one = (base.one,) + (base.zero,) * (d - 1)

    def mul(self, a, b):
        B, d = self.B, self.d
        p = [B.zero] * (2 * d - 1)
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                p[i + j] = B.add(p[i + j], B.mul(x, y))
        for k in range(2 * d - 2, d - 1, -1):
            p[k - d] = B.add(p[k - d], B.mul(p[k], self.c))
        return tuple(p[:d])

    def pow(self, a, e):
        r = self.one
        for bit in bin(e)[2:]:
            r = self.mul(r, r)
            if bit == "1":
                r = self.mul(r, a)
        return r


def gt_field(name):
    """-> (field with .zero / .one / .pow, decode(record bytes) -> element, F_q coefficients per record)"""
    S, p = intref.fam(name), _params(name)
    q, fb = S.q, S.fb
    ints = lambda raw: [int.from_bytes(raw[i:i + fb], "big") % q for i in range(0, len(raw), fb)]
    if S.type == "e":
        return S.fq, (lambda raw: ints(raw)[0]), 1
    if S.type in ("a", "a1"):
        E = intref.Ext(q, [1, 0])                                # F_q[i], i^2 = -1: re then im
        return E, (lambda raw: E.from_coeffs(ints(raw))), 2
    if S.type in ("d", "g"):
        d = p["k"] // 2
        E = intref.Ext(q, [p["coeff%d" % i] for i in range(d)])
        T = Tower(E, 2, E.embed(p["nqr"]))                       # F_q^d[sqrt(nqr)]: x then y
        return T, (lambda raw: tuple(E.from_coeffs(ints(raw)[j * d:(j + 1) * d]) for j in range(2))), 2 * d
    E = intref.Ext(q, [-p["beta"], 0])                           # type f: F_q^2[X] / (X^6 + alpha)
    T = Tower(E, 6, E.neg(E.from_coeffs([p["alpha0"], p["alpha1"]])))
    return T, (lambda raw: tuple(E.from_coeffs(ints(raw)[2 * j:2 * j + 2]) for j in range(6))), 12


@functools.lru_cache(maxsize=None)
def gt_battery(name):
    """-> records, expected classes, labels: the fixture's pairing values (battery_gt's elements), 1, 0, a pairing value
    times the F_q scalar 2, random field elements (no final power: outside; on type f also outside the cyclotomic
    subgroup), a coordinate >= q"""
    S = intref.fam(name)
    K, decode, nco = gt_field(name)
    fb, q = S.fb, S.q
    vals = intref.battery_gt(name)[0]
    seen, units = set(), []
    for row in vals:
        raw = row.tobytes()
        if raw not in seen:
            seen.add(raw)
            units.append(("pairing value", raw))
    enc = lambda cs: b"".join(int(c).to_bytes(fb, "big") for c in cs)
    first = [int.from_bytes(units[0][1][i:i + fb], "big") for i in range(0, nco * fb, fb)]
    units.append(("1", enc([1] + [0] * (nco - 1))))
    units.append(("0", bytes(nco * fb)))
    units.append(("2 x pairing value", enc([2 * c % q for c in first])))
    rng = intref._rng(name, 41)
    for _ in range(3):
        units.append(("random element", enc([intref._rand_below(rng, q) for _ in range(nco)])))
    units.append(("coordinates >= q", enc([intref.noncanonical(c, q, fb) for c in first])))
    units.append(("1 as 1 + q", enc([intref.noncanonical(1, q, fb)] + [0] * (nco - 1))))
    want = []
    for _, raw in units:
        x = decode(raw)
        want.append(INVALID if x == K.zero else IDENTITY if x == K.one else INSIDE if K.pow(x, S.r) == K.one else OUTSIDE)
    recs = np.frombuffer(b"".join(raw for _, raw in units), np.uint8).reshape(len(units), nco * fb).copy()
    return recs, np.array(want, np.uint8), [lab for lab, _ in units]
