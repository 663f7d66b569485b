"""Batteries of the fixed-base table sets (include/pbc_hip.h pbc_hip_element_pp_set_*), shared by tests/test_eppset_cpu.py
(host mirror) and tests/test_gpu_eppset.py (the library).  Every expected record is computed with the exact integers of
tests/intref.py -- Curve.mul_batch(reduce=False) and Curve.add on points, the fields' pow / mul on GT -- never with the code
under test.

A battery is a KIND of base set for one (parameter set, group) and scalar rows of m scalars each:
  "distinct"  five different fixture points (GT: pairing values and a random field element)
  "related"   B_1 = B_0 (a repeated base), B_2 = -B_0 (an opposite pair), another fixture point, a record with
              coordinates >= q -- no table of it is "complete only", so the fast lane runs and has to report the rows
              that cancel or meet
  "crafted"   a fixture point, O, an off-curve record, a point of small order where the curve has one, a fixture point:
              some table is "complete only"
  "complete"  O, the off-curve record, the point of small order: every table is "complete only"
A set of m < 5 bases is the first m of its kind, and its rows are the first m scalars of the kind's rows, so the
per-base multiples are computed once.  exceptional() walks the fast lane's additions on exact points: the table entries
[w 2^(8 row)] B in the lane's order (base-major, row-minor), and says whether a step meets equal or opposite operands.

Sizing: intref's affine law costs a modular inversion per group operation; the wide sets (a1, e) and the twists keep the
thinned rows (_thin)."""
import functools

import numpy as np

import intref
import member_battery as mb
import mpz_battery as zb

KINDS = ("distinct", "related", "crafted", "complete")
M_MAX = 5
WIDE = zb.WIDE


def curve_group(name, group):
    return zb.curve_group(name, group)


def _curve(name, group):
    S = intref.fam(name)
    return (S.g1, S.lay1) if curve_group(name, group) == 1 else (S.g2, S.lay2)


def small_order_point(name, group):
    """a finite point of order 3, 4, 6 or 2 other than (0, 0), or None (f, g149 G1: prime order)"""
    C, _ = _curve(name, group)
    for order in (3, 4, 6, 2):
        T = mb._torsion(name, curve_group(name, group), order)
        if T is not None and T != (C.F.zero, C.F.zero):
            return order, T
    return None


@functools.lru_cache(maxsize=None)
def base_set(name, group, kind):
    """-> records (m, L) uint8, labels, decoded points (None: O) -- group 3: records, labels, field elements"""
    S = intref.fam(name)
    if group == 3:
        recs, labels = zb.gt_units(name)
        K, decode, nco = mb.gt_field(name)
        pv = [i for i, lab in enumerate(labels) if lab == "pairing value"]
        vals = intref.battery_gt(name)[0]
        seen, pvr = set(), []
        for row in vals:                                          # the fixture's distinct pairing values
            if row.tobytes() not in seen:
                seen.add(row.tobytes())
                pvr.append(row)
        assert pv and len(pvr) >= 3
        by = lambda lab: recs[labels.index(lab)]
        if kind == "distinct":
            rows, labs = [pvr[0], pvr[1], pvr[2], by("random element"), pvr[3 % len(pvr)]], ["pairing value"] * 3 + ["random element", "pairing value"]
        elif kind == "related":
            rows, labs = [pvr[0], pvr[0], pvr[1], by("coordinates >= q"), by("1")], ["pairing value", "repeat of 0", "pairing value", "coordinates >= q", "1"]
        else:
            return None
        out = np.stack(rows).astype(np.uint8)
        return out, labs, [decode(r.tobytes()) for r in out]
    C, lay = _curve(name, group)
    F = C.F
    fix = lay.unpack(intref._fixture_points(name, curve_group(name, group)))
    assert len(set(fix[:5])) == 5
    off = lay.encode((fix[0][0], F.add(fix[0][1], F.embed(1))))
    nc = b"".join(int(intref.noncanonical(c, S.q, S.fb)).to_bytes(S.fb, "big") for v in fix[2] for c in F.coeffs(v))
    so = small_order_point(name, group)
    if kind == "distinct":
        units = [("fixture %d" % i, lay.encode(fix[i])) for i in range(5)]
    elif kind == "related":
        units = [("fixture 0", lay.encode(fix[0])), ("repeat of 0", lay.encode(fix[0])), ("negative of 0", lay.encode(C.neg(fix[0]))),
                 ("fixture 1", lay.encode(fix[1])), ("coordinates >= q", nc)]
    elif kind == "crafted":
        units = [("fixture 0", lay.encode(fix[0])), ("O", bytes(lay.length)), ("off curve", off)]
        units += [("order %d" % so[0], lay.encode(so[1]))] if so else [("fixture 3", lay.encode(fix[3]))]
        units += [("fixture 1", lay.encode(fix[1]))]
    elif kind == "complete":
        units = [("O", bytes(lay.length)), ("off curve", off)] + ([("order %d" % so[0], lay.encode(so[1]))] if so else [])
    else:
        raise ValueError(kind)
    recs = np.frombuffer(b"".join(raw for _, raw in units), np.uint8).reshape(len(units), lay.length).copy()
    return recs, [lab for lab, _ in units], lay.unpack(recs)


def _thin(name, group):
    S = intref.fam(name)
    return name in WIDE or (curve_group(name, group) == 2 and S.type in ("d", "g", "f")) or group == 3


@functools.lru_cache(maxsize=None)
def rows(name, group, kind):
    """-> [(label, (z_0, ..., z_{m-1}))], m = the bases of the kind; every z < 2^(8 zl)"""
    S = intref.fam(name)
    r, zl = S.r, S.zl
    m = len(base_set(name, group, kind)[0])
    thin = _thin(name, group)
    ff = (1 << (8 * zl)) - 1
    out = [("all zero", (0,) * m)]
    positions = sorted({0, 1, zl // 2, zl - 1}) if thin else range(zl)
    for n, pos in enumerate(positions):                           # a single non-zero byte, every row position
        z = [0] * m
        z[n % m] = (1, 255, 0x80, 0x5A, 2)[n % 5] << (8 * pos)
        out.append(("byte %d" % pos, tuple(z)))
    out.append(("r - 1", (r - 1,) * m))
    out.append(("r", (r,) * m))
    out.append(("all 0xFF", (ff,) * m))
    out.append(("r - 1, r, 0xFF, 1, 2", tuple((r - 1, r, ff, 1, 2)[j] for j in range(m))))
    rng = intref._rng(name, 300 + 10 * group + KINDS.index(kind))
    if kind == "related" and group != 3:
        k = int.from_bytes(rng.bytes(zl), "big") % (r // 4)
        pad = lambda *z: tuple(list(z) + [0] * (m - len(z)))
        # rows that cancel: [k] B + [k] B + [2 k] (-B) = O
        out += [("cancel 1", pad(1, 1, 2)), ("cancel 0x0103", pad(0x0103, 0x0103, 0x0206)), ("cancel random", pad(k, k, 2 * k)),
                ("cancel pair", pad(5, 0, 5))]
        # rows that meet mid-way: a partial sum equals the next table entry (513 + 255 = 3 * 256), or its negative
        # (513 - 1 = 2 * 256: the sum passes through O and goes on)
        out += [("meet at once", pad(1, 1)), ("meet row 1", pad(0x0100, 0x0100)), ("meet mid-way", pad(0x0201, 0x03FF)),
                ("meet the negative mid-way", pad(0x0201, 0, 0x0201, 7, 9))]
    for i in range(3 if thin else 8):
        out.append(("random %d" % i, tuple(int.from_bytes(rng.bytes(zl), "big") for _ in range(m))))
    if name == "a1":                                             # (the host mirror builds one table entry per non-zero scalar byte: sparse rows)
        sparse = lambda: sum(int(rng.integers(1, 256)) << (8 * int(p)) for p in rng.choice(zl, 8, replace=False))
        out = [row for row in out if row[0] in ("all zero", "byte 0", "byte %d" % (zl - 1))]
        out += [("sparse random %d" % i, tuple(sparse() for _ in range(m))) for i in range(2)]
        if kind == "related":
            out += [("cancel 1", (1, 1, 2, 0, 0)), ("meet at once", (1, 1, 0, 0, 0)), ("meet mid-way", (0x0201, 0x03FF, 0, 0, 0))]
    return out


def zr_bytes(name, group, kind, m):
    """-> (rows, m * zl) uint8: the first m scalars of every row, big-endian records of Z_r"""
    zl = intref.fam(name).zl
    R = rows(name, group, kind)
    raw = b"".join(int(z).to_bytes(zl, "big") for _, zs in R for z in zs[:m])
    return np.frombuffer(raw, np.uint8).reshape(len(R), m * zl).copy()


def _flat(K, x):
    return zb._flat(K, x)


@functools.lru_cache(maxsize=None)
def _multiples(name, group, kind):
    """[row][j] = [z_j] B_j (GT: B_j^z_j) for every row and base of the kind"""
    recs, _, pts = base_set(name, group, kind)
    R = rows(name, group, kind)
    m = len(pts)
    if group == 3:
        K, _, _ = mb.gt_field(name)
        memo = {}
        out = []
        for _, zs in R:
            line = []
            for j, z in enumerate(zs):
                key = (pts[j], z)
                if key not in memo:
                    memo[key] = K.pow(pts[j], z) if z else K.one
                line.append(memo[key])
            out.append(line)
        return out
    C, _ = _curve(name, group)
    units = [(z, pts[j]) for _, zs in R for j, z in enumerate(zs) if pts[j] is not None]
    it = iter(C.mul_batch(units, reduce=False))
    return [[next(it) if pts[j] is not None else None for j in range(m)] for _ in R]


@functools.lru_cache(maxsize=None)
def expected(name, group, kind, m):
    """-> (rows, L) uint8: sum_{j < m} [z_j] B_j folded left to right (GT: the product of the powers)"""
    mult = _multiples(name, group, kind)
    if group == 3:
        S = intref.fam(name)
        K, _, nco = mb.gt_field(name)
        out = []
        for line in mult:
            acc = K.one
            for x in line[:m]:
                acc = K.mul(acc, x)
            out.append(b"".join(int(c).to_bytes(S.fb, "big") for c in _flat(K, acc)))
        return np.frombuffer(b"".join(out), np.uint8).reshape(len(out), nco * S.fb).copy()
    C, lay = _curve(name, group)
    out = []
    for line in mult:
        acc = None
        for P in line[:m]:
            acc = C.add(acc, P)
        out.append(acc)
    return lay.pack(out)


def single(name, group, kind, j):
    """-> (rows, L) uint8: [z_j] B_j alone, what a segment of pow_zn on table j gives for the rows' j-th scalars"""
    mult = _multiples(name, group, kind)
    if group == 3:
        S = intref.fam(name)
        K, _, nco = mb.gt_field(name)
        raw = b"".join(b"".join(int(c).to_bytes(S.fb, "big") for c in _flat(K, line[j])) for line in mult)
        return np.frombuffer(raw, np.uint8).reshape(len(mult), nco * S.fb).copy()
    _, lay = _curve(name, group)
    return lay.pack([line[j] for line in mult])


# ---- the fast lane's walk on exact points -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(name, cgroup, P):
    """[row][w] = [w 2^(8 row)] P for w = 0 .. 255 (w = 0: None), zl rows: 255 batched additions over the rows"""
    S = intref.fam(name)
    C = S.g1 if cgroup == 1 else S.g2
    heads, Q = [], P
    for _ in range(S.zl):
        heads.append(Q)
        for _ in range(8):
            Q = C.dbl(Q)
    tab = [[None, h] for h in heads]
    for _ in range(254):
        for t, E in zip(tab, C.add_many([(t[-1], h) for t, h in zip(tab, heads)])):
            t.append(E)
    return tab


@functools.lru_cache(maxsize=None)
def exceptional(name, group, kind, m):
    """-> bool per row: the fast lane's additions over the first m bases, in its order, meet equal or opposite operands.
    (All bases finite and of large order: kinds "distinct" and "related".)  A row all of whose bytes are zero meets nothing."""
    S = intref.fam(name)
    C, _ = _curve(name, group)
    _, _, pts = base_set(name, group, kind)
    assert all(P is not None for P in pts[:m])
    out = []
    for _, zs in rows(name, group, kind):
        acc, hit = None, False
        for j in range(m):
            if hit:
                break
            P = pts[j]
            neg = P == C.neg(pts[0]) and j > 0                   # (the table of -B_0 is the negated table of B_0)
            tab = _table(name, curve_group(name, group), pts[0] if neg else P)
            zb_ = int(zs[j]).to_bytes(S.zl, "big")
            for row in range(S.zl):
                w = zb_[S.zl - 1 - row]
                if not w:
                    continue
                E = tab[row][w]
                assert E is not None
                if neg:
                    E = C.neg(E)
                if acc is None:
                    acc = E
                    continue
                if acc[0] == E[0]:
                    hit = True
                    break
                acc = C.add(acc, E)
        out.append(hit)
    return np.array(out, bool)


def tiled(recs, n):
    """n units: the battery's rows, repeated"""
    idx = np.arange(n) % len(recs)
    return recs[idx], idx
