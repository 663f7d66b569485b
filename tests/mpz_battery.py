"""Batteries of element_mul_mpz / element_pow_mpz (include/pbc_hip.h pbc_hip_element_mul_mpz_batch), shared by
tests/test_mpz_cpu.py (host mirror) and tests/test_gpu_mpz.py (the library).  Every expected record is computed with the
exact integers of tests/intref.py -- Curve.mul_batch(reduce=False) on points, the fields' pow on GT -- never with the
code under test.  Scalars travel as the big-endian BYTES the C-ABI takes, so that leading zero bytes are part of a row.

Sizing.  intref's affine law costs a modular inversion per group operation, a tower product in Python tens of
microseconds, every (unit, scalar) pair is one exact computation, and the host mirror of tests/test_mpz_cpu.py walks every
pair three times on code built for stepping, not for speed: the point battery keeps two units of every label of
member_battery.point_units (three of the crafted whole-curve points); on the twists and the 33-word sets one of every
label and two subgroup points (33-word sets: without the two re-encodings of zero and of a coordinate, which the
narrower sets keep; at most 16); the GT battery one record of every label; the 512-byte scalar runs on 4 points / 2 GT
records of a set."""
import functools

import numpy as np

import intref
import member_battery as mb

WIDE = ("a1", "e", "a_160_1024")                                 # 33-word fields
MAX_BYTES = 512


def curve_group(name, group):
    """G2 of the symmetric types is G1: one curve, one battery"""
    return 1 if group == 2 and intref.fam(name).type in ("a", "a1", "e") else group


def _kb(k, lead=0):
    return bytes(lead) + int(k).to_bytes((int(k).bit_length() + 7) // 8, "big")


@functools.lru_cache(maxsize=None)
def scalars(name, group):
    """-> [(label, k, bytes)], the last row the 512-byte all-ones value.  N: the order of the curve (group 3: of G1's)"""
    S = intref.fam(name)
    r, zl = S.r, S.zl
    group = curve_group(name, group)
    N = mb.curve_order(name, 1 if group == 3 else group)
    rows = [(str(k), k) for k in (0, 1, 2, 3)]
    rows += [("r - 1", r - 1), ("r", r), ("r + 1", r + 1), ("N - 1", N - 1), ("N", N), ("N + 1", N + 1)]
    for j in sorted({1, 7, 8, 31, 32, 33, 64, r.bit_length() - 1, r.bit_length()}):
        rows += [("2^%d" % j, 1 << j), ("2^%d - 1" % j, (1 << j) - 1)]
    rows.append(("long zero run", (1 << 70) + 3))                # NAF 1 0^67 1 0 -1: a run of 67 zeros, longer than any window
    rng = intref._rng(name, 90 + group)
    mid = (1 << 16) + 1 + intref._rand_below(rng, r - (1 << 17) - 1)
    assert (1 << 16) < mid < r - (1 << 16)
    rows.append(("random mid", mid))
    rows.append(("random 8 zl bits", (1 << (8 * zl - 1)) | intref._rand_below(rng, 1 << (8 * zl - 1))))
    rows.append(("random 8 zl + 1 bits", (1 << (8 * zl)) | intref._rand_below(rng, 1 << (8 * zl))))
    out = [(lab, k, _kb(k)) for lab, k in rows]
    out.append(("three leading zero bytes", 0x0123456789, _kb(0x0123456789, 3)))
    out.append(("512 bytes of ones", (1 << (8 * MAX_BYTES)) - 1, b"\xff" * MAX_BYTES))
    return out


@functools.lru_cache(maxsize=None)
def point_units(name, group):
    """-> records (n, L) uint8, labels, decoded points (None: O): member_battery.point_units, thinned as stated above"""
    S = intref.fam(name)
    group = curve_group(name, group)
    lay = S.lay1 if group == 1 else S.lay2
    twist = group == 2
    seen, keep = {}, []
    for lab, raw in mb.point_units(name, group):
        key = "crafted" if lab.startswith("crafted") else lab
        seen[key] = seen.get(key, 0) + 1
        most = 2 if key == "subgroup" else 1 if (twist or name in WIDE) else 3 if key == "crafted" else 2
        if seen[key] <= most:
            keep.append((lab, raw))
    if name in WIDE:
        keep = [u for u in keep if u[0] not in ("zero as q", "coordinates >= q", "fixture")][:16]
    recs = np.frombuffer(b"".join(raw for _, raw in keep), np.uint8).reshape(len(keep), lay.length).copy()
    return recs, [lab for lab, _ in keep], lay.unpack(recs)


def long_rows(name, group):
    """the units the 512-byte scalar runs on: a subgroup point, a whole-curve point, O or off-curve, a small order"""
    _, labels, _ = point_units(name, group)
    pick = []
    for want in ("subgroup", "crafted", "off curve", "order "):
        for i, lab in enumerate(labels):
            if lab.startswith(want) and i not in pick:
                pick.append(i)
                break
    return pick


@functools.lru_cache(maxsize=None)
def point_expected(name, group):
    """-> {scalar label: (rows, expected records)}: rows = the unit indices the scalar runs on"""
    S = intref.fam(name)
    group = curve_group(name, group)
    C, lay = (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)
    recs, labels, pts = point_units(name, group)
    rows_all = list(range(len(pts)))
    ks = scalars(name, group)
    short = [(lab, k) for lab, k, _ in ks[:-1]]
    res = C.mul_batch([(k, pts[i]) for _, k in short for i in rows_all if pts[i] is not None], reduce=False)
    out, it = {}, iter(res)
    for lab, k in short:
        out[lab] = (rows_all, lay.pack([next(it) if pts[i] is not None else None for i in rows_all]))
    lab, k, _ = ks[-1]
    rows = long_rows(name, group)
    res = iter(C.mul_batch([(k, pts[i]) for i in rows if pts[i] is not None], reduce=False))
    out[lab] = (rows, lay.pack([next(res) if pts[i] is not None else None for i in rows]))
    return out


def subgroup_rows(name, group):
    _, labels, _ = point_units(name, group)
    return [i for i, lab in enumerate(labels) if lab in ("subgroup", "neg subgroup")]


# ---- GT -------------------------------------------------------------------------------------------------------------------
def _flat(K, x):
    if isinstance(K, mb.Tower):
        return [c for v in x for c in _flat(K.B, v)]
    return list(K.coeffs(x))


@functools.lru_cache(maxsize=None)
def gt_units(name):
    """-> records, labels: one record of every label of member_battery.gt_battery, and what that battery lacks -- elements
    the subgroup shortcuts ACCEPT that are no members of the order-r subgroup: "-1" (norm 1, order 2); on types a / a1
    "norm 1, outside" = x^(q - 1) = conj(x) / x for a random x (norm 1, order dividing q + 1); on type f "cyclotomic,
    outside" = x^((q^6 - 1)(q^2 + 1)) (in the cyclotomic subgroup of order q^4 - q^2 + 1, which the cyclotomic lane tests for)"""
    S = intref.fam(name)
    recs, _, labels = mb.gt_battery(name)
    first = [labels.index(lab) for lab in dict.fromkeys(labels)]
    recs, labels = recs[first].copy(), [labels[i] for i in first]
    K, decode, nco = mb.gt_field(name)
    q, fb = S.q, S.fb
    extra = [("-1", (q - 1).to_bytes(fb, "big") + bytes((nco - 1) * fb))]
    x = decode(recs[labels.index("random element")].tobytes())
    enc = lambda y: b"".join(int(c).to_bytes(fb, "big") for c in _flat(K, y))
    if S.type in ("a", "a1"):
        y = K.pow(x, q - 1)
        assert K.pow(y, q + 1) == K.one and K.pow(y, S.r) != K.one
        extra.append(("norm 1, outside", enc(y)))
    elif S.type == "f":
        y = K.pow(x, (q ** 6 - 1) * (q ** 2 + 1))
        assert K.pow(y, q ** 4 - q ** 2 + 1) == K.one and K.pow(y, S.r) != K.one
        extra.append(("cyclotomic, outside", enc(y)))
    more = np.frombuffer(b"".join(raw for _, raw in extra), np.uint8).reshape(len(extra), nco * fb)
    return np.concatenate([recs, more]), labels + [lab for lab, _ in extra]


def gt_unit_order(name):
    """the order of the unit group of GT's field, q^k - 1 (x^that = 1 for every x != 0)"""
    S = intref.fam(name)
    K, _, nco = mb.gt_field(name)
    return S.q ** nco - 1


def gt_pow(name, recs, k):
    """-> expected records of recs[i]^k"""
    S = intref.fam(name)
    K, decode, nco = mb.gt_field(name)
    out = []
    for row in np.ascontiguousarray(recs, np.uint8):
        y = K.pow(decode(row.tobytes()), k) if k else K.one
        out.append(b"".join(int(c).to_bytes(S.fb, "big") for c in _flat(K, y)))
    return np.frombuffer(b"".join(out), np.uint8).reshape(len(out), nco * S.fb).copy()


@functools.lru_cache(maxsize=None)
def gt_expected(name):
    """-> {scalar label: (rows, expected records)}; the 512-byte scalar on two records (a pairing value, a random element)"""
    recs, labels = gt_units(name)
    ks = scalars(name, 3)
    out = {lab: (list(range(len(recs))), gt_pow(name, recs, k)) for lab, k, _ in ks[:-1]}
    rows = [labels.index("pairing value"), labels.index("random element")]
    out[ks[-1][0]] = (rows, gt_pow(name, recs[rows], ks[-1][1]))
    return out
