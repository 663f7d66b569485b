"""GPU tests (-m gpu) of the fixed-base table sets (include/pbc_hip.h pbc_hip_element_pp_set_*): multi-base powers against
the exact-integer records of tests/eppset_battery.py and against the entry points that already exist (the single-base
object, pow2_zn / pow3_zn, mul_zn + add), per family and group; the crafted bases, with and without "hip_group_slow 1";
segmented powers against single-base objects; the _dev forms back to back on one stream, on a set built on that stream;
a set cleared and rebuilt; the 33-word sets through the host-buffer form."""
import numpy as np
import pytest

import eppset_battery as eb
import intref
import pbc_amd
from conftest import _param

pytestmark = pytest.mark.gpu

SETS = ["a", "d159", "f", "g149"]
NS = (1, 63, 64, 65, 129)                                        # 129: one more than a workgroup
COUNTS = [0, 1, 63, 64, 65, 0, 130]


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


@pytest.fixture(scope="module")
def objs():
    class Lazy(dict):
        def __missing__(self, key):
            name, extra = key if isinstance(key, tuple) else (key, "")
            self[key] = pbc_amd.Pairing(_param(name) + extra)
            return self[key]
    return Lazy()


def _zl(name):
    return intref.fam(name).zl


def _composition(H, group, bases, z):
    """sum_j [z_j] B_j through the entry points that exist without the set: element_mul_zn + element_add, folded left to
    right (GT: element_pow_zn + element_mul)"""
    n, m = len(z), len(bases)
    zl = z.shape[1] // m
    acc = None
    for j in range(m):
        b, zj = np.ascontiguousarray(np.tile(bases[j], (n, 1))), np.ascontiguousarray(z[:, j * zl:(j + 1) * zl])
        if group == 3:
            t = H.element_pow_zn_GT(b, zj)
            acc = t if acc is None else H.element_mul_GT(acc, t)
        else:
            t = H.element_mul_zn(group, b, zj)
            acc = t if acc is None else H.element_group_op("add", group, acc, t)
    return acc


def _multi(H, group, bases, z):
    """element_pow2_zn / element_pow3_zn with the bases tiled"""
    n, m = len(z), len(bases)
    zl = z.shape[1] // m
    return H.element_pow_multi(group, [np.ascontiguousarray(np.tile(bases[j], (n, 1))) for j in range(m)],
                               [np.ascontiguousarray(z[:, j * zl:(j + 1) * zl]) for j in range(m)])


def _random_rows(name, group, m, n, salt):
    rng = intref._rng(name, 500 + 10 * group + salt)
    return np.frombuffer(rng.bytes(n * m * _zl(name)), np.uint8).reshape(n, m * _zl(name)).copy()


# ---- multi-base powers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("name", SETS)
def test_prod_shapes_against_intref_and_the_existing_entry_points(objs, name, group):
    """m in {1, 2, 3, 5} x n in {1, 63, 64, 65, 129} on distinct fixture bases: the battery's rows, repeated, equal intref's
    records; 129 random units equal the single-base object (m = 1), pow2_zn / pow3_zn (m = 2, 3) and mul_zn + add (m = 5)
    byte for byte"""
    H = objs[name]
    for m in (1, 2, 3, 5):
        bases = eb.base_set(name, group, "distinct")[0][:m]
        S = H.element_pp_set_init(group, bases)
        assert S.m == S.count() == m
        rows, want = eb.zr_bytes(name, group, "distinct", m), eb.expected(name, group, "distinct", m)
        for n in NS:
            z, idx = eb.tiled(rows, n)
            got = S.prod(z)
            bad = [i for i in range(n) if not np.array_equal(got[i], want[idx[i]])]
            assert not bad, (m, n, bad[:8])
        z = _random_rows(name, group, m, 129, m)
        got = S.prod(z)
        if m == 1:
            pp = H.element_pp_init(group, bases[0])
            ref = pp.pow_zn(z)
            pp.clear()
        elif m in (2, 3):
            ref = _multi(H, group, bases, z)
        else:
            ref = _composition(H, group, bases, z)
        assert np.array_equal(got, ref), m
        assert S.prod(z[:0]).shape == (0, S.length)
        S.clear()


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", SETS)
def test_crafted_bases(objs, name, group):
    """the crafted-base batteries: a repeated base and an opposite pair with the rows that cancel and meet (the fast lane
    has to hand them to the complete lane), a set with O, an off-curve record and a point of small order among its bases,
    and the set all of whose tables are "complete only" -- intref's records, the rows placed so that a wavefront mixes them;
    the same bytes with "hip_group_slow 1"; the related set also against mul_zn + add"""
    for extra in ("", "hip_group_slow 1\n"):
        H = objs[(name, extra)]
        for kind in ("related", "crafted", "complete"):
            bases = eb.base_set(name, group, kind)[0]
            m = len(bases)
            S = H.element_pp_set_init(group, bases)
            rows, want = eb.zr_bytes(name, group, kind, m), eb.expected(name, group, kind, m)
            z, idx = eb.tiled(rows, 129)
            got = S.prod(z)
            bad = [i for i in range(len(z)) if not np.array_equal(got[i], want[idx[i]])]
            assert not bad, (kind, extra, bad[:8])
            if kind == "related" and not extra:
                assert np.array_equal(got, _composition(H, group, bases, z))
            S.clear()


@pytest.mark.parametrize("name", SETS)
def test_gt_related_bases(objs, name):
    """GT: a repeated base, a record with coordinates >= q and the identity among the bases"""
    H = objs[name]
    bases = eb.base_set(name, 3, "related")[0]
    S = H.element_pp_set_init(3, bases)
    rows, want = eb.zr_bytes(name, 3, "related", len(bases)), eb.expected(name, 3, "related", len(bases))
    z, idx = eb.tiled(rows, 65)
    assert np.array_equal(S.prod(z), want[idx])
    S.clear()


# ---- segmented powers -----------------------------------------------------------------------------------------------------
def _segment_bases(name, group):
    """7 bases: fixture points, one O and one of small order (the off-curve record where the curve has no such point)"""
    if group == 3:
        d, r = eb.base_set(name, 3, "distinct")[0], eb.base_set(name, 3, "related")[0]
        return np.stack([d[0], d[1], r[4], d[2], r[3], d[3], d[4]])          # (the identity and coordinates >= q among them)
    d, c = eb.base_set(name, group, "distinct")[0], eb.base_set(name, group, "crafted")
    special = [i for i, lab in enumerate(c[1]) if lab.startswith("order ")] or [c[1].index("off curve")]
    return np.stack([d[0], d[1], c[0][c[1].index("O")], d[2], c[0][special[0]], d[3], d[4]])


@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("name", SETS)
def test_segmented_pow_zn_equals_the_single_base_objects(objs, name, group):
    """counts [0, 1, 63, 64, 65, 0, 130] over 7 bases: every segment equals pbc_hip_element_pp_pow_zn_batch on a
    single-base object for its base; the segment of O is all zero bytes; with "hip_group_slow 1" the same bytes; bad
    offsets are refused on a live set"""
    H = objs[name]
    bases = _segment_bases(name, group)
    off = _offsets(COUNTS)
    n = int(off[-1])
    z = _random_rows(name, group, 1, n, 7)
    r = intref.fam(name).r
    for i, k in enumerate((0, 1, r - 1, r, (1 << (8 * _zl(name))) - 1)):                 # edge scalars at the front of the widest segments
        for t in (3, 4, 6):
            z[int(off[t]) + i] = np.frombuffer(int(k).to_bytes(_zl(name), "big"), np.uint8)
    want = np.empty((n, H._group_len(group)), np.uint8)
    for t, c in enumerate(COUNTS):
        if c:
            pp = H.element_pp_init(group, bases[t])
            want[int(off[t]):int(off[t + 1])] = pp.pow_zn(z[int(off[t]):int(off[t + 1])])
            pp.clear()
    S = H.element_pp_set_init(group, bases)
    got = S.pow_zn(z, off)
    bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:8]
    if group != 3:
        assert not got[int(off[2]):int(off[3])].any()            # the segment of O
        assert got[int(off[3]):int(off[4])][5:].any(axis=1).all()
    assert S.pow_zn(z[:0], np.zeros(8, np.uint64)).shape == (0, S.length)
    with pytest.raises(pbc_amd.PbcHipError, match="offsets decrease at index 1"):
        S.pow_zn(z[:5], np.array([0, 5, 3, 5, 5, 5, 5, 5], np.uint64))
    with pytest.raises(pbc_amd.PbcHipError, match=r"offsets\[0\] must be 0"):
        S.pow_zn(z[:5], np.array([1, 5, 5, 5, 5, 5, 5, 5], np.uint64))
    S.clear()
    if group != 3:
        Hs = objs[(name, "hip_group_slow 1\n")]
        S = Hs.element_pp_set_init(group, bases)
        assert np.array_equal(S.pow_zn(z, off), want)
        S.clear()


def test_host_form_in_chunks(objs):
    """"hip_host_chunk 100": several staged chunks, each lane finding its table from the call's offsets and its own unit number"""
    name, group = "d159", 1
    H = objs[(name, "hip_host_chunk 100\n")]
    bases = _segment_bases(name, group)
    off = _offsets(COUNTS)
    z = _random_rows(name, group, 1, int(off[-1]), 8)
    S, R = H.element_pp_set_init(group, bases), objs[name].element_pp_set_init(group, bases)
    assert np.array_equal(S.pow_zn(z, off), R.pow_zn(z, off))
    zz = _random_rows(name, group, 7, 130, 9)
    assert np.array_equal(S.prod(zz), R.prod(zz))
    assert np.array_equal(R.prod(zz), _composition(objs[name], group, bases, zz))
    S.clear()
    R.clear()


# ---- the _dev forms, set reuse ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", [("a", 1), ("d159", 2), ("f", 3)])
def test_dev_forms_on_one_stream(objs, name, group):
    """a set built with _init_dev on a non-default stream and used at once on that stream: a multi-base power, then two
    segmented calls back to back with different offsets (each array overwritten right after its call); one
    synchronisation at the end; nothing written past the results.  Then the set is cleared and rebuilt from host records"""
    import torch
    H = objs[name]
    bases = _segment_bases(name, group)
    m, L, zl = len(bases), H._group_len(group), _zl(name)
    off, off2 = _offsets(COUNTS), _offsets([5, 0, 70, 1, 0, 64, 3])
    n1, n2, n3 = int(off[-1]), int(off2[-1]), 65
    z = _random_rows(name, group, 1, n1, 11)
    zp = _random_rows(name, group, m, n3, 12)
    R = H.element_pp_set_init(group, bases)                      # the host-buffer forms: checked above against the other entry points
    want = (R.prod(zp), R.pow_zn(z, off), R.pow_zn(z[:n2], off2))
    R.clear()
    db, dz, dzp = torch.from_numpy(bases).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(zp).cuda()
    outs = [torch.full((k * L + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k in (n3, n1, n2)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    S = H.element_pp_set_init_dev(group, db.data_ptr(), m, stream=st.cuda_stream)
    S.prod_dev(outs[0].data_ptr(), dzp.data_ptr(), n3, stream=st.cuda_stream)
    for out, o in ((outs[1], off.copy()), (outs[2], off2.copy())):
        S.pow_zn_dev(out.data_ptr(), dz.data_ptr(), o, stream=st.cuda_stream)
        o[:] = 0xFFFFFFFF
    st.synchronize()
    for out, w in zip(outs, want):
        got = out.cpu().numpy()
        assert (got[w.size:] == 0xA5).all()
        assert np.array_equal(got[:w.size].reshape(w.shape), w)
    S.clear()
    S = H.element_pp_set_init(group, bases[::-1].copy())        # cleared and rebuilt, the bases in another order
    assert np.array_equal(S.prod(np.ascontiguousarray(zp.reshape(n3, m, zl)[:, ::-1].reshape(n3, m * zl))), want[0])
    S.clear()


@pytest.mark.parametrize("name", ["e", "a1"])
def test_wide_sets_through_the_host_buffer_form(objs, name):
    """the 33-word sets, m = 2, n = 65: the battery's rows against intref's records, random rows against pow2_zn; GT too"""
    H = objs[name]
    for group in (1, 3):
        bases = eb.base_set(name, group, "distinct")[0][:2]
        S = H.element_pp_set_init(group, bases)
        rows, want = eb.zr_bytes(name, group, "distinct", 2), eb.expected(name, group, "distinct", 2)
        z, idx = eb.tiled(rows, 65)
        z[len(rows):] = _random_rows(name, group, 2, 65 - len(rows), 13)
        got = S.prod(z)
        assert np.array_equal(got[:len(rows)], want)
        assert np.array_equal(got, _multi(H, group, bases, z))
        S.clear()
