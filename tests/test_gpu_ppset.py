"""GPU tests (-m gpu) of the table sets (include/pbc_hip.h pbc_hip_pairing_pp_set_*): the segmented apply against m
calls on single tables and against the oracle, per family; the resident loop over several strides; products over a set
against the reference's product fixtures and against the uniform entry point with tiled first arguments; the _dev forms
back to back on one stream and on a set built on that stream; the host form in several chunks."""
import numpy as np
import pytest

import pbc_amd
from conftest import _param, golden

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 0, 130]
COUNTS_A1 = [0, 1, 2, 0, 65]          # a lane of a1.param needs 0.2 s
# family -> (parameter file, the fixture its records come from, units per table)
FAMILIES = {"a": ("a", "a_chain1024.vec", COUNTS), "a_160_256": ("a_160_256", "a_160_256_rand6.vec", COUNTS),
            "a1": ("a1", "a1_chain8.vec", COUNTS_A1), "d159": ("d159", "d_chain256.vec", COUNTS),
            "g149": ("g149", "g149_chain64.vec", COUNTS)}


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def _records(family, m, n):
    """m first arguments and n second arguments, the family's fixture repeated as needed"""
    v = golden(FAMILIES[family][1])
    return np.ascontiguousarray(v.g1[np.arange(m) % len(v.g1)]), np.ascontiguousarray(v.g2[(np.arange(n) * 7 + 3) % len(v.g2)])


@pytest.fixture(scope="module")
def objs():
    class Lazy(dict):
        def __missing__(self, family):
            self[family] = pbc_amd.Pairing(_param(FAMILIES[family][0]))
            return self[family]
    return Lazy()


@pytest.fixture(scope="module")
def ones(oracles):
    class Lazy(dict):
        def __missing__(self, family):
            O = oracles[FAMILIES[family][0]]
            self[family] = O.gt_pow(golden(FAMILIES[family][1]).gt[:1], np.zeros((1, 4), np.uint8))[0]
            return self[family]
    return Lazy()


@pytest.fixture(scope="module")
def segmented(objs):
    """family -> (g1, g2, offsets, expected): one off-curve first argument (the table of 64 units; a1: of 2) and one
    off-curve g2 in the middle of the last segment; expected = m calls of pbc_hip_pairing_pp_apply_batch on tables of
    pbc_hip_pairing_pp_init.  Computed once, shared by the cases, never written."""
    class Lazy(dict):
        def __missing__(self, family):
            counts = FAMILIES[family][2]
            off = _offsets(counts)
            g1, g2 = _records(family, len(counts), int(off[-1]))
            bad_table = 3 if len(counts) == 7 else 2
            g1[bad_table, -1] ^= 1
            g2[int(off[-2]) + counts[-1] // 2, -1] ^= 1
            H = objs[family]
            want = np.empty((int(off[-1]), H.length_in_bytes_GT), np.uint8)
            for t, c in enumerate(counts):
                if c:
                    pp = H.pp_init(g1[t])
                    want[int(off[t]):int(off[t + 1])] = pp.apply(g2[int(off[t]):int(off[t + 1])])
                    pp.clear()
            self[family] = (g1, g2, off, want, bad_table)
            return self[family]
    return Lazy()


# ---- segmented apply ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_segmented_apply_per_family(objs, oracles, ones, segmented, family):
    g1, g2, off, want, bad_table = segmented[family]
    H = objs[family]
    S = H.pp_set_init(g1)
    assert S.m == len(g1)
    got = S.apply(g2, off)
    S.clear()
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:10]
    one = ones[family]
    a, b = int(off[bad_table]), int(off[bad_table + 1])
    assert b > a and all(np.array_equal(r, one) for r in got[a:b])               # the off-curve first argument
    mid = int(off[-2]) + FAMILIES[family][2][-1] // 2
    assert np.array_equal(got[mid], one) and not np.array_equal(got[mid - 1], one) and not np.array_equal(got[mid + 1], one)
    # at most 8 units against the oracle: the first and the last unit of tables, the two identities among them
    table_of = np.searchsorted(off, np.arange(len(g2)), side="right") - 1
    units = sorted({int(off[1]), int(off[2]), a, b - 1, mid - 1, mid, len(g2) - 1})[:8]
    O = oracles[FAMILIES[family][0]]
    ref = O.pairing_batch(g1[table_of[units]], g2[units])
    assert np.array_equal(got[units], ref)


def test_segmented_apply_over_several_strides_of_the_resident_loop(segmented):
    """a.param with "hip_resident_slots 2": two workgroups, four wave slots a stride, eight slots"""
    g1, g2, off, want, _ = segmented["a"]
    H = pbc_amd.Pairing(_param("a") + "hip_resident_slots 2\n")
    S = H.pp_set_init(g1)
    assert len(S.plan(off)) == 8
    assert np.array_equal(S.apply(g2, off), want)
    S.clear()
    H.clear()


@pytest.mark.parametrize("family", ["a", "d159"])
def test_host_form_in_chunks_and_empty_calls(segmented, family):
    """"hip_host_chunk 100": four staged chunks, each with its own plan cut out of the offsets; all tables empty: nothing to do"""
    g1, g2, off, want, _ = segmented[family]
    H = pbc_amd.Pairing(_param(FAMILIES[family][0]) + "hip_host_chunk 100\n")
    S = H.pp_set_init(g1)
    assert np.array_equal(S.apply(g2, off), want)
    assert S.apply(g2[:0], np.zeros(len(g1) + 1, np.uint64)).shape == (0, H.length_in_bytes_GT)
    with pytest.raises(pbc_amd.PbcHipError, match="offsets decrease at index 1"):
        S.apply(g2[:5], np.array([0, 5, 3] + [5] * (len(g1) - 2), np.uint64))
    with pytest.raises(pbc_amd.PbcHipError, match=r"offsets\[0\] must be 0"):
        S.apply(g2[:5], np.array([1] + [5] * len(g1), np.uint64))
    S.clear()
    H.clear()


# ---- products -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,vec", [("a", "a_prod16x4.vec"), ("a", "a_prod3x10_edge.vec"),
                                        ("d159", "d_prod16x4.vec"), ("d159", "d_prod3x10_edge.vec")])
def test_products_of_the_reference_fixtures(objs, family, vec):
    """every product of the fixture as a set of its k first arguments with n = 1: the fixture's bytes"""
    v = golden(vec)
    H = objs[family]
    for u in range(v.n):
        S = H.pp_set_init(v.g1[u * v.k:(u + 1) * v.k])
        got = S.prod(v.g2[u * v.k:(u + 1) * v.k])
        S.clear()
        assert got.shape == (1, v.lenT)
        assert np.array_equal(got[0], v.gt[u]), (vec, u)


@pytest.mark.parametrize("family", ["a", "d159", "g149"])
def test_product_shapes_against_the_uniform_entry_point(objs, ones, family):
    """m in {1, 2, 3} x n in {1, 65, 130} against pbc_hip_element_prod_pairing_batch with the first arguments tiled; an O
    first argument makes every product the identity; an off-curve g2 term makes its product the identity and no other;
    n == 0 is an empty result"""
    H = objs[family]
    one = ones[family]
    for m in (1, 2, 3):
        g1, g2 = _records(family, m, 130 * m)
        S = H.pp_set_init(g1)
        for n in (1, 65, 130):
            b = g2[:n * m].copy()
            hit = (n // 2) * m + (m - 1)
            b[hit, -1] ^= 1                                              # off the curve, in product n // 2 only
            got = S.prod(b)
            want = H.element_prod_pairing(np.tile(g1, (n, 1)), b, m)
            assert np.array_equal(got, want), (m, n)
            assert np.array_equal(got[n // 2], one)
            assert sum(np.array_equal(r, one) for r in got) == 1
        assert S.prod(g2[:0]).shape == (0, H.length_in_bytes_GT)
        S.clear()
        g1o = g1.copy()
        g1o[m - 1] = 0                                                   # the all-zero record: O
        S = H.pp_set_init(g1o)
        got = S.prod(g2[:65 * m])
        S.clear()
        assert np.array_equal(got, H.element_prod_pairing(np.tile(g1o, (65, 1)), g2[:65 * m], m))
        assert all(np.array_equal(r, one) for r in got)


# ---- the _dev forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["a", "d159"])
def test_dev_forms_on_one_stream(objs, segmented, family):
    """a set built with _init_dev on a non-default stream and used on that stream without a host synchronisation: two
    segmented calls back to back with different offsets (each array overwritten right after its call), then a product
    call; one synchronisation at the end"""
    import torch
    g1, g2, off, want, _ = segmented[family]
    H = objs[family]
    m, lt = len(g1), H.length_in_bytes_GT
    off2 = _offsets([5, 0, 70, 1, 0, 64, 3])
    n2 = int(off2[-1])
    want2 = np.empty((n2, lt), np.uint8)
    for t in range(m):
        if off2[t + 1] > off2[t]:
            pp = H.pp_init(g1[t])
            want2[int(off2[t]):int(off2[t + 1])] = pp.apply(g2[int(off2[t]):int(off2[t + 1])])
            pp.clear()
    nprod = 9
    want3 = H.element_prod_pairing(np.tile(g1, (nprod, 1)), g2[:nprod * m], m)
    d1, d2 = torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()
    outs = [torch.full((k * lt + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k in (len(want), n2, nprod)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    S = H.pp_set_init_dev(d1.data_ptr(), m, stream=st.cuda_stream)
    for out, o in ((outs[0], off.copy()), (outs[1], off2.copy())):
        S.apply_dev(out.data_ptr(), d2.data_ptr(), o, stream=st.cuda_stream)
        o[:] = 0xFFFFFFFF
    S.prod_dev(outs[2].data_ptr(), d2.data_ptr(), nprod, stream=st.cuda_stream)
    st.synchronize()
    for out, w in zip(outs, (want, want2, want3)):
        got = out.cpu().numpy()
        assert (got[w.size:] == 0xA5).all()
        assert np.array_equal(got[:w.size].reshape(w.shape), w)
    S.clear()
