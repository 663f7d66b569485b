"""GPU tests (-m gpu) of the ragged products of pairings (include/pbc_hip.h pbc_hip_element_prod_pairing_ragged_batch / _dev):
parity with the oracle per product on every family, with the default fold factor and with "hip_ragged_fold 2" (many
levels on few terms); long products against the uniform entry point folded on the host; the identity rule at the block
boundaries of the fold; validity carried apart from the values; uniform offsets against element_prod_pairing; the
_dev form twice on one stream; the host form over pinned and pageable buffers and a device listed twice."""
import numpy as np
import pytest

import pbc_amd
from conftest import _param, golden

pytestmark = pytest.mark.gpu

# family -> (parameter file, the fixture its terms come from)
FAMILIES = {"a": ("a", "a_prod16x4.vec"), "d159": ("d159", "d_prod16x4.vec"), "f": ("f", "f_prod4x3.vec"),
            "g149": ("g149", "g149_prod4x3.vec"), "a1": ("a1", "a1_rand6.vec"), "e": ("e", "e_rand6.vec"),
            "a_160_256": ("a_160_256", "a_160_256_rand6.vec"), "d201": ("d201", "d201_rand12.vec")}
LONG = [0, 1, 2, 3, 0, 7, 16, 17, 33]
SHORT = [0, 1, 2, 5, 3]
F_DEFAULT = 16


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def _terms(family, T):
    """T term records, the family's fixture repeated as needed"""
    v = golden(FAMILIES[family][1])
    idx = np.arange(T) % len(v.g1)
    return np.ascontiguousarray(v.g1[idx]), np.ascontiguousarray(v.g2[idx])


@pytest.fixture(scope="module")
def objs():
    """(family, fold) -> the product; fold None: the default"""
    class Lazy(dict):
        def __missing__(self, key):
            family, fold = key
            self[key] = pbc_amd.Pairing(_param(FAMILIES[family][0]) + ("hip_ragged_fold %d\n" % fold if fold else ""))
            return self[key]
    return Lazy()


@pytest.fixture(scope="module")
def ones(oracles):
    class Lazy(dict):
        def __missing__(self, family):
            O = oracles[FAMILIES[family][0]]
            self[family] = O.gt_pow(golden(FAMILIES[family][1]).gt[:1], np.zeros((1, 4), np.uint8))[0]
            return self[family]
    return Lazy()


def _oracle_products(O, one, g1, g2, off):
    out = np.empty((len(off) - 1, len(one)), np.uint8)
    for u in range(len(off) - 1):
        a, b = int(off[u]), int(off[u + 1])
        out[u] = O.prod_pairing_batch(g1[a:b], g2[a:b], b - a)[0] if b > a else one
    return out


@pytest.fixture(scope="module")
def expected(oracles, ones):
    """(family, lengths) -> terms, offsets and the oracle's products: computed once, shared by the cases"""
    class Lazy(dict):
        def __missing__(self, key):
            family, lengths = key
            off = _offsets(lengths)
            g1, g2 = _terms(family, int(off[-1]))
            self[key] = (g1, g2, off, _oracle_products(oracles[FAMILIES[family][0]], ones[family], g1, g2, off))
            return self[key]
    return Lazy()


PARITY = [(f, tuple(LONG)) for f in ("a", "d159", "f", "g149")] + [(f, tuple(SHORT)) for f in ("a1", "e")] + \
         [(f, (2, 0, 5)) for f in ("a_160_256", "d201")]


@pytest.mark.parametrize("fold", [None, 2])
@pytest.mark.parametrize("family,lengths", PARITY)
def test_parity_per_family(objs, expected, family, lengths, fold):
    """a, d159, f, g149: [0, 1, 2, 3, 0, 7, 16, 17, 33] (79 terms: empty products, one term, F, F + 1, 2 F + 1 of the
    default); a1, e: [0, 1, 2, 5, 3]; a generated type a size and another d file: [2, 0, 5].  Fold 2: up to six levels."""
    g1, g2, off, want = expected[(family, lengths)]
    got = objs[(family, fold)].element_prod_pairing_ragged(g1, g2, off)
    assert got.shape == want.shape
    bad = [u for u in range(len(want)) if not np.array_equal(got[u], want[u])]
    assert not bad, bad


def _host_fold(H, gts):
    """the product of GT records, folded with element_mul_GT"""
    while len(gts) > 1:
        half = len(gts) // 2
        head = H.element_mul_GT(gts[:half], gts[half:2 * half])
        gts = np.concatenate([head, gts[2 * half:]])
    return gts[0]


@pytest.mark.parametrize("family,count,k,n", [("a", 4097, 17, 241), ("d159", 1025, 25, 41)])
def test_long_products(objs, oracles, ones, family, count, k, n):
    """[1, count, 2] with the default fold: count crosses two fold levels.  The long product: the uniform entry point on
    the same terms (k x n = count), folded on the host with element_mul_GT; the neighbours: the oracle."""
    assert k * n == count and count > F_DEFAULT * F_DEFAULT
    H = objs[(family, None)]
    off = _offsets([1, count, 2])
    g1, g2 = _terms(family, int(off[-1]))
    got = H.element_prod_pairing_ragged(g1, g2, off)
    want_long = _host_fold(H, H.element_prod_pairing(g1[1:1 + count], g2[1:1 + count], k))
    O = oracles[FAMILIES[family][0]]
    assert np.array_equal(got[1], want_long)
    assert np.array_equal(got[0], O.pairing_batch(g1[:1], g2[:1])[0])
    assert np.array_equal(got[2], O.prod_pairing_batch(g1[-2:], g2[-2:], 2)[0])
    assert not np.array_equal(got[1], ones[family])


@pytest.mark.parametrize("family", ["a", "d159"])
def test_identity_rule_at_block_boundaries(objs, expected, ones, family):
    """an all-zero record and an off-curve record, in G1 and in G2 (d159: the twist), as the first, the last, the F-th
    and the (F + 1)-th term of a product of 2 F + 1 terms: that product is the identity, its neighbours (3 and 2 terms)
    keep the oracle's values.  The 16 variants travel in one call."""
    F = F_DEFAULT
    lengths = (3, 2 * F + 1, 2)
    g1, g2, off, want = expected[(family, lengths)]
    T = int(off[-1])
    G1, G2, W, L = [], [], [], []
    for kind in ("zero", "off-curve"):
        for group in (1, 2):
            for pos in (0, 2 * F, F - 1, F):
                a, b = g1.copy(), g2.copy()
                rec = (a if group == 1 else b)[3 + pos]
                if kind == "zero":
                    rec[:] = 0
                else:
                    rec[-1] ^= 1                              # the lowest bit of y: no longer a root of x^3 + a x + b
                w = want.copy()
                w[1] = ones[family]
                G1.append(a); G2.append(b); W.append(w); L.extend(lengths)
    got = objs[(family, None)].element_prod_pairing_ragged(np.concatenate(G1), np.concatenate(G2), _offsets(L))
    assert len(got) == 48 and T == 38
    W = np.concatenate(W)
    bad = [u for u in range(len(W)) if not np.array_equal(got[u], W[u])]
    assert not bad, bad
    assert not np.array_equal(want[1], ones[family])          # (the untouched product is not the identity)


@pytest.mark.parametrize("fold", [None, 2])
@pytest.mark.parametrize("family", ["a", "f"])
def test_flags_are_not_inferred_from_values(objs, oracles, ones, family, fold):
    """[(P, Q), (-P, Q), (P2, Q2)] = e(P2, Q2): the first two terms multiply to 1, yet every flag is valid;
    [(O, Q), (P2, Q2)] is the identity although e(O, Q) has the bytes of 1"""
    H = objs[(family, fold)]
    g1, g2 = _terms(family, 2)
    negP = H.element_group_op("neg", 1, g1[:1])
    a = np.concatenate([g1[:1], negP, g1[1:2], np.zeros_like(g1[:1]), g1[1:2]])
    b = np.concatenate([g2[:1], g2[:1], g2[1:2], g2[:1], g2[1:2]])
    got = H.element_prod_pairing_ragged(a, b, _offsets([3, 2]))
    want = oracles[FAMILIES[family][0]].pairing_batch(g1[1:2], g2[1:2])[0]
    assert not np.array_equal(want, ones[family])
    assert np.array_equal(got[0], want)
    assert np.array_equal(got[1], ones[family])


@pytest.mark.parametrize("family", ["a", "d159"])
def test_uniform_offsets_give_element_prod_pairing(objs, family):
    """k = 16, n = 400: 6400 terms, above hip_wave_max"""
    H = objs[(family, None)]
    g1, g2 = _terms(family, 6400)
    got = H.element_prod_pairing_ragged(g1, g2, np.arange(401, dtype=np.uint64) * 16)
    assert np.array_equal(got, H.element_prod_pairing(g1, g2, 16))


@pytest.mark.parametrize("family", ["a", "d159"])
def test_dev_form_twice_on_one_stream(objs, expected, family):
    """two calls back to back on a non-default stream with different offsets and outputs, one synchronisation: the
    second call's plan must not disturb the first call's kernels.  The offsets arrays are overwritten right after each call."""
    import torch
    H = objs[(family, 2)]                                      # fold 2: every call reads several levels of its plan
    st = torch.cuda.Stream()
    runs = []
    for lengths in (tuple(LONG), (5, 0, 9, 1)):
        g1, g2, off, want = expected[(family, lengths)]
        d1, d2 = torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()
        out = torch.full((len(want) * want.shape[1] + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        runs.append((d1, d2, out, off.copy(), want))
    torch.cuda.synchronize()
    for d1, d2, out, off, want in runs:
        H.element_prod_pairing_ragged_dev(out.data_ptr(), d1.data_ptr(), d2.data_ptr(), off, stream=st.cuda_stream)
        off[:] = 0xFFFFFFFF
    st.synchronize()
    for d1, d2, out, off, want in runs:
        got = out.cpu().numpy()
        assert (got[want.size:] == 0xA5).all()
        assert np.array_equal(got[:want.size].reshape(want.shape), want)


@pytest.mark.parametrize("family", ["a", "d159"])
def test_host_form_buffers_and_device_set(expected, family):
    """pinned buffers, pageable buffers (the wrapper's arrays), chunks of 20 terms ("hip_host_chunk 20": several chunks on
    the ring of streams, a 33-term product a chunk of its own), and use_devices([0, 0]): two ranges balanced by terms"""
    import torch
    g1, g2, off, want = expected[(family, tuple(LONG))]
    H = pbc_amd.Pairing(_param(FAMILIES[family][0]) + "hip_host_chunk 20\n")
    assert np.array_equal(H.element_prod_pairing_ragged(g1, g2, off), want)              # pageable
    h1, h2 = torch.from_numpy(g1).pin_memory(), torch.from_numpy(g2).pin_memory()
    out = torch.zeros(want.shape, dtype=torch.uint8).pin_memory()
    assert pbc_amd.lib().pbc_hip_element_prod_pairing_ragged_batch(H._h, out.data_ptr(), h1.data_ptr(), h2.data_ptr(), off.ctypes.data, len(off) - 1) == 0
    assert np.array_equal(out.numpy(), want)                                             # pinned
    H.use_devices([0, 0])
    assert np.array_equal(H.element_prod_pairing_ragged(g1, g2, off), want)
    H.use_devices([])
    H.clear()
    D = pbc_amd.Pairing(_param(FAMILIES[family][0]))
    D.use_devices([0, 0])
    assert np.array_equal(D.element_prod_pairing_ragged(g1, g2, off), want)
    D.clear()
