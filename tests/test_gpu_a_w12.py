"""GPU tests (-m gpu) of the type a lane kernels on the weight-(1, 2) Miller steps (pairing_al.cuh double_step / add_step).
Batches this small normally take the one-pairing-per-wavefront kernels, which keep their Jacobian steps; "hip_wave_max 0"
sends them to al_pairing_kernel / al_miller_kernel + al_prod_finish_kernel, the kernels of the large batches."""
import numpy as np
import pytest

from conftest import golden, _param

pytestmark = pytest.mark.gpu

RESIDENT = 1024 * 128            # lanes of one chip residency: 256 CUs x 4 workgroups x 128 lanes


@pytest.fixture(scope="module")
def lanes():
    import pbc_amd
    return pbc_amd.Pairing(_param("a") + "hip_wave_max 0\n")


@pytest.fixture(scope="module")
def records():
    """a_rand32 followed by a_edge20 (O, off-curve records, points of order two): inputs and the reference's outputs"""
    r, e = golden("a_rand32.vec"), golden("a_edge20.vec")
    return np.concatenate([r.g1, e.g1]), np.concatenate([r.g2, e.g2]), np.concatenate([r.gt, e.gt])


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_partly_filled_workgroups(lanes, records, n):
    g1, g2, gt = records
    idx = np.arange(n) % len(g1)
    if n == 1:
        idx = np.array([40])               # an edge record, not the first random one every other test starts with
    out = lanes.element_pairing(g1[idx], g2[idx])
    assert out.shape == (n, 128)
    assert np.array_equal(out, gt[idx])


def test_one_residency_plus_one_unit(lanes, oracle_a):
    """1024 x 128 resident lanes + 1: the lane stride wraps.  Unit u pairs P_i with Q_(i + d), i = u mod 1024,
    d = u div 1024, of a_chain1024.vec: the first 1024 units are the fixture's own pairs, the others cross pairs."""
    v = golden("a_chain1024.vec")
    n = RESIDENT + 1
    u = np.arange(n)
    i, j = u % 1024, (u % 1024 + u // 1024) % 1024
    out = lanes.element_pairing(v.g1[i], v.g2[j])
    assert out.shape == (n, 128)
    assert np.array_equal(out[:1024], v.gt)
    rng = np.random.default_rng(12)
    s = np.concatenate([rng.integers(1024, n - 1, 63), [n - 1]])     # the unit past the residency among them
    assert np.array_equal(out[s], oracle_a.pairing_batch(v.g1[i[s]], v.g2[j[s]]))


def test_products_of_three_on_the_term_lanes(lanes, oracle_a):
    """130 products of three terms: al_miller_kernel over 390 terms (a partly filled fourth workgroup), then
    al_prod_finish_kernel over 130 products; the last ten are a_prod3x10_edge.vec's (unacceptable terms)"""
    v, e = golden("a_chain1024.vec"), golden("a_prod3x10_edge.vec")
    rng = np.random.default_rng(13)
    i, j = rng.integers(0, 1024, 360), rng.integers(0, 1024, 360)
    g1, g2 = np.concatenate([v.g1[i], e.g1]), np.concatenate([v.g2[j], e.g2])
    out = lanes.element_prod_pairing(g1, g2, 3)
    assert out.shape == (130, 128)
    assert np.array_equal(out[120:], e.gt)
    assert np.array_equal(out, oracle_a.prod_pairing_batch(g1, g2, 3))
