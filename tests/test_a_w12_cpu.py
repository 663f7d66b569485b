"""CPU tests of the limb-form type a Miller loop in weight-(1, 2) coordinates (pairing_al.cuh double_step / add_step:
x = X / Z, y = Y / Z^2) on the host mirror (tests/hostsim): AL<16>::pairing_lane and the one-term-per-lane product against
the reference's stored outputs, bit for bit.  The mirror carries a worst-case (limb size, value) bound through every
operation and aborts the process when one is violated, so one pass over any input proves the bounds for all inputs."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, golden, _param

hostsim = pytest.importorskip("hostsim")

STEPS = 159                      # doubling steps of a.param's Miller loop (exp2)
PARENT_MACS = 2146508            # multiply-adds of one pairing with the Jacobian steps (9 M + 6 S + 2 two-term sums a step)
M, S, SOP2 = 648, 495, 972       # multiply-adds of a product, a squaring, a two-term sum (18 limbs)


@pytest.fixture(scope="module")
def sims():
    class Lazy(dict):
        def __missing__(self, name):
            self[name] = hostsim.HostSim(_param(name))
            return self[name]
    return Lazy()


FIXTURES = [
    ("a", "a_rand32.vec"),
    ("a", "a_edge20.vec"),                      # O, off-curve records, points of order two
    ("a", "a_full12.vec"),                      # points of the whole curve, outside the order-r subgroup
    ("a_160_512_mm", "a_160_512_mm_rand6.vec"),  # r = 2^160 - 2^31 - 1: the addition step takes -P
]


@pytest.mark.parametrize("pname,name", FIXTURES)
def test_single_pairings_match_reference(sims, pname, name):
    v = golden(name)
    assert v.k == 1
    assert np.array_equal(sims[pname].prod_pairing(v.g1, v.g2, 1), v.gt)


@pytest.mark.parametrize("pname,name", FIXTURES)
def test_products_of_three_over_the_same_records(sims, oracles, pname, name):
    """one term per lane (miller_record_lane), then prod_finish_lane, over the records of the same fixtures taken three at
    a time: the product of the three stored outputs where every record is acceptable (the reference's GT
    multiplication), and the compiled reference's element_prod_pairing on all of them"""
    v = golden(name)
    n = v.n // 3
    g1, g2 = v.g1[:3 * n], v.g2[:3 * n]
    got = sims[pname].prod_pairing(g1, g2, 3)
    assert np.array_equal(got, oracles[pname].prod_pairing_batch(g1, g2, 3))
    if name != "a_edge20.vec":
        O = oracles[pname]
        assert np.array_equal(got, O.gt_mul(O.gt_mul(v.gt[0:3 * n:3], v.gt[1:3 * n:3]), v.gt[2:3 * n:3]))


def test_stored_products_of_three_with_a_negated_addition_step(sims):
    """(a.param's stored products, a_prod3x10_edge.vec and a_prodfull3x4.vec, run through the same routines in
    test_hostsim.py)"""
    v = golden("a_160_512_mm_prod3x4_edge.vec")
    assert v.k == 3
    assert np.array_equal(sims["a_160_512_mm"].prod_pairing(v.g1, v.g2, 3), v.gt)


def test_multiply_adds_of_one_pairing(sims):
    """The doubling step is 5 M + 5 S + 1 two-term sum for point and line where the Jacobian one took 7 M + 6 S: 819
    multiply-adds fewer, the full target (495 would have been the saving with the line's real part as two products).
    The addition step, once per pairing, is 12 M + 4 S where the Jacobian one took 11 M + 3 S.  Reached:
    159 x 819 - 1143 = 129 078 fewer than the parent's 2 146 508."""
    v = golden("a_rand32.vec")
    sim = sims["a"]
    sim.macs(reset=True)
    sim.prod_pairing(v.g1[:1], v.g2[:1], 1)
    macs = sim.macs(reset=True)
    table = json.load(open(os.path.join(ROOT, "profiles", "executed_macs.json")))
    assert macs == table["a"]["executed_macs_per_unit"]
    assert macs <= PARENT_MACS - STEPS * S
    assert (2 * M + S) - SOP2 == 819
    assert macs == PARENT_MACS - STEPS * 819 + (M + S)
    # control flow is data-independent: a second pairing, an edge record, costs the same
    e = golden("a_edge20.vec")
    sim.prod_pairing(e.g1[:1], e.g2[:1], 1)
    assert sim.macs(reset=True) == macs
    # ... and a term of a product is the same Miller loop
    sim.prod_pairing(v.g1[:3], v.g2[:3], 3)
    per3 = sim.macs(reset=True)
    sim.prod_pairing(v.g1[:2], v.g2[:2], 2)
    per2 = sim.macs(reset=True)
    assert table["a-prod16"]["executed_macs_per_unit"] == per2 + 14 * (per3 - per2)
