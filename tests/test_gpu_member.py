"""GPU tests of pbc_hip_element_membership_batch / _dev (include/pbc_hip.h): the batteries of tests/member_battery.py
(expected classes: exact integers, tests/intref.py) through the library on its default route and with "hip_group_slow 1"
(every lane through the complete pass / the generic power), whole and in slices that cross a wavefront and a workgroup
with the flagged units first, last and alone; the _dev form on a stream of its own; two host threads on one stream."""
import numpy as np
import pytest

import member_battery as mb
import pbc_amd
from conftest import _param

pytestmark = pytest.mark.gpu

SETS = ["a", "a1", "d159", "e", "f", "g149", "d201", "a_160_256"]
WIDE = ("a1", "e")                                               # 33-word fields: one slice per route
LENGTHS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def pairings():
    """(name, slow) -> the library's object"""
    class Lazy(dict):
        def __missing__(self, key):
            name, slow = key
            self[key] = pbc_amd.Pairing(_param(name) + ("hip_group_slow 1\n" if slow else ""))
            return self[key]
    objs = Lazy()
    yield objs
    for H in objs.values():
        H.clear()


def _battery(name, group):
    return mb.gt_battery(name) if group == 3 else mb.point_battery(name, group)


def _special(name, group):
    """-> (label, row) of the unit the slices place first, last and alone.  G1 / G2: member_battery.flagged_unit -- a point
    of order 3, 4, 6 or 2 with class OUTSIDE, which the fast lane flags for the complete pass (asserted on the host mirror,
    tests/test_member_cpu.py); a.param GT: an element of norm != 1, which the Lucas lane flags for the generic power.
    Where nothing can be flagged (f, g149 G1: curves of prime order; GT elsewhere: one kernel) it is just a unit of
    another class than its neighbours, and the label says so"""
    _, want, labels = _battery(name, group)
    if group == 3:
        if name == "a":
            return "flagged", labels.index("random element")
        return "odd one out", labels.index("random element")
    f = mb.flagged_unit(name, group)
    if f is not None:
        assert want[f] == mb.OUTSIDE
        return "flagged", f
    return "odd one out", labels.index("off curve")


def _slices(name, group):
    """[(label, row indices)]: lengths 1, 63, 64, 65, 257 of subgroup points / pairing values with the special unit first,
    last, and alone, and the battery in its own order (flagged units mid-batch)"""
    _, want, labels = _battery(name, group)
    kind, f = _special(name, group)
    plain = [i for i, lab in enumerate(labels) if lab in ("subgroup", "pairing value")]
    out = []
    for n in ((65,) if name in WIDE else LENGTHS):
        if n == 1:
            out.append(("%s alone" % kind, [f]))
            continue
        fill = [plain[i % len(plain)] for i in range(n)]
        out.append(("%d %s first" % (n, kind), [f] + fill[1:]))
        if name not in WIDE:
            out.append(("%d %s last" % (n, kind), fill[:-1] + [f]))
            out.append(("%d battery order" % n, [i % len(labels) for i in range(n)]))
    return out


def test_slices_place_a_flagged_unit_where_one_exists():
    """every type a / a1 / e set, and d159 / d201 on both groups, have a unit the fast lane flags, and the slices use it"""
    for name in SETS:
        for group in (1, 2):
            kind, f = _special(name, group)
            assert (kind == "flagged") == (name not in ("f", "g149")), (name, group)
    assert _special("a", 3)[0] == "flagged"


@pytest.mark.parametrize("slow", [False, True], ids=["default", "group_slow"])
@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("name", SETS)
def test_membership_batch(pairings, name, group, slow):
    H = pairings[(name, slow)]
    recs, want, labels = _battery(name, group)
    got = H.element_membership(group, recs)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = [(i, labels[i], int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad
    for lab, rows in _slices(name, group):
        got = H.element_membership(group, recs[rows])
        assert np.array_equal(got, want[rows]), (lab, [labels[i] for i, (g, w) in zip(rows, zip(got, want[rows])) if g != w])


@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("name", ["a", "d159", "f"])
def test_membership_dev_on_its_own_stream(pairings, name, group):
    """the _dev form on a non-default stream: the host form's bytes, nothing but the n result bytes written"""
    import torch
    H = pairings[(name, False)]
    recs, want, _ = _battery(name, group)
    rows = [i % len(recs) for i in range(257)]
    host = H.element_membership(group, recs[rows])
    assert np.array_equal(host, want[rows])
    d_in = torch.from_numpy(np.ascontiguousarray(recs[rows])).cuda()
    d_res = torch.full((len(rows) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    H.element_membership_dev(group, d_res.data_ptr(), d_in.data_ptr(), len(rows), s.cuda_stream)
    s.synchronize()
    out = d_res.cpu().numpy()
    assert np.array_equal(out[:len(rows)], host) and (out[len(rows):] == 0xEE).all()
    assert np.array_equal(d_in.cpu().numpy(), recs[rows])


def test_empty_batch_succeeds_and_touches_nothing(pairings):
    import ctypes
    H = pairings[("d159", False)]
    res = np.full(8, 0xEE, np.uint8)
    L = pbc_amd.lib()
    for group in (1, 2, 3):
        assert L.pbc_hip_element_membership_batch(H._h, group, ctypes.c_void_p(res.ctypes.data), None, 0) == 0
        assert L.pbc_hip_element_membership_batch_dev(H._h, group, None, None, 0, None) == 0
        assert H.element_membership(group, np.zeros((0, 1), np.uint8)).shape == (0,)
    assert (res == 0xEE).all()


def test_two_threads_issue_on_one_stream(pairings):
    """two host threads enqueue the two-pass call (a.param G1: the limb-form kernel + the complete kernel for the lanes it
    flags, sharing the flags workspace of (device, stream)) on the SAME stream of one object, as
    test_gpu_group2.py test_two_threads_issue_on_one_stream does for the other operations: every result equals the
    single-threaded one.  The batches mix flagged units (small orders) with subgroup points at different places."""
    import threading
    import torch
    H = pairings[("a", False)]
    recs, want, labels = mb.point_battery("a", 1)
    n, rounds = 3000, 8
    jobs = []
    for t in range(2):
        rows = np.array([(i * (3 + 2 * t) + t) % len(recs) for i in range(n)])
        x = np.ascontiguousarray(recs[rows])
        single = H.element_membership(1, x)
        assert np.array_equal(single, want[rows])
        jobs.append((x, single))
    outs = [[torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(rounds)] for _ in range(2)]
    dev = [torch.from_numpy(x).cuda() for x, _ in jobs]
    torch.cuda.synchronize()
    errs = []

    def worker(t):
        try:
            for i in range(rounds):
                H.element_membership_dev(1, outs[t][i].data_ptr(), dev[t].data_ptr(), n, 0)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for t in range(2):
        for i in range(rounds):
            assert np.array_equal(outs[t][i].cpu().numpy(), jobs[t][1]), (t, i)
