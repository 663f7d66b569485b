#!/usr/bin/env python3
"""Times of the table-set entry points (include/pbc_hip.h pbc_hip_pairing_pp_set_*) on a.param against the paths they
replace, on the same box in the same process, on device-resident buffers and one stream:

    init   a set of m = 1024 tables, one launch         against  1024 calls of pbc_hip_pairing_pp_init
    apply  one segmented apply of 1024 x 128 units      against  1024 calls of pbc_hip_pairing_pp_apply_batch_dev (128 units each)
    prod   pp_set_prod, m = 16, n = 2^16                 against  pbc_hip_element_prod_pairing_batch_dev, n = 2^16, k = 16, same terms

    python tools/pp_set_rate.py [--steps 5] [--warmup 2] [--rounds 3] [--tables 1024] [--units 128] [--log2n 16] [init apply prod]

init is timed with the host clock (both sides return when their tables are built); apply and prod with events around
every step after the warm-up of tools/ragged_rate.py, the sides in alternation, best round of each.  The yardsticks are
entry points this feature leaves as they are, so both sides come from one build.  Before anything is timed the two
sides' results are compared; a difference ends the run.  Prints one JSON line per row and, last, the rows of the table
in profiles/pp_set_notes.md."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_timed(step, stream, args):
    import torch
    t0, spun = time.perf_counter(), 0
    while spun < max(1, args.warmup) or (time.perf_counter() - t0 < 0.3 and spun < 256):
        step()
        spun += 1
        if spun >= max(1, args.warmup):
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for e0, e1 in evs:
        e0.record(stream)
        step()
        e1.record(stream)
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in evs) / len(evs)


def host_timed(step, args):
    import torch
    for _ in range(max(1, args.warmup)):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sum(ms) / len(ms)


def rounds(sides, timer, args):
    ms = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, f in sides.items():
            ms[k].append(timer(f))
    return ms


def measure(what, args):
    import torch
    import oracle
    import pbc_amd
    P = pbc_amd.Pairing(pbc_amd.param_text("a"))
    v = oracle.Vec(os.path.join(ROOT, "tests", "golden", "a_chain1024.vec"))
    LT = P.length_in_bytes_GT
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    if what == "init":
        m = args.tables
        g1 = np.ascontiguousarray(v.g1[np.arange(m) % v.n])
        keep = []

        def entry():
            keep.append(P.pp_set_init(g1))
            keep.pop().clear()

        def yardstick():
            for t in range(m):
                P.pp_init(g1[t]).clear()
        shape = "%d tables" % m
        ms = rounds({"entry": entry, "yardstick": yardstick}, lambda f: host_timed(f, args), args)
    elif what == "apply":
        m, c = args.tables, args.units
        n = m * c
        g1 = np.ascontiguousarray(v.g1[np.arange(m) % v.n])
        g2 = torch.from_numpy(np.ascontiguousarray(v.g2[(np.arange(n) * 7 + 3) % v.n])).cuda()
        off = np.arange(m + 1, dtype=np.uint64) * c
        S = P.pp_set_init(g1)
        pps = [P.pp_init(g1[t]) for t in range(m)]
        out_e = torch.empty(n, LT, dtype=torch.uint8, device="cuda")
        out_y = torch.empty(n, LT, dtype=torch.uint8, device="cuda")
        l2 = P.length_in_bytes_G2

        def entry():
            S.apply_dev(out_e.data_ptr(), g2.data_ptr(), off, stream=s)

        def yardstick():
            for t in range(m):
                pps[t].apply_dev(out_y.data_ptr() + t * c * LT, g2.data_ptr() + t * c * l2, c, s)
        entry()
        yardstick()
        torch.cuda.synchronize()
        if not torch.equal(out_e, out_y):
            sys.exit("pp_set_rate.py: the segmented apply differs from the single tables -- refusing to time")
        shape = "%d tables x %d units" % (m, c)
        ms = rounds({"entry": entry, "yardstick": yardstick}, lambda f: event_timed(f, stream, args), args)
        S.clear()
        for pp in pps:
            pp.clear()
    else:
        m, n = 16, 1 << args.log2n
        g1 = np.ascontiguousarray(v.g1[np.arange(m) % v.n])
        g2 = torch.from_numpy(np.ascontiguousarray(v.g2[(np.arange(n * m) * 7 + 3) % v.n])).cuda()
        g1t = torch.from_numpy(np.ascontiguousarray(np.tile(g1, (n, 1)))).cuda()
        S = P.pp_set_init(g1)
        out_e = torch.empty(n, LT, dtype=torch.uint8, device="cuda")
        out_y = torch.empty(n, LT, dtype=torch.uint8, device="cuda")

        def entry():
            S.prod_dev(out_e.data_ptr(), g2.data_ptr(), n, stream=s)

        def yardstick():
            P.element_prod_pairing_dev(out_y.data_ptr(), g1t.data_ptr(), g2.data_ptr(), n, m, s)
        entry()
        yardstick()
        torch.cuda.synchronize()
        if not torch.equal(out_e, out_y):
            sys.exit("pp_set_rate.py: the product over the set differs from element_prod_pairing -- refusing to time")
        shape = "m = 16, n = 2^%d" % args.log2n
        ms = rounds({"entry": entry, "yardstick": yardstick}, lambda f: event_timed(f, stream, args), args)
        S.clear()
    P.clear()
    best = {k: min(x) for k, x in ms.items()}
    r = {"what": what, "shape": shape, "steps": args.steps, "rounds": args.rounds, "entry_ms": [round(x, 3) for x in ms["entry"]],
         "yardstick_ms": [round(x, 3) for x in ms["yardstick"]], "entry_over_yardstick": round(best["entry"] / best["yardstick"], 4)}
    return r, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--units", type=int, default=128)
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("rows", nargs="*", default=["init", "apply", "prod"])
    args = ap.parse_args()
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    import torch
    box = "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    rows = []
    for what in args.rows:
        if what not in ("init", "apply", "prod"):
            sys.exit("pp_set_rate.py: unknown row %r" % what)
        r, best = measure(what, args)
        r.update(box=box, head=head or None)
        print(json.dumps(r), flush=True)
        rows.append("| %s | %s | %.3f | %.3f | %.4f |" % (what, r["shape"], best["entry"], best["yardstick"], r["entry_over_yardstick"]))
    print("box: %s; commit: %s" % (box, head or "(not a git checkout)"))
    print("| row | shape | table set, ms | yardstick, ms | set / yardstick |\n|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
