#!/usr/bin/env python3
"""Rate of pbc_hip_element_membership_batch_dev against the way a caller had to get the same answer before it existed --
pbc_hip_element_mul_zn_batch_dev with every scalar = r, then a scan of the result records for zeros (the scan is NOT
counted) -- on the same box in the same run, on device-resident buffers and one stream, timed with events after the
warm-up bench_group.py uses (the warm-up steps topped up to 0.3 s of launches).  The two are timed in alternation,
several rounds each; the best round of each is compared.  The inputs are the fixture's points (G1: of the order-r
subgroup; G2 of types d, f: points of the whole twist, as the reference draws them), tiled.

    python tools/membership_bench.py [--steps 5] [--warmup 2] [--rounds 3] [a:1:20 d159:1:18 d159:2:18 f:1:18 f:2:18]

Prints one JSON line per row and, last, the rows of the table in profiles/membership_notes.md."""
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
FIXTURE = {"a": "a_rand32.vec", "d159": "d_rand32.vec", "f": "f_rand16.vec"}


def group_order(text, key="r"):
    for line in text.splitlines():
        f = line.split()
        if len(f) == 2 and f[0] == key:
            return int(f[1])
    raise KeyError(key)


def measure(pname, group, log2n, args):
    import torch
    import oracle
    import pbc_amd
    text = pbc_amd.param_text(pname)
    P = pbc_amd.Pairing(text)
    v = oracle.Vec(os.path.join(ROOT, "tests", "golden", FIXTURE[pname]))
    n = 1 << log2n
    pts = v.g1 if group == 1 else v.g2
    lp, lz = pts.shape[1], P.length_in_bytes_Zr
    x = torch.from_numpy(np.ascontiguousarray(pts[np.arange(n) % v.n])).cuda()
    r = np.frombuffer(group_order(text).to_bytes(lz, "big"), np.uint8)
    z = torch.from_numpy(np.ascontiguousarray(np.tile(r, (n, 1)))).cuda()
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, lp, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream

    def entry():
        P.element_membership_dev(group, res.data_ptr(), x.data_ptr(), n, s)

    def mul_by_r():
        P.element_mul_zn_dev(group, out.data_ptr(), x.data_ptr(), z.data_ptr(), n, s)

    def timed(step):
        spin_t0, spun = time.perf_counter(), 0
        while spun < max(1, args.warmup) or (time.perf_counter() - spin_t0 < 0.3 and spun < 256):
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

    entry()
    mul_by_r()
    torch.cuda.synchronize()
    # the two must tell the same story before anything is timed: finite points of the curve, INSIDE <=> [r] P is the zero record
    inside = (out == 0).all(dim=1)
    if not torch.equal(res, torch.where(inside, 2, 1).to(torch.uint8)):
        sys.exit("membership_bench.py: %s group %d: the verdicts differ from [r] P -- refusing to time" % (pname, group))
    ms = {"entry": [], "mul_by_r": []}
    for _ in range(args.rounds):
        ms["entry"].append(timed(entry))
        ms["mul_by_r"].append(timed(mul_by_r))
    share = float(inside.float().mean())
    P.clear()
    best = {k: min(t) for k, t in ms.items()}
    return {"param": pname, "group": group, "log2n": log2n, "steps": args.steps, "rounds": args.rounds, "inside_share": round(share, 4),
            "entry_ms": [round(t, 3) for t in ms["entry"]], "mul_by_r_ms": [round(t, 3) for t in ms["mul_by_r"]],
            "entry_units_per_s": round(n / best["entry"] * 1e3, 1), "mul_by_r_units_per_s": round(n / best["mul_by_r"] * 1e3, 1),
            "entry_over_mul_by_r": round(best["mul_by_r"] / best["entry"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("rows", nargs="*", default=["a:1:20", "d159:1:18", "d159:2:18", "f:1:18", "f:2:18"])
    args = ap.parse_args()
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    import torch
    box = "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    table = []
    for spec in args.rows:
        pname, group, log2n = spec.split(":")
        r = measure(pname, int(group), int(log2n), args)
        r.update(box=box, head=head or None)
        print(json.dumps(r), flush=True)
        table.append("| %s | G%d | 2^%d | %.2f | %.1f | %.1f | %.4f |" % (pname, r["group"], r["log2n"], r["inside_share"], r["entry_units_per_s"],
                                                                     r["mul_by_r_units_per_s"], r["entry_over_mul_by_r"]))
    print("box: %s; commit: %s" % (box, head or "(not a git checkout)"))
    print("| parameters | group | batch | share INSIDE | element_membership_batch_dev, units/s | element_mul_zn_batch_dev with r, units/s | ratio |\n|---|---|---|---|---|---|---|")
    print("\n".join(table))


if __name__ == "__main__":
    main()
