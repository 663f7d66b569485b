#!/usr/bin/env python3
"""Rate of pbc_hip_is_almost_coddh_batch_dev against the composition a caller had to write before it existed -- two
element_pairing_dev, element_mul_GT_dev, then the comparisons in torch -- on the same box in the same run, on
device-resident buffers and one stream, timed with events after the warm-up bench_group.py uses (the warm-up steps
topped up to 0.3 s of launches).  The two are timed in alternation, several rounds each.

    python tools/coddh_rate.py [--steps 5] [--warmup 2] [--rounds 3] [a:20 d159:18 f:18]

Prints one JSON line per parameter set and, last, the rows of the table in profiles/coddh_notes.md."""
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


def measure(pname, log2n, args):
    import torch
    import oracle
    import pbc_amd
    P = pbc_amd.Pairing(pbc_amd.param_text(pname))
    v = oracle.Vec(os.path.join(ROOT, "tests", "golden", FIXTURE[pname]))
    n = 1 << log2n
    LT = P.length_in_bytes_GT
    i = np.arange(n) % v.n
    # unit j: (P_i, P_i, Q_i, Q_i) -- verdict 1 -- and every third one (P_i, P_i+1, Q_i, Q_i) -- verdict 0
    nx = np.where(np.arange(n) % 3 == 0, (i + 1) % v.n, i)
    a, b, c, d = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v.g1[i], v.g1[nx], v.g2[i], v.g2[i]))
    want = torch.from_numpy((nx == i).astype(np.uint8)).cuda()
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    T0 = torch.empty(n, LT, dtype=torch.uint8, device="cuda")
    T1 = torch.empty(n, LT, dtype=torch.uint8, device="cuda")
    M = torch.empty(n, LT, dtype=torch.uint8, device="cuda")
    one = np.zeros(LT, np.uint8)
    one[P.length_in_bytes_Fq - 1] = 1
    d_one = torch.from_numpy(one).cuda()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    out = {}

    def entry():
        P.is_almost_coddh_dev(res.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), n, stream=s)
        out["entry"] = res

    def composition():
        P.element_pairing_dev(T0.data_ptr(), a.data_ptr(), d.data_ptr(), n, s)
        P.element_pairing_dev(T1.data_ptr(), b.data_ptr(), c.data_ptr(), n, s)
        P.element_mul_GT_dev(M.data_ptr(), T0.data_ptr(), T1.data_ptr(), n, s)
        out["composition"] = ((T0 == T1).all(dim=1) | (M == d_one).all(dim=1)).to(torch.uint8)

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
    composition()
    torch.cuda.synchronize()
    if not (torch.equal(out["entry"], want) and torch.equal(out["composition"], want)):
        sys.exit("coddh_rate.py: %s verdicts differ from the construction -- refusing to time" % pname)
    ms = {"entry": [], "composition": []}
    for _ in range(args.rounds):
        ms["entry"].append(timed(entry))
        ms["composition"].append(timed(composition))
    P.clear()
    best = {k: min(x) for k, x in ms.items()}
    return {"param": pname, "log2n": log2n, "steps": args.steps, "rounds": args.rounds,
            "entry_ms": [round(x, 3) for x in ms["entry"]], "composition_ms": [round(x, 3) for x in ms["composition"]],
            "entry_verdicts_per_s": round(n / best["entry"] * 1e3, 1), "composition_verdicts_per_s": round(n / best["composition"] * 1e3, 1),
            "entry_over_composition": round(best["composition"] / best["entry"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("sets", nargs="*", default=["a:20", "d159:18", "f:18"])
    args = ap.parse_args()
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    import torch
    box = "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    rows = []
    for spec in args.sets:
        pname, log2n = spec.split(":")
        r = measure(pname, int(log2n), args)
        r.update(box=box, head=head or None)
        print(json.dumps(r), flush=True)
        rows.append("| %s | 2^%d | %.1f | %.1f | %.4f |" % (pname, r["log2n"], r["entry_verdicts_per_s"], r["composition_verdicts_per_s"],
                                                         r["entry_over_composition"]))
    print("box: %s; commit: %s" % (box, head or "(not a git checkout)"))
    print("| parameters | batch | is_almost_coddh_batch_dev, verdicts/s | composition, verdicts/s | entry / composition |\n|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
