#!/usr/bin/env python3
"""Times of pbc_hip_element_prod_pairing_ragged_batch_dev against the entry points it is measured by, on the same box in
the same run, on device-resident buffers and one stream, timed with events after the warm-up tools/coddh_rate.py uses
(the warm-up steps topped up to 0.3 s of launches), the sides in alternation, several rounds each:

    long   ONE product of 2^L terms            against  element_pairing_dev on 2^L units (strictly more arithmetic)
    short  2^L products of 16 terms, uniform   against  element_prod_pairing_dev, n = 2^L, k = 16

    python tools/ragged_rate.py [--steps 5] [--warmup 2] [--rounds 3] [--fold 4,8,16,32,64] [a:long:16 a:short:16 d159:long:16 f:long:16]

--fold: one row per fold factor ("hip_ragged_fold N"; default: the library's).  The yardsticks are entry points whose
kernels this feature does not touch, so both sides come from one build.  Prints one JSON line per row and, last, the
rows of the table in profiles/ragged_notes.md."""
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


def measure(pname, shape, log2n, fold, args):
    import torch
    import oracle
    import pbc_amd
    P = pbc_amd.Pairing(pbc_amd.param_text(pname) + ("hip_ragged_fold %d\n" % fold if fold else ""))
    ragged = hasattr(pbc_amd.lib(), "pbc_hip_element_prod_pairing_ragged_batch_dev")
    v = oracle.Vec(os.path.join(ROOT, "tests", "golden", FIXTURE[pname]))
    LT = P.length_in_bytes_GT
    if shape == "long":
        T, n = 1 << log2n, 1
        off = np.array([0, T], np.uint64)
    else:
        T, n = 16 << log2n, 1 << log2n
        off = np.arange(n + 1, dtype=np.uint64) * 16
    i = np.arange(T) % v.n
    g1, g2 = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v.g1[i], v.g2[i]))
    out_r = torch.empty(n, LT, dtype=torch.uint8, device="cuda")
    out_y = torch.empty(T if shape == "long" else n, LT, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream

    def entry():
        P.element_prod_pairing_ragged_dev(out_r.data_ptr(), g1.data_ptr(), g2.data_ptr(), off, stream=s)

    def yardstick():
        if shape == "long":
            P.element_pairing_dev(out_y.data_ptr(), g1.data_ptr(), g2.data_ptr(), T, s)
        else:
            P.element_prod_pairing_dev(out_y.data_ptr(), g1.data_ptr(), g2.data_ptr(), n, 16, s)

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

    sides = {"yardstick": yardstick}
    if ragged:
        sides["entry"] = entry
        entry()
        yardstick()
        torch.cuda.synchronize()
        if shape == "short" and not torch.equal(out_r, out_y):
            sys.exit("ragged_rate.py: %s: the ragged call differs from element_prod_pairing -- refusing to time" % pname)
    ms = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, f in sides.items():
            ms[k].append(timed(f))
    P.clear()
    best = {k: min(x) for k, x in ms.items()}
    r = {"param": pname, "shape": shape, "log2n": log2n, "terms": T, "products": n, "fold": fold or "default", "steps": args.steps,
         "rounds": args.rounds, "yardstick_ms": [round(x, 3) for x in ms["yardstick"]]}
    if ragged:
        r.update(entry_ms=[round(x, 3) for x in ms["entry"]], entry_over_yardstick=round(best["entry"] / best["yardstick"], 4))
    return r, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fold", default="")
    ap.add_argument("sets", nargs="*", default=["a:long:16", "a:short:16", "d159:long:16", "f:long:16"])
    args = ap.parse_args()
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    import torch
    box = "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    folds = [int(x) for x in args.fold.split(",") if x] or [0]
    rows = []
    for spec in args.sets:
        pname, shape, log2n = spec.split(":")
        for fold in folds:
            r, best = measure(pname, shape, int(log2n), fold, args)
            r.update(box=box, head=head or None, lib=os.environ.get("PBC_HIP_LIB", "libpbc_hip.so"))
            print(json.dumps(r), flush=True)
            rows.append("| %s | %s | 2^%d | %s | %s | %.3f | %s |" % (
                pname, shape, r["log2n"], r["fold"], "%.3f" % best["entry"] if "entry" in best else "-", best["yardstick"],
                "%.4f" % r["entry_over_yardstick"] if "entry" in best else "-"))
    print("box: %s; commit: %s; library: %s" % (box, head or "(not a git checkout)", os.environ.get("PBC_HIP_LIB", "libpbc_hip.so")))
    print("| parameters | shape | 2^L | fold | ragged call, ms | yardstick, ms | ragged / yardstick |\n|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
