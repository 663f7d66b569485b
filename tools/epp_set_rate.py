#!/usr/bin/env python3
"""Rates of the multi-base power of a fixed-base table set (include/pbc_hip.h pbc_hip_element_pp_set_prod_batch_dev)
against the same result through the entry points that exist without it, on the same box in the same process, on
device-resident buffers and one stream:

    set          prod_dev of a set of m tables, n units of m scalars
    composition  m single-base element_pp objects with pow_zn_dev, m - 1 element_add_batch_dev
                 (GT: element_mul_GT_batch_dev)
    powN         for m = 2, 3: element_pow2_zn / element_pow3_zn with the bases tiled per unit

for G1 of a.param, d159.param and f.param and GT of a.param, m in {2, 3, 4, 16, 64}, n = 2^18.

    python tools/epp_set_rate.py [--steps 3] [--warmup 1] [--rounds 2] [--log2n 18] [--m 2,3,4,16,64] [a:1 d159:1 f:1 a:3]

Events around every step, a warm-up directly before every timed region, the sides in alternation, best round of each.
Before a row is timed the sides' results are compared byte for byte; a difference ends the run.  Prints one JSON line per
row and, last, the rows of the table in profiles/epp_set_notes.md."""
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


def event_timed(step, stream, args):
    import torch
    t0, spun = time.perf_counter(), 0
    while spun < max(1, args.warmup) or (time.perf_counter() - t0 < 0.3 and spun < 64):
        step()
        spun += 1
        torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for e0, e1 in evs:
        e0.record(stream)
        step()
        e1.record(stream)
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in evs) / len(evs)


def measure(name, group, m, args):
    import torch
    import oracle
    import pbc_amd
    P = pbc_amd.Pairing(pbc_amd.param_text(name))
    v = oracle.Vec(os.path.join(ROOT, "tests", "golden", FIXTURE[name]))
    src = v.gt if group == 3 else v.g1
    # base j = [j // len + 1] src[j % len]: more bases than the fixture has points are multiples of them
    k = np.zeros((m, P.length_in_bytes_Zr), np.uint8)
    k[:, -1] = np.arange(m) // len(src) + 1
    tiled = np.ascontiguousarray(src[np.arange(m) % len(src)])
    bases = P.element_pow_zn_GT(tiled, k) if group == 3 else P.element_mul_zn(group, tiled, k)
    assert len({b.tobytes() for b in bases}) == m
    n, zl, L = 1 << args.log2n, P.length_in_bytes_Zr, P._group_len(group)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * m + group)
    z = torch.randint(0, 256, (n, m, zl), dtype=torch.uint8, device="cuda", generator=gen)
    zj = [z[:, j].contiguous() for j in range(m)]                # the composition's own layout: one array of scalars per base
    S = P.element_pp_set_init(group, bases)
    pps = [P.element_pp_init(group, bases[j]) for j in range(m)]
    out = {k: torch.empty(n, L, dtype=torch.uint8, device="cuda") for k in ("set", "composition", "powN")}
    tmp = torch.empty(n, L, dtype=torch.uint8, device="cuda")

    def run_set():
        S.prod_dev(out["set"].data_ptr(), z.data_ptr(), n, stream=s)

    def run_composition():
        acc = out["composition"].data_ptr()
        pps[0].pow_zn_dev(acc, zj[0].data_ptr(), n, s)
        for j in range(1, m):
            pps[j].pow_zn_dev(tmp.data_ptr(), zj[j].data_ptr(), n, s)
            if group == 3:
                P.element_mul_GT_dev(acc, acc, tmp.data_ptr(), n, s)
            else:
                P.element_group_op_dev("add", group, acc, acc, tmp.data_ptr(), n, s)
    sides = {"set": run_set, "composition": run_composition}
    if m in (2, 3):
        bt = [torch.from_numpy(np.ascontiguousarray(np.tile(bases[j], (n, 1)))).cuda() for j in range(m)]

        def run_pow():
            P.element_pow_multi_dev(group, out["powN"].data_ptr(), [b.data_ptr() for b in bt], [x.data_ptr() for x in zj], n, s)
        sides["powN"] = run_pow
    for f in sides.values():
        f()
    torch.cuda.synchronize()
    for k in sides:
        if not torch.equal(out[k], out["set"]):
            sys.exit("epp_set_rate.py: %s differs from the set's prod (%s group %d, m = %d) -- refusing to time" % (k, name, group, m))
    ms = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, f in sides.items():
            ms[k].append(event_timed(f, stream, args))
    S.clear()
    for pp in pps:
        pp.clear()
    words = -(-P.length_in_bytes_Fq // 4)
    entry = 4 * words * (L // P.length_in_bytes_Fq) if group == 3 else 8 * words
    P.clear()
    table_mb = m * zl * (256 if group == 3 else 255) * entry / 1e6
    best = {k: min(x) for k, x in ms.items()}
    r = {"param": name, "group": group, "m": m, "n": n, "steps": args.steps, "rounds": args.rounds, "tables_mb": round(table_mb, 2),
         "ms": {k: [round(x, 3) for x in xs] for k, xs in ms.items()},
         "units_per_s": {k: round(n / (b * 1e-3)) for k, b in best.items()},
         "set_over_composition_rate": round(best["composition"] / best["set"], 3)}
    if "powN" in best:
        r["set_over_powN_rate"] = round(best["powN"] / best["set"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--m", default="2,3,4,16,64")
    ap.add_argument("cases", nargs="*", default=["a:1", "d159:1", "f:1", "a:3"])
    args = ap.parse_args()
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    import torch
    if not torch.cuda.is_available():
        sys.exit("epp_set_rate.py: no GPU -- rates are measured on the device or not at all")
    box = "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    rows = []
    for case in args.cases:
        name, group = case.split(":")
        for m in [int(x) for x in args.m.split(",")]:
            r = measure(name, int(group), m, args)
            r.update(box=box, head=head or None)
            print(json.dumps(r), flush=True)
            u = r["units_per_s"]
            rows.append("| %s %s | %d | %.2f | %d | %d | %.2f | %s |" % (name, "GT" if group == "3" else "G" + group, m, r["tables_mb"], u["set"], u["composition"],
                                                                       r["set_over_composition_rate"], "%d (%.2f)" % (u["powN"], r["set_over_powN_rate"]) if "powN" in u else ""))
    print("box: %s; commit: %s; n = 2^%d" % (box, head or "(not a git checkout)", args.log2n))
    print("| set, group | m | tables, MB | set, units/s | composition, units/s | set / composition | pow2 / pow3, units/s (set / powN) |\n|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
