#!/usr/bin/env python3
"""Rate of pbc_hip_element_mul_mpz_batch_dev (a) against the only way the parent commit offers for the same job (b):
pbc_hip_element_mul_zn_batch_dev / pbc_hip_element_pow_zn_GT_batch_dev fed the scalar replicated n times -- in one
process, on one build, on device-resident buffers and one stream, timed with events after the warm-up bench_group.py uses
(the warm-up steps topped up to 0.3 s of launches, directly before the timed steps).  (a) and (b) are timed in
alternation, `--rounds` rounds each; the best round of each is compared and the spread of (b)'s rounds is the margin:
the requirement is (a) >= (b) - spread on every row.  Rows where (b) cannot run (integers above a Z_r record: the cofactor
of a_160_1024, #E'/r on the d159 twist) report (a) alone.

    python tools/mul_mpz_bench.py [--steps 5] [--warmup 2] [--rounds 3] [rows: param:group:log2n ...]

Inputs are the fixture's records, tiled (G1: points of the order-r subgroup; G2 of types d, f: points of the whole twist;
GT: pairing values).  Before a row is timed the two results are compared byte for byte.
Prints one JSON line per row and, last, the rows of the table in profiles/mul_mpz_notes.md."""
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
FIXTURE = {"a": "a_rand32.vec", "d159": "d_rand32.vec", "f": "f_rand16.vec", "g149": "g149_rand16.vec", "a_160_1024": "a_160_1024_rand4.vec"}
ROWS = ["a:1:20", "d159:1:18", "d159:2:18", "f:1:18", "f:2:18", "g149:1:18", "a:3:20", "d159:3:18", "f:3:18"]
ALONE = ["a_160_1024:1:18:cofactor", "d159:2:18:cofactor"]


def params(text):
    out = {}
    for line in text.splitlines():
        f = line.split()
        if len(f) == 2 and f[1].lstrip("-").isdigit():
            out[f[0]] = int(f[1])
    return out


def twist_order_d(p):
    """#E'(F_q^d) of a type d / g set: the twist of E over F_q^d, E of trace t = q + 1 - n over F_q"""
    q, n, d = p["q"], p["n"], p["k"] // 2
    t = q + 1 - n
    tj, tprev = t, 2
    for _ in range(d - 1):
        tj, tprev = t * tj - q * tprev, tj
    return q ** d + 1 + tj


def scalars(pname, p, lz, kind):
    """[(label, k)] of a row"""
    r = p["r"]
    if kind == "cofactor":
        if pname == "a_160_1024":
            return [("(q + 1) / r, %d bits" % p["h"].bit_length(), p["h"])]
        N = twist_order_d(p)
        assert N % r == 0
        return [("#E' / r, %d bits" % (N // r).bit_length(), N // r)]
    rng = np.random.default_rng(20 + lz)
    rnd = (1 << (8 * lz - 1)) | int.from_bytes(rng.bytes(lz), "big") >> 1
    return [("random, %d bits" % rnd.bit_length(), rnd % (1 << (8 * lz))), ("r", r), ("2^64 + 1", (1 << 64) + 1)]


def measure(spec, args):
    import torch
    import oracle
    import pbc_amd
    f = spec.split(":")
    pname, group, log2n, kind = f[0], int(f[1]), int(f[2]), (f[3] if len(f) > 3 else "")
    text = pbc_amd.param_text(pname)
    p = params(text)
    P = pbc_amd.Pairing(text)
    v = oracle.Vec(os.path.join(ROOT, "tests", "golden", FIXTURE[pname]))
    n = 1 << log2n
    recs = v.g1 if group == 1 else v.g2 if group == 2 else v.gt
    lrec, lz = recs.shape[1], P.length_in_bytes_Zr
    x = torch.from_numpy(np.ascontiguousarray(recs[np.arange(n) % v.n])).cuda()
    out_a = torch.empty(n, lrec, dtype=torch.uint8, device="cuda")
    out_b = torch.empty(n, lrec, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []

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

    for lab, k in scalars(pname, p, lz, kind):
        fits = k < (1 << (8 * lz)) and kind != "cofactor"
        z = torch.from_numpy(np.ascontiguousarray(np.tile(np.frombuffer(k.to_bytes(lz, "big"), np.uint8), (n, 1)))).cuda() if fits else None

        def new():
            P.element_mul_mpz_dev(group, out_a.data_ptr(), x.data_ptr(), k, n, s)

        def old():
            if group == 3:
                P.element_pow_zn_GT_dev(out_b.data_ptr(), x.data_ptr(), z.data_ptr(), n, s)
            else:
                P.element_mul_zn_dev(group, out_b.data_ptr(), x.data_ptr(), z.data_ptr(), n, s)

        new()
        if fits:
            old()
        torch.cuda.synchronize()
        if fits and not torch.equal(out_a, out_b):
            sys.exit("mul_mpz_bench.py: %s group %d, k = %s: the two results differ -- refusing to time" % (pname, group, lab))
        ms = {"a": [], "b": []}
        for _ in range(args.rounds):
            ms["a"].append(timed(new))
            if fits:
                ms["b"].append(timed(old))
        digits = pbc_amd.Pairing.mpz_digits(k, 1 if group == 3 else 0)
        w = 1 if group == 3 else (2 if np.array_equal(digits, pbc_amd.Pairing.mpz_digits(k, 2)) else 4)
        row = {"param": pname, "group": group, "log2n": log2n, "k": lab, "w": w, "digits": int(digits.size), "nonzero": int(np.count_nonzero(digits)),
               "steps": args.steps, "rounds": args.rounds, "a_ms": [round(t, 3) for t in ms["a"]], "b_ms": [round(t, 3) for t in ms["b"]]}
        if fits:
            spread = max(ms["b"]) - min(ms["b"])
            row.update(b_spread_ms=round(spread, 3), a_over_b=round(min(ms["b"]) / min(ms["a"]), 4), ok=bool(min(ms["a"]) <= min(ms["b"]) + spread))
        rows.append(row)
    P.clear()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("rows", nargs="*", default=ROWS + ALONE)
    args = ap.parse_args()
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    import torch
    box = "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))
    table = []
    for spec in args.rows:
        for r in measure(spec, args):
            r.update(box=box, head=head or None)
            print(json.dumps(r), flush=True)
            g = "GT" if r["group"] == 3 else "G%d" % r["group"]
            b = "%.3f" % min(r["b_ms"]) if r["b_ms"] else "cannot run"
            tail = "%.3f | %.3f | %s" % (r["b_spread_ms"], r["a_over_b"], "yes" if r["ok"] else "NO") if r["b_ms"] else "- | - | -"
            table.append("| %s | %s | 2^%d | %s | %d | %d / %d | %.3f | %s | %s |" % (r["param"], g, r["log2n"], r["k"], r["w"], r["nonzero"], r["digits"],
                                                                                  min(r["a_ms"]), b, tail))
    print("box: %s; commit: %s" % (box, head or "(not a git checkout)"))
    print("| parameters | group | batch | k | w | non-zero / digits | (a) mul_mpz, ms | (b) replicated Z_r records, ms | spread of (b), ms | (b) / (a) | (a) >= (b) - spread |\n" + "|---" * 11 + "|")
    print("\n".join(table))


if __name__ == "__main__":
    main()
