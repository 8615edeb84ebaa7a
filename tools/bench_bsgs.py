#!/usr/bin/env python3
"""Baby-step/giant-step linear transform -- a plaintext matrix times an encrypted vector with babies + giants rotations (CKKS N = 16384,
6 x 50-bit, L = 5).

For (babies, giants) in {(4,4), (8,8), (8,32)} and batch in {1, 64} one run times, in the same process, alternating the variants round by round:
  bsgs       troyn_linear_transform_bsgs                 one decomposition, `giants` divisions for the inner sums, ONE for the outer sum
  composed   troyn_apply_galois_weighted_sums, then per giant step troyn_apply_galois + troyn_switch_key and troyn_add: 2 * giants divisions
The composed form only uses entries that predate the one-call entry, with every buffer prepared beforehand, so it stands for the library
without the addition on the same commit.  Every giant step is keyed in both variants (no identity).  The results are NOT compared word for
word (the composed form rounds once per giant step; include/troyn.h); tests/test_gpu_bsgs.py checks the words against the specification.
Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device
synchronise.

python tools/bench_bsgs.py [--reps 10] [--rounds 3] [--shapes 4x4,8x8,8x32] [--batches 1,64]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry
import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="4x4,8x8,8x32")
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bsgs.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L = 16384, 14, 5
    q = pkg.capi.coeff_modulus_create(n, [50] * 6)
    plan = pkg.Plan(dev, log_n, q)
    gen = torch.Generator(device=dev).manual_seed(6)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    max_b, max_g = max(b for b, _ in shapes), max(g for _, g in shapes)
    key = lambda: [bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)]
    baby_keys, giant_keys = [key() for _ in range(max_b)], [key() for _ in range(max_g)]
    baby_el = [pow(3, t + 1, 2 * n) for t in range(max_b)]                       # rotations by 1 .. babies steps
    weights = [[bench.uniform_residues(torch, (), q, n, dev, gen).view(len(q), n) for _ in range(max_b)] for _ in range(max_g)]
    print("# %s; CKKS N=%d, 6 x 50-bit, L=%d; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L, args.reps, args.rounds), flush=True)
    for babies, giants in shapes:
        giant_el = [pow(3, babies * (g + 1), 2 * n) for g in range(giants)]      # rotations by babies, 2 babies, ... steps
        for batch in [int(x) for x in args.batches.split(",")]:
            ct = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
            o_bsgs = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)
            o_composed = torch.empty_like(o_bsgs)
            inner = torch.empty((giants, batch, 2, L, n), dtype=torch.int64, device=dev)
            rotated = torch.empty_like(o_bsgs)
            target = torch.empty((batch, L, n), dtype=torch.int64, device=dev)
            bel, bks, gks = baby_el[:babies], baby_keys[:babies], giant_keys[:giants]
            rows = [row[:babies] for row in weights[:giants]]

            def bsgs():
                plan.linear_transform_bsgs(L, ct, bel, bks, giant_el, gks, rows, out=o_bsgs)

            def composed():
                plan.apply_galois_weighted_sums(L, ct, bel, bks, rows, out=inner)
                for g in range(giants):
                    dest = o_composed if g == 0 else rotated
                    plan.apply_galois_poly(inner[g], L, giant_el[g], True, out=dest)
                    target.copy_(dest[:, 1])
                    plan.switch_key(L, target, gks[g], dest=dest, assign=pkg.ASSIGN_OVERWRITE_EXCEPT_FIRST)
                    if g:
                        plan.add(o_composed, rotated, L, out=o_composed)

            variants = [("bsgs", bsgs), ("composed", composed)]
            times = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    times[name].append(bench.timed(torch, fn, args.reps))
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"babies": babies, "giants": giants, "batch": batch,
                   "ms": {k: round(med[k] * 1e3, 4) for k in med},
                   "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
                   "diagonals_per_s_bsgs": round(babies * giants * batch / med["bsgs"], 1),
                   "speedup_bsgs_vs_composed": round(med["composed"] / med["bsgs"], 4)}
            print(json.dumps(rec), flush=True)
            print("babies %d giants %2d batch %3d: bsgs %.3f ms | composed %.3f ms (x%.3f)" %
                  (babies, giants, batch, med["bsgs"] * 1e3, med["composed"] * 1e3, rec["speedup_bsgs_vs_composed"]), flush=True)
            del ct, o_bsgs, o_composed, inner, rotated, target
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
