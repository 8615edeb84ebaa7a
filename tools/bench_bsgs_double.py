#!/usr/bin/env python3
"""Double-hoisted against single-hoisted baby-step/giant-step linear transform (CKKS N = 16384, 6 x 50-bit, L = 5; BFV N = 8192
{60,40,40,60}, L = 3).

For (babies, giants) in {(4,4), (8,8)} and batch in {1, 64} one run times, in the same process, alternating the variants round by round:
  single   troyn_linear_transform_bsgs                  `giants` divisions of both components for the inner sums, ONE for the outer sum
  double   troyn_linear_transform_bsgs_double_hoisted   per giant step one division of component 1 alone, ONE for the outer sum
Every giant step is keyed in both variants (no identity).  The two results are NOT compared word for word: they differ by design
(include/troyn.h).  Once per point the single-hoisted entry is checked word for word against its Plan-level composition
(apply_galois_weighted_sums, then apply_galois_sum_each).  The double-hoisted entry has no such composition -- the undivided inner sums
never leave the workspace -- so it is checked to give the same words on a second call into a fresh buffer; its words are pinned to the
specification by tests/test_gpu_bsgs_double.py.
Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device
synchronise; a point is the median of `rounds` rounds.

python tools/bench_bsgs_double.py [--reps 10] [--rounds 3] [--shapes 4x4,8x8] [--batches 1,64] [--schemes ckks,bfv]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry
import bench

CONFIGS = {"ckks": (16384, [50] * 6, 5, True), "bfv": (8192, [60, 40, 40, 60], 3, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="4x4,8x8")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--schemes", default="ckks,bfv")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bsgs_double.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    max_b, max_g = max(b for b, _ in shapes), max(g for _, g in shapes)
    for scheme in args.schemes.split(","):
        n, bits, L, ntt = CONFIGS[scheme]
        q = pkg.capi.coeff_modulus_create(n, bits)
        plan = pkg.Plan(dev, n.bit_length() - 1, q)
        gen = torch.Generator(device=dev).manual_seed(6)
        key = lambda: [bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)]
        baby_keys, giant_keys = [key() for _ in range(max_b)], [key() for _ in range(max_g)]
        baby_el = [pow(3, t + 1, 2 * n) for t in range(max_b)]                       # rotations by 1 .. babies steps
        weights = [[bench.uniform_residues(torch, (), q, n, dev, gen).view(len(q), n) for _ in range(max_b)] for _ in range(max_g)]
        print("# %s; %s N=%d, %s, L=%d; reps %d, rounds %d (median of rounds; min..max)" %
              (torch.cuda.get_device_name(0), scheme.upper(), n, bits, L, args.reps, args.rounds), flush=True)
        for babies, giants in shapes:
            giant_el = [pow(3, babies * (g + 1), 2 * n) for g in range(giants)]      # rotations by babies, 2 babies, ... steps
            for batch in [int(x) for x in args.batches.split(",")]:
                ct = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
                o_single = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)
                o_double = torch.empty_like(o_single)
                bel, bks, gks = baby_el[:babies], baby_keys[:babies], giant_keys[:giants]
                rows = [row[:babies] for row in weights[:giants]]
                form = dict(is_ckks=ntt, is_ntt_form=ntt)

                def single():
                    plan.linear_transform_bsgs(L, ct, bel, bks, giant_el, gks, rows, out=o_single, **form)

                def double():
                    plan.linear_transform_bsgs_double_hoisted(L, ct, bel, bks, giant_el, gks, rows, out=o_double, **form)

                # once per point: each entry against what it must equal
                single()
                inner = plan.apply_galois_weighted_sums(L, ct, bel, bks, rows, **form)
                composed = plan.apply_galois_sum_each(L, inner, giant_el, gks, **form)
                double()
                again = plan.linear_transform_bsgs_double_hoisted(L, ct, bel, bks, giant_el, gks, rows, **form)
                torch.cuda.synchronize()
                if not torch.equal(o_single.view(-1), composed.view(-1)):
                    raise SystemExit("the single-hoisted entry differs from its composition")
                if not torch.equal(o_double.view(-1), again.view(-1)):
                    raise SystemExit("the double-hoisted entry is not reproducible")
                if torch.equal(o_double, o_single):
                    raise SystemExit("the two entries gave the same words: the double-hoisted path did not run")
                del inner, composed, again
                variants = [("single", single), ("double", double)]
                times = {name: [] for name, _ in variants}
                for _ in range(args.rounds):
                    for name, fn in variants:
                        times[name].append(bench.timed(torch, fn, args.reps))
                med = {k: statistics.median(v) for k, v in times.items()}
                rec = {"scheme": scheme, "n": n, "L": L, "babies": babies, "giants": giants, "batch": batch,
                       "ms": {k: round(med[k] * 1e3, 4) for k in med},
                       "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
                       "speedup_double_vs_single": round(med["single"] / med["double"], 4)}
                print(json.dumps(rec), flush=True)
                print("%s babies %d giants %2d batch %3d: single %.3f ms | double %.3f ms (x%.3f)" %
                      (scheme, babies, giants, batch, med["single"] * 1e3, med["double"] * 1e3, rec["speedup_double_vs_single"]), flush=True)
                del ct, o_single, o_double
                torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
