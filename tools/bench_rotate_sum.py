#!/usr/bin/env python3
"""Hoisted rotations: many Galois keys applied to one ciphertext with one digit decomposition (CKKS N = 16384, 6 x 50-bit, L = 5).

For terms in {2, 8, 32} and batch in {1, 64} one run times, alternating the variants round by round:
  sum            troyn_apply_galois_sum                      one decomposition, one division by the special prime
  many           troyn_apply_galois_many                     one decomposition, `terms` divisions
  composed_sum   terms x (troyn_apply_galois + copy of the permuted c1 + troyn_switch_key) + (terms - 1) x troyn_add
  composed_many  terms x (troyn_apply_galois + copy of the permuted c1 + troyn_switch_key)
The composed forms only use entries that predate the hoisted ones (what Evaluator::apply_galois does per rotation), with every buffer
allocated beforehand, so they stand for the library without the addition on the same commit.  The results are NOT compared word for word:
the hoisted digits differ from the composed ones by multiples of q_j (include/troyn.h); tests/test_gpu_hoist.py checks the words against the
specification.  Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed
by a device synchronise.

python tools/bench_rotate_sum.py [--reps 10] [--rounds 3] [--terms 2,8,32] [--batches 1,64]"""
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
    ap.add_argument("--terms", default="2,8,32")
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rotate_sum.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L = 16384, 14, 5
    q = pkg.capi.coeff_modulus_create(n, [50] * 6)
    plan = pkg.Plan(dev, log_n, q)
    gen = torch.Generator(device=dev).manual_seed(5)
    max_terms = max(int(x) for x in args.terms.split(","))
    elements = [pow(3, t + 1, 2 * n) for t in range(max_terms)]          # rotations by 1 .. max_terms steps
    keys = [[bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)] for _ in range(max_terms)]
    print("# %s; CKKS N=%d, 6 x 50-bit, L=%d; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L, args.reps, args.rounds), flush=True)
    for terms in [int(x) for x in args.terms.split(",")]:
        for batch in [int(x) for x in args.batches.split(",")]:
            ct = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
            o_sum = torch.empty_like(ct)
            o_many = torch.empty((terms, batch, 2, L, n), dtype=torch.int64, device=dev)
            c_many = torch.empty_like(o_many)
            c_sum, c_tmp = torch.empty_like(ct), torch.empty_like(ct)
            target = torch.empty((batch, L, n), dtype=torch.int64, device=dev)
            el, ks = elements[:terms], keys[:terms]

            def hoisted_sum():
                plan.apply_galois_sum(L, ct, el, ks, out=o_sum)

            def hoisted_many():
                plan.apply_galois_many(L, ct, el, ks, out=o_many)

            def rotate_into(t, dest):
                plan.apply_galois_poly(ct, L, el[t], True, out=dest)
                target.copy_(dest[:, 1])
                plan.switch_key(L, target, ks[t], dest=dest, assign=pkg.ASSIGN_OVERWRITE_EXCEPT_FIRST, is_ckks=True, is_ntt_form=True)

            def composed_sum():
                rotate_into(0, c_sum)
                for t in range(1, terms):
                    rotate_into(t, c_tmp)
                    plan.add(c_sum, c_tmp, L, out=c_sum)

            def composed_many():
                for t in range(terms):
                    rotate_into(t, c_many[t])

            variants = [("sum", hoisted_sum), ("composed_sum", composed_sum), ("many", hoisted_many), ("composed_many", composed_many)]
            times = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    times[name].append(bench.timed(torch, fn, args.reps))
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"terms": terms, "batch": batch,
                   "ms": {k: round(med[k] * 1e3, 4) for k in med},
                   "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
                   "rotations_per_s_sum": round(terms * batch / med["sum"], 1),
                   "speedup_sum_vs_composed": round(med["composed_sum"] / med["sum"], 4),
                   "speedup_many_vs_composed": round(med["composed_many"] / med["many"], 4)}
            print(json.dumps(rec), flush=True)
            print("terms %2d batch %3d: sum %.3f ms | composed %.3f ms (x%.3f) || many %.3f ms | composed %.3f ms (x%.3f)" %
                  (terms, batch, med["sum"] * 1e3, med["composed_sum"] * 1e3, rec["speedup_sum_vs_composed"],
                   med["many"] * 1e3, med["composed_many"] * 1e3, rec["speedup_many_vs_composed"]), flush=True)
            del ct, o_sum, o_many, c_many, c_sum, c_tmp, target
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
