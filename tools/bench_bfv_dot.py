#!/usr/bin/env python3
"""BFV inner product: SUM_t a_t * b_t with one scale-down and one key switch (troyn_bfv_multiply_accumulate_relinearize).

Two shapes: BASELINE config 4 (N = 32768, eleven 50-bit primes, L = 10) and N = 8192 {40,40,40} (L = 2).  For terms in {2, 8, 32} and
batch = products / terms one run times, alternating the variants round by round:
  new          troyn_bfv_multiply_accumulate_relinearize
  composition  terms x troyn_bfv_multiply + (terms - 1) x troyn_add + one troyn_relinearize    (the same sum from the entries that predate it)
  per_pair     terms x (troyn_bfv_multiply + troyn_relinearize) folded with troyn_add           (what users write today)
Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device
synchronise; the figure per variant is the median of `rounds` such timings and the spread (min..max) is printed beside it.  `new` and
`composition` round differently (one floor against one per term), so their words are not compared here (tests/test_gpu_bfv_dot.py checks `new`
against the specification).

python tools/bench_bfv_dot.py [--reps 10] [--rounds 3] [--terms 2,8,32]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry
import bench

SHAPES = [("config4", 32768, [50] * 11, 10, 64), ("n8192", 8192, [40, 40, 40], 2, 256)]      # name, N, chain, L, products per call
PLAIN_MODULUS = 786433


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--terms", default="2,8,32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bfv_dot.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    ok = True
    for name, n, bits, L, products in SHAPES:
        q = pkg.capi.coeff_modulus_create(n, bits)
        plan = pkg.Plan(dev, n.bit_length() - 1, q)
        behz = pkg.Behz(plan, L, PLAIN_MODULUS)
        gen = torch.Generator(device=dev).manual_seed(5)
        keys = [bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)]
        print("# %s; BFV %s N=%d, %s, L=%d, t=%d; %d products per call; reps %d, rounds %d (median of rounds; min..max)" %
              (torch.cuda.get_device_name(0), name, n, bits, L, PLAIN_MODULUS, products, args.reps, args.rounds), flush=True)
        for terms in [int(x) for x in args.terms.split(",")]:
            batch = max(1, products // terms)
            a = [bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen) for _ in range(terms)]
            b = [bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen) for _ in range(terms)]
            p0 = torch.empty((batch, 3, L, n), dtype=torch.int64, device=dev)
            p1 = torch.empty_like(p0)
            o_new = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)
            o_c, o_p, o_t = torch.empty_like(o_new), torch.empty_like(o_new), torch.empty_like(o_new)

            def new():
                behz.bfv_multiply_accumulate_relinearize(a, b, keys, out=o_new)

            def composition():
                behz.multiply(a[0], 2, b[0], 2, out=p0)
                for t in range(1, terms):
                    behz.multiply(a[t], 2, b[t], 2, out=p1)
                    plan.add(p0, p1, L, out=p0)
                plan.relinearize(L, p0, keys, out=o_c, is_ckks=False, is_ntt_form=False)

            def per_pair():
                behz.multiply(a[0], 2, b[0], 2, out=p0)
                plan.relinearize(L, p0, keys, out=o_p, is_ckks=False, is_ntt_form=False)
                for t in range(1, terms):
                    behz.multiply(a[t], 2, b[t], 2, out=p1)
                    plan.relinearize(L, p1, keys, out=o_t, is_ckks=False, is_ntt_form=False)
                    plan.add(o_p, o_t, L, out=o_p)

            variants = [("new", new), ("composition", composition), ("per_pair", per_pair)]
            times = {v: [] for v, _ in variants}
            for _ in range(args.rounds):
                for v, fn in variants:
                    times[v].append(bench.timed(torch, fn, args.reps))
            med = {k: statistics.median(v) for k, v in times.items()}
            ahead = bool(max(times["new"]) < min(times["composition"]))
            rec = {"shape": name, "n": n, "L": L, "terms": terms, "batch": batch,
                   "ms": {k: round(med[k] * 1e3, 4) for k in med},
                   "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
                   "speedup_vs_composition": round(med["composition"] / med["new"], 4),
                   "speedup_vs_per_pair": round(med["per_pair"] / med["new"], 4),
                   "new_ahead_of_composition_beyond_spread": ahead}
            ok = ok and ahead
            print(json.dumps(rec), flush=True)
            print("%s terms %2d batch %3d: new %.3f ms (%.3f..%.3f) | composition %.3f ms (%.3f..%.3f) x%.3f | per pair %.3f ms (%.3f..%.3f) x%.3f" %
                  (name, terms, batch, med["new"] * 1e3, min(times["new"]) * 1e3, max(times["new"]) * 1e3,
                   med["composition"] * 1e3, min(times["composition"]) * 1e3, max(times["composition"]) * 1e3, rec["speedup_vs_composition"],
                   med["per_pair"] * 1e3, min(times["per_pair"]) * 1e3, max(times["per_pair"]) * 1e3, rec["speedup_vs_per_pair"]), flush=True)
            del a, b, p0, p1, o_new, o_c, o_p, o_t
            torch.cuda.empty_cache()
    print("# new ahead of the composition beyond the run-to-run spread at every point: %s" % ok, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
