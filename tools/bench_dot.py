#!/usr/bin/env python3
"""Ciphertext dot product with lazy relinearization: SUM_t a_t * b_t, one relinearize, one rescale (CKKS N = 16384, 6 x 50-bit, L = 5).

For terms in {2, 8, 32} and batch = 1024 / terms (1024 products per call at every point) one run times, alternating the variants round by round:
  new         troyn_ckks_multiply_accumulate_relinearize_rescale
  baseline_b  terms x dyadic_convolute + (terms - 1) x add + relinearize + divide_and_round_q_last_ntt   (lazy relinearization by hand)
  baseline_a  terms x ckks_multiply_relinearize_rescale (fused) + (terms - 1) x two-polynomial add       (one key switch per term)
and the accumulate kernel alone against dyadic_convolute at terms = 1, both as achieved bytes/s on the traffic the algorithm needs:
(4 terms + 3) * 8 * N * L * batch bytes.  The baselines only use entries that predate the accumulate, so they stand for the library without it.
Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself (tools/ramp_probe.py: the clocks need 20-25 ms of load), then
`reps` back-to-back calls closed by a device synchronise.  The outputs of new and baseline_b are compared word for word at the timed sizes.

python tools/bench_dot.py [--reps 20] [--rounds 3] [--terms 2,8,32] [--products 1024]"""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--terms", default="2,8,32")
    ap.add_argument("--products", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dot.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L = 16384, 14, 5
    q = pkg.capi.coeff_modulus_create(n, [50] * 6)
    plan = pkg.Plan(dev, log_n, q)
    gen = torch.Generator(device=dev).manual_seed(5)
    keys = [bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)]
    unit = 8 * n * L                    # bytes of one limb-polynomial row set [L][N]
    print("# %s; CKKS N=%d, 6 x 50-bit, L=%d; %d products per call; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L, args.products, args.reps, args.rounds), flush=True)
    ok = True
    for terms in [int(x) for x in args.terms.split(",")]:
        batch = args.products // terms
        a = [bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen) for _ in range(terms)]
        b = [bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen) for _ in range(terms)]
        p0 = torch.empty((batch, 3, L, n), dtype=torch.int64, device=dev)
        p1 = torch.empty_like(p0)
        r2 = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)
        o_new = torch.empty((batch, 2, L - 1, n), dtype=torch.int64, device=dev)
        o_b, o_a, o_t = torch.empty_like(o_new), torch.empty_like(o_new), torch.empty_like(o_new)

        def new():
            plan.ckks_multiply_accumulate_relinearize_rescale(L, a, b, keys, out=o_new)

        def baseline_b():
            plan.dyadic_convolute(a[0], 2, b[0], 2, L, out=p0)
            for t in range(1, terms):
                plan.dyadic_convolute(a[t], 2, b[t], 2, L, out=p1)
                plan.add(p0, p1, L, out=p0)
            plan.relinearize(L, p0, keys, out=r2, is_ckks=True, is_ntt_form=True)
            plan.divide_and_round_q_last_ntt(L, r2, 2, out=o_b)

        def baseline_a():
            plan.ckks_multiply_relinearize_rescale(L, a[0], b[0], keys, out=o_a)
            for t in range(1, terms):
                plan.ckks_multiply_relinearize_rescale(L, a[t], b[t], keys, out=o_t)
                plan.add(o_a, o_t, L - 1, out=o_a)

        def kernel_new():
            plan.dyadic_convolute_accumulate(a, b, L, out=p0)

        def kernel_conv1():
            plan.dyadic_convolute(a[0], 2, b[0], 2, L, out=p1)

        variants = [("new", new), ("baseline_b", baseline_b), ("baseline_a", baseline_a), ("kernel_accumulate", kernel_new), ("kernel_convolute_1", kernel_conv1)]
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(bench.timed(torch, fn, args.reps))
        new(); baseline_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(o_new, o_b))      # (baseline_a rounds per term: another function of the inputs, not compared)
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"terms": terms, "batch": batch, "new_equals_baseline_b": same,
               "ms": {k: round(med[k] * 1e3, 4) for k in med},
               "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
               "products_per_s_new": round(args.products / med["new"], 1),
               "speedup_vs_baseline_b": round(med["baseline_b"] / med["new"], 4),
               "speedup_vs_baseline_a": round(med["baseline_a"] / med["new"], 4),
               "kernel_accumulate_bytes": (4 * terms + 3) * unit * batch,
               "kernel_accumulate_TB_per_s": round((4 * terms + 3) * unit * batch / med["kernel_accumulate"] / 1e12, 4),
               "kernel_convolute_1_TB_per_s": round(7 * unit * batch / med["kernel_convolute_1"] / 1e12, 4),
               "new_faster_than_baseline_b": bool(max(times["new"]) < min(times["baseline_b"]))}
        ok = ok and same and med["new"] < med["baseline_b"]
        print(json.dumps(rec), flush=True)
        print("terms %2d batch %4d: new %.3f ms | baseline_b (by hand, lazy) %.3f ms (x%.3f) | baseline_a (key switch per term) %.3f ms (x%.3f) | "
              "accumulate kernel %.3f ms = %.2f TB/s on (4t+3) rows; dyadic_convolute at one term %.2f TB/s | words equal: %s" %
              (terms, batch, med["new"] * 1e3, med["baseline_b"] * 1e3, rec["speedup_vs_baseline_b"], med["baseline_a"] * 1e3, rec["speedup_vs_baseline_a"],
               med["kernel_accumulate"] * 1e3, rec["kernel_accumulate_TB_per_s"], rec["kernel_convolute_1_TB_per_s"], same), flush=True)
        del a, b, p0, p1, r2, o_new, o_b, o_a, o_t
        torch.cuda.empty_cache()
    print("# new ahead of baseline_b at every point and word-identical to it: %s" % ok, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
