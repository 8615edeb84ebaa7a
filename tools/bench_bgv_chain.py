#!/usr/bin/env python3
"""BGV multiply -> relinearize -> mod-switch as one call against the three calls it equals (BGV N = 16384, four 50-bit primes: L = 3 data
limbs and the special prime, t = 65537).

For batch in {1, 64} one run times, in the same process, alternating the variants round by round:
  fused       troyn_bgv_multiply_relinearize_mod_switch        one forward transform of 2 (L-1) rows per item, c_0, c_1 and the relinearized
                                                               ciphertext never written
  composed    troyn_dyadic_convolute, troyn_bgv_relinearize, troyn_bgv_mod_t_and_divide_q_last_ntt into preallocated buffers
  composed_2  the same three calls timed a second time: the distance between the two composed figures is the run's own noise
The variants compute the same words and the tool checks that once per point before timing.  Every timing follows bench.timed: at least
50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device synchronise; the figure of a variant is the
median of `rounds` such timings.

python tools/bench_bgv_chain.py [--reps 10] [--rounds 5] [--batches 1,64]"""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bgv_chain.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, K, t = 16384, 14, 4, 65537
    L = K - 1
    q = pkg.capi.coeff_modulus_create(n, [50] * K)
    plan = pkg.Plan(dev, log_n, q)
    key_level, level = pkg.Bgv(plan, K, t), pkg.Bgv(plan, L, t)
    gen = torch.Generator(device=dev).manual_seed(11)
    keys = [bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)]
    print("# %s; BGV N=%d, %d x 50-bit, L=%d, t=%d; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, K, L, t, args.reps, args.rounds), flush=True)
    for batch in [int(x) for x in args.batches.split(",")]:
        a = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        b = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        o_fused = torch.empty((batch, 2, L - 1, n), dtype=torch.int64, device=dev)
        o_comp = torch.empty_like(o_fused)
        p3 = torch.empty((batch, 3, L, n), dtype=torch.int64, device=dev)
        r2 = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)

        def fused():
            key_level.multiply_relinearize_mod_switch(level, a, b, keys, out=o_fused)

        def composed():
            plan.dyadic_convolute(a, 2, b, 2, L, out=p3)
            key_level.relinearize(L, p3, keys, out=r2)
            level.mod_t_and_divide_q_last_ntt(r2, 2, out=o_comp)

        fused(); composed()
        torch.cuda.synchronize()
        if not torch.equal(o_fused, o_comp):
            raise SystemExit("bench_bgv_chain.py: the fused entry and the three calls differ at batch %d" % batch)
        variants = [("fused", fused), ("composed", composed), ("composed_2", composed)]
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(bench.timed(torch, fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = abs(med["composed"] - med["composed_2"])
        gain = min(med["composed"], med["composed_2"]) - med["fused"]
        rec = {"batch": batch, "ms": {k: round(med[k] * 1e3, 4) for k in med},
               "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
               "composed_spread_ms": round(spread * 1e3, 4), "fused_gain_ms": round(gain * 1e3, 4),
               "speedup_fused_vs_composed": round(min(med["composed"], med["composed_2"]) / med["fused"], 4),
               "fused_ahead_by_more_than_spread": bool(gain > spread)}
        print(json.dumps(rec), flush=True)
        print("batch %3d: fused %.3f ms | composed %.3f ms, again %.3f ms (spread %.3f ms) | x%.3f" %
              (batch, med["fused"] * 1e3, med["composed"] * 1e3, med["composed_2"] * 1e3, spread * 1e3, rec["speedup_fused_vs_composed"]), flush=True)
        del a, b, p3, r2, o_fused, o_comp
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
