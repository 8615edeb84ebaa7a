#!/usr/bin/env python3
"""Hoisted BGV rotations and the BGV baby-step/giant-step linear transform (BGV N = 16384, 4 x 50-bit, L = 3, t = 65537).

For batch in {1, 64} one run times, in the same process, alternating the variants round by round:
  sum         troyn_bgv_apply_galois_sum over 8 rotations: one decomposition, ONE division
  composed    8 x (troyn_apply_galois + troyn_bgv_switch_key) and the additions: 8 decompositions, 8 divisions
  composed2   the same composed form timed a second time, so that its own spread is visible
  bsgs        troyn_bgv_linear_transform_bsgs, 4 babies x 4 giants
  bsgs_composed / bsgs_composed2   per baby step apply_galois + troyn_bgv_switch_key, the plaintext products and additions per giant step,
              then per giant step apply_galois + troyn_bgv_switch_key and the additions
The composed forms only use entries that predate the hoisted BGV entries, with every buffer prepared beforehand.  The results are NOT
compared word for word (include/troyn.h: the hoisted digits differ and a sum is divided once); tests/test_gpu_bgv_hoist.py checks the words
against the specification.  Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back
calls closed by a device synchronise.

--tails CALLS is the workload of a kernel trace instead of a timing: per batch, CALLS x (troyn_bgv_switch_key on `batch` targets, then
troyn_bgv_apply_galois_sum of ONE term on `batch` items).  Both divide batch * 2 * L rows, the first with bgv_delta_kernel + bgv_finish_kernel,
the second with bgv_hoist_delta_kernel + bgv_hoist_finish_kernel, so the per-kernel averages of
  rocprofv3 --kernel-trace --stats -f csv -- python tools/bench_bgv_hoist.py --tails 200 --batches 64
compare the two tails on the same row count (nothing else traced alongside).

python tools/bench_bgv_hoist.py [--reps 10] [--rounds 3] [--batches 1,64] [--tails CALLS]"""
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
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--tails", type=int, default=0, help="run the two tails CALLS times each for a kernel trace; no timing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bgv_hoist.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L, t = 16384, 14, 3, 65537
    rotations, babies, giants = 8, 4, 4
    q = pkg.capi.coeff_modulus_create(n, [50] * 4)
    K = len(q)
    plan = pkg.Plan(dev, log_n, q)
    bgv = pkg.Bgv(plan, K, t)
    gen = torch.Generator(device=dev).manual_seed(6)
    key = lambda: [bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)]
    keys = [key() for _ in range(rotations)]
    elements = [pow(3, u + 1, 2 * n) for u in range(rotations)]
    baby_el, giant_el = elements[:babies], [pow(3, babies * (g + 1), 2 * n) for g in range(giants)]
    weights = [[bench.uniform_residues(torch, (), q, n, dev, gen).view(K, n) for _ in range(babies)] for _ in range(giants)]
    print("# %s; BGV N=%d, 4 x 50-bit, L=%d, t=%d; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L, t, args.reps, args.rounds), flush=True)
    for batch in [int(x) for x in args.batches.split(",")]:
        ct = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        shape = (batch, 2, L, n)
        o_sum, o_comp, rotated, acc, prod = (torch.empty(shape, dtype=torch.int64, device=dev) for _ in range(5))
        o_bsgs, o_bcomp = torch.empty_like(o_sum), torch.empty_like(o_sum)
        baby_rot = torch.empty((babies,) + shape, dtype=torch.int64, device=dev)
        target = torch.empty((batch, L, n), dtype=torch.int64, device=dev)

        def rotate(src, element, ks, dest):
            plan.apply_galois_poly(src, L, element, True, out=dest)
            target.copy_(dest[:, 1])
            bgv.switch_key(L, target, ks, dest=dest, assign=pkg.ASSIGN_OVERWRITE_EXCEPT_FIRST)

        def hoisted_sum():
            bgv.apply_galois_sum(L, ct, elements, keys, out=o_sum)

        def composed():
            for u in range(rotations):
                rotate(ct, elements[u], keys[u], o_comp if u == 0 else rotated)
                if u:
                    plan.add(o_comp, rotated, L, out=o_comp)

        def bsgs():
            bgv.linear_transform_bsgs(L, ct, baby_el, keys[:babies], giant_el, keys[babies:babies + giants], weights, out=o_bsgs)

        def bsgs_composed():
            for b in range(babies):
                rotate(ct, baby_el[b], keys[b], baby_rot[b])
            for g in range(giants):
                for b in range(babies):
                    # the plaintext product of both components with the weight's data rows (rows 0 .. L-1 of the key-level layout)
                    plan.dyadic_broadcast_product(baby_rot[b], 2, weights[g][b], L, shared_plain=True, out=acc if b == 0 else prod)
                    if b:
                        plan.add(acc, prod, L, out=acc)
                rotate(acc, giant_el[g], keys[babies + g], o_bcomp if g == 0 else rotated)
                if g:
                    plan.add(o_bcomp, rotated, L, out=o_bcomp)

        if args.tails:
            target.copy_(ct[:, 1])
            for i in range(args.tails + 20):      # (20 warm-up rounds lead the trace; they are 9 % of the calls behind an average)
                bgv.switch_key(L, target, keys[0], dest=o_comp, assign=pkg.ASSIGN_OVERWRITE)
                bgv.apply_galois_sum(L, ct, elements[:1], keys[:1], out=o_sum)
            torch.cuda.synchronize()
            print("tails: batch %d, %d rows per tail, %d calls of each entry" % (batch, batch * 2 * L, args.tails + 20), flush=True)
            continue
        variants = [("sum", hoisted_sum), ("composed", composed), ("composed2", composed),
                    ("bsgs", bsgs), ("bsgs_composed", bsgs_composed), ("bsgs_composed2", bsgs_composed)]
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(bench.timed(torch, fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"batch": batch, "rotations": rotations, "babies": babies, "giants": giants,
               "ms": {k: round(med[k] * 1e3, 4) for k in med},
               "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
               "speedup_sum_vs_composed": round(med["composed"] / med["sum"], 4),
               "speedup_bsgs_vs_composed": round(med["bsgs_composed"] / med["bsgs"], 4)}
        print(json.dumps(rec), flush=True)
        print("batch %3d: sum %.3f ms | composed %.3f / %.3f ms (x%.3f) || bsgs %.3f ms | composed %.3f / %.3f ms (x%.3f)" %
              (batch, med["sum"] * 1e3, med["composed"] * 1e3, med["composed2"] * 1e3, rec["speedup_sum_vs_composed"],
               med["bsgs"] * 1e3, med["bsgs_composed"] * 1e3, med["bsgs_composed2"] * 1e3, rec["speedup_bsgs_vs_composed"]), flush=True)
        del ct, o_sum, o_comp, rotated, acc, prod, o_bsgs, o_bcomp, baby_rot, target
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
