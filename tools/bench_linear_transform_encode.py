#!/usr/bin/env python3
"""Matrix diagonals encoded into BSGS weights (troyn_ckks_encode_diagonals) at N = 16384 on seven 50-bit primes, key level (L = 7), n = N/2 = 8192,
16 / 64 / 256 items: item t is diagonal t of a dense random complex matrix rotated back by its giant step t - t mod 16.

One run times, in the same process, alternating round by round:
  diagonals  the entry on the table of diagonals [items][n][2]
  matrix     the entry on the row-major matrix [n][n][2] itself (1 GiB): every lane reads a row of its own, 16 uncoalesced bytes
  gather     the way without the entry: torch.index_select materialises the rotated diagonals [items][N/2][2] on the device (its index tensor is built
             outside the timing), then troyn_ckks_encode_simd
All three give the same words; that is checked once per point before timing.  Every timing follows bench.timed: at least 50 ms of warm-up on the timed
call itself, then `reps` back-to-back calls closed by a device synchronise; the median of the rounds is reported with min..max.

python tools/bench_linear_transform_encode.py [--reps 10] [--rounds 3] [--items 16,64,256]"""
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
    ap.add_argument("--items", default="16,64,256")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_transform_encode.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    N, log_n, L, scale = 16384, 14, 7, 2.0 ** 40
    n = N // 2
    q = pkg.capi.coeff_modulus_create(N, [50] * 7)
    plan = pkg.Plan(dev, log_n, q)
    enc = plan.ckks_handle()
    gen = torch.Generator(device=dev).manual_seed(5)
    matrix = torch.rand((n, n, 2), dtype=torch.float64, device=dev, generator=gen) * 2 - 1
    rows = torch.arange(n, device=dev)
    print("# %s; CKKS N=%d, 7 x 50-bit, L = %d (key level), n = %d, scale 2^40; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), N, L, n, args.reps, args.rounds), flush=True)
    for items in [int(x) for x in args.items.split(",")]:
        k = torch.arange(items, device=dev)
        shift = k - k % 16
        diags = matrix[rows[None, :], (rows[None, :] + k[:, None]) % n].contiguous()                 # [items][n][2]: diag_k[i] = M[i][(i + k) mod n]
        pairs = torch.stack([k, shift], dim=1).to(torch.int32).contiguous()
        lin = (k[:, None] * n + ((rows[None, :] - shift[:, None]) % n)).reshape(-1)               # row of diags.view(-1, 2) for every (item, slot)
        flat = diags.view(-1, 2)
        values = torch.empty((items * n, 2), dtype=torch.float64, device=dev)

        def by_diagonals():
            return enc.encode_diagonals(L, diags, pairs, scale, n)

        def by_matrix():
            return enc.encode_diagonals(L, matrix, pairs, scale, n, matrix=True)

        def by_gather():
            torch.index_select(flat, 0, lin, out=values)
            return enc.encode_simd(L, values.view(items, n, 2), scale)

        want = by_gather()
        if not (torch.equal(by_diagonals(), want) and torch.equal(by_matrix(), want)):
            raise SystemExit("bench_linear_transform_encode.py: the three ways differ at %d items" % items)
        del want
        variants = [("diagonals", by_diagonals), ("matrix", by_matrix), ("gather", by_gather)]
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(bench.timed(torch, fn, args.reps))
        med = {name: statistics.median(v) for name, v in times.items()}
        rec = {"items": items, "us": {name: round(med[name] * 1e6, 1) for name in med},
               "us_min_max": {name: [round(min(v) * 1e6, 1), round(max(v) * 1e6, 1)] for name, v in times.items()},
               "gather_over_diagonals": round(med["gather"] / med["diagonals"], 3), "gather_over_matrix": round(med["gather"] / med["matrix"], 3),
               "residue_MiB": round(8 * L * N * items / 2 ** 20, 1), "saved_MiB": round(2 * 16 * n * items / 2 ** 20, 1)}
        print(json.dumps(rec), flush=True)
        print("items %3d: diagonals %.1f us | matrix %.1f us | gather + encode_simd %.1f us (x%.3f of diagonals, x%.3f of matrix)" %
              (items, med["diagonals"] * 1e6, med["matrix"] * 1e6, med["gather"] * 1e6, rec["gather_over_diagonals"], rec["gather_over_matrix"]), flush=True)
        del diags, pairs, lin, flat, values
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
