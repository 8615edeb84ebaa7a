#!/usr/bin/env python3
"""Plaintext-weighted hoisted rotations -- the diagonal method of a plaintext matrix times an encrypted vector (CKKS N = 16384, 6 x 50-bit,
L = 5).

For terms in {8, 32}, slots in {1, 4} and batch in {1, 64} one run times, alternating the variants round by round:
  weighted   troyn_apply_galois_weighted_sums            one decomposition, the weights applied before ONE division per slot
  composed   troyn_apply_galois_many, then per slot troyn_multiply_plain_accumulate over its outputs: `terms` divisions, whatever the slots
The composed form only uses entries that predate the weighted one, with every buffer and pointer table prepared beforehand, so it stands for
the library without the addition on the same commit.  The results are NOT compared word for word (the composed form rounds once per term;
include/troyn.h); tests/test_gpu_weighted_hoist.py checks the words against the specification.  Every timing follows bench.timed: at least
50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device synchronise.

python tools/bench_linear_transform.py [--reps 10] [--rounds 3] [--terms 8,32] [--slots 1,4] [--batches 1,64]"""
import argparse
import ctypes as C
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
    ap.add_argument("--terms", default="8,32")
    ap.add_argument("--slots", default="1,4")
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_transform.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    lib = pkg.capi.lib()
    dev = torch.device("cuda", 0)
    n, log_n, L = 16384, 14, 5
    q = pkg.capi.coeff_modulus_create(n, [50] * 6)
    plan = pkg.Plan(dev, log_n, q)
    gen = torch.Generator(device=dev).manual_seed(5)
    ints = lambda s: [int(x) for x in s.split(",")]
    max_terms, max_slots = max(ints(args.terms)), max(ints(args.slots))
    elements = [pow(3, t + 1, 2 * n) for t in range(max_terms)]          # rotations by 1 .. max_terms steps
    keys = [[bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)] for _ in range(max_terms)]
    # key-level weights [K][N]; the composed form multiplies at the data level: the same words, rows 0 .. L-1
    weights = [[bench.uniform_residues(torch, (), q, n, dev, gen).view(len(q), n) for _ in range(max_terms)] for _ in range(max_slots)]
    print("# %s; CKKS N=%d, 6 x 50-bit, L=%d; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L, args.reps, args.rounds), flush=True)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for terms in ints(args.terms):
        for slots in ints(args.slots):
            for batch in ints(args.batches):
                ct = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
                o_weighted = torch.empty((slots, batch, 2, L, n), dtype=torch.int64, device=dev)
                o_composed = torch.empty_like(o_weighted)
                rotated = torch.empty((terms, batch, 2, L, n), dtype=torch.int64, device=dev)
                el, ks = elements[:terms], keys[:terms]
                ws_rows = [row[:terms] for row in weights[:slots]]
                # the pointer tables of the composed form's multiply-accumulate: per slot, (term, item) -> rotated[t][b] * w[s][t] into out[s][b]
                count = terms * batch
                arr = lambda ptrs: (C.c_void_p * count)(*ptrs)
                tables = []
                for s in range(slots):
                    tables.append((arr([rotated[t, b].data_ptr() for t in range(terms) for b in range(batch)]),
                                   arr([ws_rows[s][t].data_ptr() for t in range(terms) for b in range(batch)]),
                                   arr([o_composed[s, b].data_ptr() for t in range(terms) for b in range(batch)])))
                mac_ws = torch.empty(max(int(lib.troyn_multiply_plain_accumulate_workspace_bytes(count)), 16), dtype=torch.uint8, device=dev)

                def weighted():
                    plan.apply_galois_weighted_sums(L, ct, el, ks, ws_rows, out=o_weighted)

                def composed():
                    plan.apply_galois_many(L, ct, el, ks, out=rotated)
                    for cts, pts, dsts in tables:
                        pkg.capi.check(lib.troyn_multiply_plain_accumulate(plan.h, 0, L, 2, cts, pts, dsts, count, 1,
                                                                           C.c_void_p(mac_ws.data_ptr()), mac_ws.numel(), stream()))

                variants = [("weighted", weighted), ("composed", composed)]
                times = {name: [] for name, _ in variants}
                for _ in range(args.rounds):
                    for name, fn in variants:
                        times[name].append(bench.timed(torch, fn, args.reps))
                med = {k: statistics.median(v) for k, v in times.items()}
                rec = {"terms": terms, "slots": slots, "batch": batch,
                       "ms": {k: round(med[k] * 1e3, 4) for k in med},
                       "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
                       "diagonals_per_s_weighted": round(terms * slots * batch / med["weighted"], 1),
                       "speedup_weighted_vs_composed": round(med["composed"] / med["weighted"], 4)}
                print(json.dumps(rec), flush=True)
                print("terms %2d slots %d batch %3d: weighted %.3f ms | composed %.3f ms (x%.3f)" %
                      (terms, slots, batch, med["weighted"] * 1e3, med["composed"] * 1e3, rec["speedup_weighted_vs_composed"]), flush=True)
                del ct, o_weighted, o_composed, rotated, tables, mac_ws
                torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
