#!/usr/bin/env python3
"""CKKS ModRaise (troyn_ckks_mod_raise) at N = 16384 on seven 50-bit primes (six data limbs and the special prime): L_in in {1, 2} -> L_out = 6,
two polynomials, batch 1 and 64, NTT form.

There is no device path for this operation without the entry, so there is no composed form to beat.  One run times, in the same process,
alternating round by round:
  raise      the whole call in NTT form: copy of the low rows, inverse NTT of L_in rows, extension kernel, forward NTT of L_out - L_in rows
  intt+ntt   its unavoidable parts alone, through troyn_ntt: an inverse transform over L_in rows, then a forward one over L_out - L_in rows
  kernel     the extension kernel alone: the same call in coefficient form (no transform; the kernel also writes the L_in low rows), reported as
             effective GB/s over 8 (L_in + L_out) bytes per coefficient
  copy       torch's device copy of the kernel's footprint (as many words read as written), the figure tools/bwtest.py reports per size
Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device
synchronise; the median of the rounds is reported with min..max.

python tools/bench_mod_raise.py [--reps 20] [--rounds 5] [--batches 1,64]"""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mod_raise.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L_out, pc = 16384, 14, 6, 2
    q = pkg.capi.coeff_modulus_create(n, [50] * 7)
    plan = pkg.Plan(dev, log_n, q)
    enc = plan.ckks_handle()
    lib, h = plan.lib, enc.h
    gen = torch.Generator(device=dev).manual_seed(11)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    print("# %s; CKKS N=%d, 7 x 50-bit (L_out = %d), %d polynomials; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L_out, pc, args.reps, args.rounds), flush=True)
    for L_in in (1, 2):
        fresh = L_out - L_in
        for batch in [int(x) for x in args.batches.split(",")]:
            src = bench.uniform_residues(torch, (batch, pc), q[:L_in], n, dev, gen)
            out = torch.empty((batch, pc, L_out, n), dtype=torch.int64, device=dev)
            out_coeff = torch.empty_like(out)
            tmp_in = torch.empty_like(src)
            tmp_new = bench.uniform_residues(torch, (batch, pc), q[L_in:L_out], n, dev, gen)
            tmp_new_out = torch.empty_like(tmp_new)
            nbytes = lib.troyn_ckks_mod_raise_workspace_bytes(h, L_in, L_out, pc, batch, 1)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            coefs = batch * pc * n
            copy_words = coefs * (L_in + L_out) // 2
            ca, cb = torch.empty(copy_words, dtype=torch.int64, device=dev), torch.empty(copy_words, dtype=torch.int64, device=dev)

            def whole():
                pkg.capi.check(lib.troyn_ckks_mod_raise(h, L_in, L_out, 1, vp(src), pc, vp(out), vp(ws), nbytes, batch, st))

            def parts():
                plan.ntt(src, pc, L_in, inverse=True, out=tmp_in)
                plan.ntt(tmp_new, pc, fresh, inverse=False, out=tmp_new_out, table_start=L_in, table_count=fresh)

            def kernel():
                pkg.capi.check(lib.troyn_ckks_mod_raise(h, L_in, L_out, 0, vp(src), pc, vp(out_coeff), None, 0, batch, st))

            def copy():
                cb.copy_(ca)

            # the whole call is NTT o extend o INTT of the parts' own transforms: checked once before timing
            whole(); kernel()
            coeff_in = plan.ntt(src, pc, L_in, inverse=True, out=torch.empty_like(src))
            ext = enc.mod_raise(coeff_in, L_in, L_out, pc, False)
            new_rows = plan.ntt(ext[:, :, L_in:].contiguous(), pc, fresh, inverse=False, out=torch.empty_like(tmp_new), table_start=L_in, table_count=fresh)
            torch.cuda.synchronize()
            if not (torch.equal(out[:, :, :L_in], src) and torch.equal(out[:, :, L_in:], new_rows)):
                raise SystemExit("bench_mod_raise.py: the NTT-form call differs from its composition at L_in %d batch %d" % (L_in, batch))
            variants = [("raise", whole), ("intt+ntt", parts), ("kernel", kernel), ("copy", copy)]
            times = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    times[name].append(bench.timed(torch, fn, args.reps))
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"L_in": L_in, "L_out": L_out, "batch": batch,
                   "us": {k: round(med[k] * 1e6, 2) for k in med},
                   "us_min_max": {k: [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)] for k, v in times.items()},
                   "raise_over_parts": round(med["raise"] / med["intt+ntt"], 3),
                   "kernel_GBps": round(8 * coefs * (L_in + L_out) / med["kernel"] / 1e9, 1),
                   "copy_GBps": round(16 * copy_words / med["copy"] / 1e9, 1),
                   "kernel_MiB": round(8 * coefs * (L_in + L_out) / 2**20, 2)}
            print(json.dumps(rec), flush=True)
            print("L_in %d batch %3d: raise %.1f us | intt+ntt %.1f us (x%.2f) | kernel %.1f us = %.0f GB/s | copy of the same bytes %.0f GB/s" %
                  (L_in, batch, med["raise"] * 1e6, med["intt+ntt"] * 1e6, rec["raise_over_parts"], med["kernel"] * 1e6, rec["kernel_GBps"], rec["copy_GBps"]), flush=True)
            del src, out, out_coeff, tmp_in, tmp_new, tmp_new_out, ws, ca, cb
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
