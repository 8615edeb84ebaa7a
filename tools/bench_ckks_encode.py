#!/usr/bin/env python3
"""CKKS encodings and decodings per second: the batched device path (CKKSEncoder.*_batched, troyn_ckks_*) against the per-plaintext methods
of the same build (host FFT and RNS conversion, device NTT).  N = 16384, key-level plaintexts, batches 1 / 16 / 256.

    python tools/bench_ckks_encode.py [--log-n 14] [--bits 60,40,40,40,40,60] [--batches 1,16,256] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "troy-nova_amd"))


def _rate(fn, items, warm_s=0.05, min_s=0.3):
    """items per second of fn(); warmed up for at least warm_s, measured for at least min_s (fn waits for its own results)"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        fn()
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return reps * items / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=14)
    ap.add_argument("--bits", default="60,40,40,40,40,60")
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import pytroy
    n, bits = 1 << args.log_n, [int(b) for b in args.bits.split(",")]
    p = pytroy.EncryptionParameters(pytroy.SchemeType.CKKS)
    p.set_poly_modulus_degree(n)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(n, bits))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 1)
    ctx.to_device_inplace()
    enc = pytroy.CKKSEncoder(ctx)
    pid, scale = ctx.key_parms_id(), 2.0 ** 40
    rng = np.random.default_rng(0)
    rows = []
    for batch in [int(b) for b in args.batches.split(",")]:
        values = [(rng.uniform(-1, 1, n // 2) + 1j * rng.uniform(-1, 1, n // 2)).tolist() for _ in range(batch)]
        plains = enc.encode_complex64_simd_new_batched(values, pid, scale)
        row = {
            "batch": batch,
            "encode_batched_per_s": _rate(lambda: enc.encode_complex64_simd_new_batched(values, pid, scale), batch),
            "encode_single_per_s": _rate(lambda: [enc.encode_complex64_simd_new(v, pid, scale) for v in values[:16]], min(batch, 16)),
            "decode_batched_per_s": _rate(lambda: enc.decode_complex64_simd_batched(plains), batch),
            "decode_single_per_s": _rate(lambda: [enc.decode_complex64_simd_new(q) for q in plains[:16]], min(batch, 16)),
        }
        rows.append(row)
        print("batch %4d  encode %10.1f/s batched  %10.1f/s per-plaintext   decode %10.1f/s batched  %10.1f/s per-plaintext" % (
            batch, row["encode_batched_per_s"], row["encode_single_per_s"], row["decode_batched_per_s"], row["decode_single_per_s"]), flush=True)
    result = {"tool": "bench_ckks_encode", "n": n, "bits": bits, "level": "key", "scale_log2": 40, "rows": rows}
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
