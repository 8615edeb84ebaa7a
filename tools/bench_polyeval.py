#!/usr/bin/env python3
"""Scalar-weighted sums of ciphertexts -- the leaf step of a polynomial evaluation, and the evaluation itself (CKKS N = 16384, 6 x 50-bit, L = 5).

For (terms, slots) in {(3,2), (7,8)} and batch in {1, 64} one run times, in the same process, alternating the variants round by round:
  sums       troyn_scalar_weighted_sums          every input read once per tile of slots, every output written once
  composed   per slot and term troyn_multiply_scalar into a temporary and troyn_add into the slot: about 5 ciphertext passes per term
The composed form only uses entries that predate the one-call entry, with every buffer prepared beforehand, so it stands for the library
without the addition on the same commit.  Its scalars are small integers (one word is the residue under every modulus, which is what
troyn_multiply_scalar takes); both variants compute the same words and the tool checks that once per point before timing.
Then, on the same chain through pytroy, one ciphertext per call:
  evaluate_polynomial   Evaluator::evaluate_polynomial of degree 7
  composed              the same schedule from the older Evaluator methods (tests/test_gpu_polyeval_api.py _composed): leaves by
                        encode_float64_single + multiply_plain + add, recombination per giant by multiply_relinearize_rescale + add
Degree 7 takes 4 of the chain's 5 levels, so the scale is 2^49 (just below the primes: the powers sit at 2^48 .. 2^46, the products at the
two-limb recombination level at 2^99 < 100 bits) and the coefficients lie in [-1/16, 1/16], which keeps the result decodable under q_0.
Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device
synchronise.

python tools/bench_polyeval.py [--reps 10] [--rounds 3] [--shapes 3x2,7x8] [--batches 1,64]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry
import bench


def tile(slots):
    """the slot tile of a launch (csrc/troyn.hip ssum_tile)"""
    return 8 if slots > 4 else 4 if slots > 2 else 2 if slots > 1 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="3x2,7x8")
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_polyeval.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L = 16384, 14, 5
    q = pkg.capi.coeff_modulus_create(n, [50] * 6)
    plan = pkg.Plan(dev, log_n, q)
    gen = torch.Generator(device=dev).manual_seed(7)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    print("# %s; CKKS N=%d, 6 x 50-bit, L=%d; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L, args.reps, args.rounds), flush=True)
    for terms, slots in shapes:
        weights = [[(1 << 40) + 977 * s + 31 * t + 5 for t in range(terms)] for s in range(slots)]      # below every modulus
        scalars = [[[w] * L for w in row] for row in weights]
        for batch in [int(x) for x in args.batches.split(",")]:
            ins = [bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen) for _ in range(terms)]
            o_sums = torch.empty((slots, batch, 2, L, n), dtype=torch.int64, device=dev)
            o_composed = torch.empty_like(o_sums)
            tmp = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)

            def sums():
                plan.scalar_weighted_sums(ins, [L] * terms, scalars, L, 2, out=o_sums)

            def composed():
                for s in range(slots):
                    plan.multiply_scalar(ins[0], weights[s][0], L, out=o_composed[s])
                    for t in range(1, terms):
                        plan.multiply_scalar(ins[t], weights[s][t], L, out=tmp)
                        plan.add(o_composed[s], tmp, L, out=o_composed[s])

            sums(); composed()
            torch.cuda.synchronize()
            if not torch.equal(o_sums, o_composed):
                raise SystemExit("bench_polyeval.py: the two variants differ at terms %d slots %d batch %d" % (terms, slots, batch))
            variants = [("sums", sums), ("composed", composed)]
            times = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    times[name].append(bench.timed(torch, fn, args.reps))
            med = {k: statistics.median(v) for k, v in times.items()}
            words = batch * 2 * L * n
            rec = {"terms": terms, "slots": slots, "batch": batch,
                   "ms": {k: round(med[k] * 1e3, 4) for k in med},
                   "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
                   "GBps_sums": round(8 * words * (terms * -(-slots // tile(slots)) + slots) / med["sums"] / 1e9, 1),
                   "speedup_sums_vs_composed": round(med["composed"] / med["sums"], 4)}
            print(json.dumps(rec), flush=True)
            print("terms %d slots %d batch %3d: sums %.3f ms | composed %.3f ms (x%.3f)" %
                  (terms, slots, batch, med["sums"] * 1e3, med["composed"] * 1e3, rec["speedup_sums_vs_composed"]), flush=True)
            del ins, o_sums, o_composed, tmp
            torch.cuda.empty_cache()
    polyeval(args)
    return 0


def polyeval(args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "troy-nova_amd"))
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import pytroy
    from test_gpu_polyeval_api import _composed
    n, bits, scale = 16384, [50] * 6, float(1 << 49)
    p = pytroy.EncryptionParameters(pytroy.SchemeType.CKKS)
    p.set_poly_modulus_degree(n)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(n, bits))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 11)
    ctx.to_device_inplace()
    enc, kg, encryptor = pytroy.CKKSEncoder(ctx), pytroy.KeyGenerator(ctx), pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    rk = kg.create_relin_keys(False)
    ev, dec = pytroy.Evaluator(ctx), pytroy.Decryptor(ctx, kg.secret_key())
    primes = [int(m.value()) for m in pytroy.CoeffModulus.create(n, bits)][:-1]
    rng = np.random.default_rng(7)
    values = rng.uniform(-1, 1, enc.slot_count())
    x = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in values], None, scale))
    coefficients = rng.uniform(-1 / 16, 1 / 16, 8).tolist()
    one = lambda: ev.evaluate_polynomial_new(x, coefficients, rk)
    composed = lambda: _composed(ev, enc, rk, x, coefficients, primes)
    want = np.polyval(coefficients[::-1], values)
    err = {name: float(np.max(np.abs(np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(fn()))).real - want))) for name, fn in (("evaluate_polynomial", one), ("composed", composed))}
    variants = [("evaluate_polynomial", one), ("composed", composed)]
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            times[name].append(bench.timed(torch, fn, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    rec = {"degree": 7, "scale_log2": 49, "ms": {k: round(med[k] * 1e3, 4) for k in med},
           "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
           "decryption_error": err, "speedup_vs_composed": round(med["composed"] / med["evaluate_polynomial"], 4)}
    print(json.dumps(rec), flush=True)
    print("degree 7, one ciphertext, scale 2^49: evaluate_polynomial %.3f ms | composed %.3f ms (x%.3f)" %
          (med["evaluate_polynomial"] * 1e3, med["composed"] * 1e3, rec["speedup_vs_composed"]), flush=True)


if __name__ == "__main__":
    sys.exit(main())
