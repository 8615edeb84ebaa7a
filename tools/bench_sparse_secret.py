#!/usr/bin/env python3
"""Sparse secrets: the fixed-Hamming-weight sampler against the dense one, and the N = 16384 bootstrap of tools/bench_bootstrap.py with
and without the sparse-secret encapsulation.  Writes profiles/sparse_secret_bench.txt (--out).

Sampler, through the C-ABI: troyn_sample_ternary_sparse (h = 32 and 192) against troyn_sample_ternary, 6 limbs, at N = 16384 and N = 65536 (the largest
ring whose index fits the 16 low bits of a key).  The sparse sampler is ONE workgroup that encrypts N/2 AES blocks and makes eight histogram passes over
its keys; the dense one is N threads with one block each.  This is the cost of an exact weight at key generation, not a target.

Full run, through pytroy, CKKS N = 16384: the chain, context, keys, message and exhausted ciphertext of tools/bench_bootstrap.py (a 60-bit q0, 22 working
primes of 50 bits, a 60-bit special prime, D = 2^50, weights at 2^50, groups 4 + 3 + 3 + 3), in two forms that alternate round by round in one process:
  dense          K = 256, degree 79, 5 double angles, as today (20 levels)
  encapsulated   an ephemeral secret of h = 32 around ModRaise, K = ceil(BootstrapPlan.half_width_for(32)) = 12, degree 39 with 2 double angles (the pair
                 tests/test_sparse_secret_spec.py derives from the float64 specification), plus the two key switches of the encapsulation
SUCH A CHAIN IS NOT A SECURE PARAMETER SET at N = 16384; the weight 32 and the chain are the caller's responsibility.  Slot error, levels, Galois key
switches (the plan's count; the encapsulation adds two ordinary key switches) and time are recorded for each form.
Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then `reps` back-to-back calls closed by a device synchronise; the
median over the rounds is reported with its range.

python tools/bench_sparse_secret.py [--reps 10] [--rounds 5] [--full-reps 3] [--skip-full] [--out profiles/sparse_secret_bench.txt]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
import bench

EPHEMERAL_WEIGHT, ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES = 32, 39, 2


def samplers(args, emit):
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    nmod = 6
    for log_n in (14, 16):
        n = 1 << log_n
        q = pkg.capi.coeff_modulus_create(n, [50] * 7)
        plan = pkg.Plan(dev, log_n, q)
        prng = pkg.Prng(plan, 0xC0FFEE, 0x51)
        variants = [("ternary", lambda: prng.ternary(nmod))] + [("ternary_sparse_h%d" % h, lambda h=h: prng.ternary_sparse(nmod, h)) for h in (32, 192)]
        for name, fn in variants:
            out = fn()
            torch.cuda.synchronize()
            weight = int(torch.count_nonzero(out[0]).item())
            if name != "ternary" and weight != int(name.split("h")[-1]):
                raise SystemExit("bench_sparse_secret.py: %s at N = %d has weight %d" % (name, n, weight))
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(bench.timed(torch, fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        emit({"samplers": True, "N": n, "limbs": nmod, "us": {k: round(med[k] * 1e6, 2) for k in med},
              "us_min_max": {k: [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)] for k, v in times.items()},
              "sparse_h32_vs_dense": round(med["ternary_sparse_h32"] / med["ternary"], 2), "includes": "the engine's allocation of the result and the host call"})


def full_run(args, emit):
    sys.path.insert(0, os.path.join(ROOT, "troy-nova_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import pytroy
    from bootstrap_staged import unit_disc
    n, bits = 16384, [60] + [50] * 22 + [60]
    delta, weight = float(1 << 50), float(1 << 50)
    p = pytroy.EncryptionParameters(pytroy.SchemeType.CKKS)
    p.set_poly_modulus_degree(n)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(n, bits))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 13)
    ctx.to_device_inplace()
    enc, kg, encryptor = pytroy.CKKSEncoder(ctx), pytroy.KeyGenerator(ctx), pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    rk = kg.create_relin_keys(False)
    ev, dec = pytroy.Evaluator(ctx), pytroy.Decryptor(ctx, kg.secret_key())
    k_small = float(math.ceil(pytroy.BootstrapPlan.half_width_for(EPHEMERAL_WEIGHT)))
    dense = pytroy.BootstrapPlan(ctx, enc, delta, 256.0, 79, 5, [], [], weight)
    small = pytroy.BootstrapPlan(ctx, enc, delta, k_small, ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, [], [], weight)
    gk = kg.create_galois_keys_from_steps(sorted(set(dense.rotation_steps()) | set(small.rotation_steps())), False)
    keys = kg.create_sparse_encapsulation_keys(EPHEMERAL_WEIGHT)
    z = unit_disc(np.random.default_rng(41), enc.slot_count())
    fresh = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in z], None, delta))
    exhausted = ev.mod_switch_to_new(fresh, ctx.last_parms_id())
    slots = lambda c: np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c)))
    one = lambda: ev.bootstrap_new(exhausted, dense, rk, gk)
    two = lambda: ev.bootstrap_new(exhausted, small, rk, gk, encapsulation_keys=keys)
    err = {"dense": float(np.max(np.abs(slots(one()) - z))), "encapsulated": float(np.max(np.abs(slots(two()) - z)))}
    variants = [("dense", one), ("encapsulated", two)]
    times = {k: [] for k, _ in variants}
    for _ in range(args.rounds):
        for k, fn in variants:
            times[k].append(bench.timed(torch, fn, args.full_reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    emit({"full_run": True, "N": n, "data_primes": len(bits) - 1, "ephemeral_weight": EPHEMERAL_WEIGHT,
          "K": {"dense": 256.0, "encapsulated": k_small}, "degree": {"dense": 79, "encapsulated": ENCAPSULATED_DEGREE},
          "double_angles": {"dense": 5, "encapsulated": ENCAPSULATED_DOUBLE_ANGLES}, "levels": {"dense": dense.levels(), "encapsulated": small.levels()},
          "galois_key_switches": {"dense": dense.key_switches(), "encapsulated": small.key_switches()}, "encapsulation_key_switches": 2,
          "ms": {k: round(med[k] * 1e3, 3) for k in med}, "ms_min_max": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
          "dense_vs_encapsulated": round(med["dense"] / med["encapsulated"], 3), "slot_error": err, "secure_parameter_set": False})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--full-reps", type=int, default=3)
    ap.add_argument("--skip-full", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_secret_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_secret.py needs an MI355X: there is no CPU path and no timing without the GPU")
    lines = ["# %s; reps %d (full run %d), rounds %d (median of rounds; min..max).  The full run's chain (N = 16384, 23 data primes) is NOT a secure parameter set." %
             (torch.cuda.get_device_name(0), args.reps, args.full_reps, args.rounds)]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    samplers(args, emit)
    if not args.skip_full:
        full_run(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
