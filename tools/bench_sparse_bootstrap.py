#!/usr/bin/env python3
"""The sparsely packed CKKS bootstrap (troy::BootstrapPlan with n < N/2, Evaluator::sub_sum) against the fully packed call of the same build.  Writes
profiles/sparse_bootstrap_bench.txt (--out).

Through pytroy, the chain and parameters of tools/bench_bootstrap.py: CKKS N = 16384, a 60-bit q0, 22 working primes of 50 bits and a 60-bit special
prime, D = 2^50, weights at 2^50, K = 256, degree 79 with 5 double angles.  SUCH A CHAIN IS NOT A SECURE PARAMETER SET at N = 16384: the figures time the
schedule, not a deployable configuration.

  bootstrap   one Evaluator::bootstrap at n = 8192 (today's path, the yardstick: default groups 4 + 3 + 3 + 3), at n = 4096 (groups 4 + 4 + 4) and at
              n = 256 (groups 4 + 4), the sparse ones with the plan's default sub_sum_radix.  One message of n values per n, tiled; one set of keys.
  sub_sum     Evaluator::sub_sum alone on the raised ciphertext (top level) at n = 256: radix 2, radix 4 and a single stage.

The variants of a group alternate round by round in one process; every timing follows bench.timed (at least 50 ms of warm-up on the timed call itself,
then `reps` back-to-back calls closed by a device synchronise); the median over the rounds is reported with its range.  The slot error of every bootstrap
against its message and of every sub_sum variant against the radix-2 result is printed beside the times.

python tools/bench_sparse_bootstrap.py [--reps 3] [--rounds 5] [--out profiles/sparse_bootstrap_bench.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: F401  (bench imports it)
import bench

N, BITS = 16384, [60] + [50] * 22 + [60]
DELTA, WEIGHT, K, DEGREE, DOUBLE_ANGLES = float(1 << 50), float(1 << 50), 256.0, 79, 5
GROUPS = {8192: [], 4096: [4, 4, 4], 256: [4, 4]}
SUB_SUM_N = 256


def run(args, emit):
    sys.path.insert(0, os.path.join(ROOT, "troy-nova_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import pytroy
    from bootstrap_staged import unit_disc
    p = pytroy.EncryptionParameters(pytroy.SchemeType.CKKS)
    p.set_poly_modulus_degree(N)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(N, BITS))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 13)
    ctx.to_device_inplace()
    enc, kg, encryptor = pytroy.CKKSEncoder(ctx), pytroy.KeyGenerator(ctx), pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    rk = kg.create_relin_keys(False)
    ev, dec = pytroy.Evaluator(ctx), pytroy.Decryptor(ctx, kg.secret_key())
    slot_count = enc.slot_count()
    plans = {n: pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, g, g, WEIGHT, n=n) for n, g in GROUPS.items()}
    radices = {"radix2": 2, "radix4": 4, "single": slot_count // SUB_SUM_N}
    steps = set()
    for plan in plans.values():
        steps |= set(plan.rotation_steps())
    for radix in radices.values():
        steps |= set(pytroy.Evaluator.sub_sum_steps(slot_count, SUB_SUM_N, radix))
    gk = kg.create_galois_keys_from_steps(sorted(steps), False)
    slots = lambda c: np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c)))      # noqa: E731
    rng = np.random.default_rng(41)
    messages, exhausted = {}, {}
    for n in GROUPS:
        messages[n] = np.tile(unit_disc(rng, n), slot_count // n)
        fresh = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in messages[n]], None, DELTA))
        exhausted[n] = ev.mod_switch_to_new(fresh, ctx.last_parms_id())

    # the bootstrap at every n
    calls = {n: (lambda n=n: ev.bootstrap_new(exhausted[n], plans[n], rk, gk)) for n in GROUPS}
    err = {n: float(np.max(np.abs(slots(calls[n]()) - messages[n]))) for n in GROUPS}
    times = {n: [] for n in GROUPS}
    for _ in range(args.rounds):
        for n in GROUPS:
            times[n].append(bench.timed(torch, calls[n], args.reps))
    med = {n: statistics.median(v) for n, v in times.items()}
    full = plans[slot_count]
    for n in GROUPS:
        plan = plans[n]
        emit({"bootstrap": True, "N": N, "n": n, "groups": [list(plan.coeff_to_slot_plan().layers_per_group()), list(plan.slot_to_coeff_plan().layers_per_group())],
              "levels": plan.levels(), "galois_key_switches": plan.key_switches(), "sub_sum_key_switches": plan.sub_sum_key_switches(), "sub_sum_radix": plan.sub_sum_radix(),
              "distinct_keys": len(plan.rotation_steps()), "ms": round(med[n] * 1e3, 3), "ms_min_max": [round(min(times[n]) * 1e3, 3), round(max(times[n]) * 1e3, 3)],
              "vs_full": round(med[slot_count] / med[n], 3), "levels_vs_full": full.levels() - plan.levels(), "slot_error": err[n], "secure_parameter_set": False})

    # sub_sum alone, on the raised ciphertext
    raised = ev.mod_raise_new(exhausted[SUB_SUM_N])
    subs = {k: (lambda r=r: ev.sub_sum_new(raised, SUB_SUM_N, gk, r)) for k, r in radices.items()}
    base = slots(subs["radix2"]())
    diff = {k: float(np.max(np.abs(slots(fn()) - base)) / max(float(np.max(np.abs(base))), 1e-300)) for k, fn in subs.items()}
    times = {k: [] for k in subs}
    for _ in range(args.rounds):
        for k, fn in subs.items():
            times[k].append(bench.timed(torch, fn, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    emit({"sub_sum": True, "N": N, "n": SUB_SUM_N, "limbs": raised.coeff_modulus_size(),
          "key_switches": {k: len([x for st in pytroy.Evaluator.sub_sum_stages(slot_count, SUB_SUM_N, r) for x in st]) for k, r in radices.items()},
          "stages": {k: len(pytroy.Evaluator.sub_sum_stages(slot_count, SUB_SUM_N, r)) for k, r in radices.items()},
          "ms": {k: round(med[k] * 1e3, 3) for k in med}, "ms_min_max": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
          "relative_difference_from_radix2": diff, "fastest": min(med, key=med.get)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_bootstrap_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_bootstrap.py needs an MI355X: there is no CPU path and no timing without the GPU")
    lines = ["# %s; reps %d, rounds %d (median of rounds; min..max).  The chain (N = 16384, 23 data primes) is NOT a secure parameter set." %
             (torch.cuda.get_device_name(0), args.reps, args.rounds)]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    run(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
