#!/usr/bin/env python3
"""The CKKS bootstrap as one call (troy::BootstrapPlan, Evaluator::bootstrap) against its staged form, and the two kernels between its stages against
the older entries they equal.  Writes profiles/bootstrap_bench.txt (--out).

Full run, through pytroy, CKKS N = 16384: a 60-bit q0, 22 working primes of 50 bits and a 60-bit special prime, D = 2^50, weights at 2^50, K = 256
(the rule K - 1 >= 6.5 sqrt((N + 1) / 12) gives 241), degree 79 with 5 double angles (the interpolated cosine has the frequency of (64, 3) at N = 1024),
the slot plans' default groups 4 + 3 + 3 + 3: 4 + 12 + 4 = 20 levels; the staged form (tests/bootstrap_staged.py: multiply_plain by 1 and i with
rescale_to_next on both sides of two eval_mod calls) takes 22.  Both run on the same chain, context, keys and exhausted ciphertext, alternating round
by round in one process.  SUCH A CHAIN IS NOT A SECURE PARAMETER SET at N = 16384 (about 1220 bits of modulus): the figure is a timing of the
schedule, not of a deployable configuration.  The slot error of both forms against the message is printed beside the times.

Kernel pair, through the C-ABI, CKKS N = 16384, 7 x 50-bit, L = 6, batch 1 and 64:
  split      troyn_ckks_complex_split              against  troyn_add + troyn_sub + troyn_dyadic_product with the transformed monomial
  join       troyn_ckks_complex_join               against  troyn_dyadic_product + troyn_add
The words are compared once per point before timing.  Every timing follows bench.timed: at least 50 ms of warm-up on the timed call itself, then
`reps` back-to-back calls closed by a device synchronise; the median over the rounds is reported with its range.

python tools/bench_bootstrap.py [--reps 10] [--rounds 5] [--full-reps 3] [--batches 1,64] [--out profiles/bootstrap_bench.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
import bench


def kernel_pair(args, emit):
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L = 16384, 14, 6
    q = pkg.capi.coeff_modulus_create(n, [50] * 7)
    plan = pkg.Plan(dev, log_n, q)
    gen = torch.Generator(device=dev).manual_seed(17)
    mono = torch.zeros((1, 1, L, n), dtype=torch.int64, device=dev)
    mono[:, :, :, n // 2] = 1
    mu = plan.ntt(mono, 1, L)
    for batch in [int(x) for x in args.batches.split(",")]:
        a = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        b = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        mus = mu.expand(batch, 2, L, n).contiguous()
        s1, d1, s2, d2, o1, o2, t = (torch.empty_like(a) for _ in range(7))

        def split():
            plan.ckks_complex_split(L, a, b, s=s1, d=d1)

        def split_composed():
            plan.add(a, b, L, out=s2)
            plan.sub(b, a, L, out=t)
            plan.dyadic_product(t, mus, L, out=d2)

        def join():
            plan.ckks_complex_join(L, a, b, out=o1)

        def join_composed():
            plan.dyadic_product(b, mus, L, out=t)
            plan.add(a, t, L, out=o2)

        variants = [("split", split), ("split_composed", split_composed), ("join", join), ("join_composed", join_composed)]
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        if not (torch.equal(s1, s2) and torch.equal(d1, d2) and torch.equal(o1, o2)):
            raise SystemExit("bench_bootstrap.py: a kernel and its composition differ at batch %d" % batch)
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(bench.timed(torch, fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        emit({"kernel_pair": True, "N": n, "L": L, "batch": batch, "us": {k: round(med[k] * 1e6, 2) for k in med},
              "us_min_max": {k: [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)] for k, v in times.items()},
              "split_vs_composed": round(med["split_composed"] / med["split"], 3), "join_vs_composed": round(med["join_composed"] / med["join"], 3)})
        del a, b, mus, s1, d1, s2, d2, o1, o2, t
        torch.cuda.empty_cache()


def full_run(args, emit):
    sys.path.insert(0, os.path.join(ROOT, "troy-nova_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import pytroy
    from bootstrap_staged import Staged, unit_disc
    n, bits = 16384, [60] + [50] * 22 + [60]
    delta, weight, K, degree, r = float(1 << 50), float(1 << 50), 256.0, 79, 5
    p = pytroy.EncryptionParameters(pytroy.SchemeType.CKKS)
    p.set_poly_modulus_degree(n)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(n, bits))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 13)
    ctx.to_device_inplace()
    enc, kg, encryptor = pytroy.CKKSEncoder(ctx), pytroy.KeyGenerator(ctx), pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    rk = kg.create_relin_keys(False)
    ev, dec = pytroy.Evaluator(ctx), pytroy.Decryptor(ctx, kg.secret_key())
    primes = [int(m.value()) for m in pytroy.CoeffModulus.create(n, bits)][:-1]
    plan = pytroy.BootstrapPlan(ctx, enc, delta, K, degree, r, [], [], weight)
    gk = kg.create_galois_keys_from_steps(plan.rotation_steps(), False)
    down, up = plan.coeff_to_slot_plan().layers_per_group(), plan.slot_to_coeff_plan().layers_per_group()
    staged = Staged(pytroy, ctx, enc, kg, primes, delta, K, degree, r, down, up, weight, galois_keys=gk)
    z = unit_disc(np.random.default_rng(41), enc.slot_count())
    fresh = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in z], None, delta))
    exhausted = ev.mod_switch_to_new(fresh, ctx.last_parms_id())
    slots = lambda c: np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c)))
    one = lambda: ev.bootstrap_new(exhausted, plan, rk, gk)
    two = lambda: staged.run(ev, rk, exhausted)
    err = {"bootstrap": float(np.max(np.abs(slots(one()) - z))), "staged": float(np.max(np.abs(slots(two()) - z)))}
    variants = [("bootstrap", one), ("staged", two)]
    times = {k: [] for k, _ in variants}
    for _ in range(args.rounds):
        for k, fn in variants:
            times[k].append(bench.timed(torch, fn, args.full_reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    emit({"full_run": True, "N": n, "data_primes": len(primes), "K": K, "degree": degree, "double_angles": r, "groups": [list(down), list(up)],
          "levels": {"bootstrap": plan.levels(), "staged": staged.levels}, "galois_key_switches": plan.key_switches(), "distinct_keys": len(plan.rotation_steps()),
          "ms": {k: round(med[k] * 1e3, 3) for k in med}, "ms_min_max": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
          "bootstrap_vs_staged": round(med["staged"] / med["bootstrap"], 3), "slot_error": err, "secure_parameter_set": False})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--full-reps", type=int, default=3)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bootstrap.py needs an MI355X: there is no CPU path and no timing without the GPU")
    lines = ["# %s; reps %d (full run %d), rounds %d (median of rounds; min..max).  The full run's chain (N = 16384, 23 data primes) is NOT a secure parameter set." %
             (torch.cuda.get_device_name(0), args.reps, args.full_reps, args.rounds)]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    kernel_pair(args, emit)
    full_run(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
