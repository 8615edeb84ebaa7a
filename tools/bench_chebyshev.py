#!/usr/bin/env python3
"""The Chebyshev step 2 T_a T_b + w T_c as one call against what the library had before it (CKKS N = 16384, 7 x 50-bit, L = 6).

For batch in {1, 64} one run times, in the same process, alternating the variants round by round:
  step       troyn_ckks_multiply_affine_relinearize_rescale   P formed in ONE pass, then the relinearize and rescale drivers
  composed   the bit-identical composition: troyn_dyadic_convolute, troyn_multiply_scalar by alpha, troyn_multiply_scalar of the addend,
             troyn_add, troyn_relinearize, troyn_divide_and_round_q_last_ntt.  The addend travels as three polynomials (the third zero,
             prepared beforehand) so that one troyn_add takes the whole batch; that pads its two passes by a third.
  cheaper    the NON-identical form a caller would write: troyn_ckks_multiply_relinearize_rescale (the fused chain on whole-limb rings)
             and then troyn_scalar_weighted_sums of the product and the addend at the lower level.  It rounds the product before the
             addend joins, so its words differ from the step's.
alpha = 2 and w = 3: one word is the residue under every modulus, which is what troyn_multiply_scalar takes.  `step` and `composed` compute
the same words and the tool checks that once per point before timing.  Every timing follows bench.timed: at least 50 ms of warm-up on the
timed call itself, then `reps` back-to-back calls closed by a device synchronise.

Then, through pytroy on one ciphertext per call (CKKS N = 16384, data primes 60 + 7 x 50 bits and a 60-bit special prime: degree 31 takes 6
levels and eval_mod 7, more than seven primes hold; the 60-bit first prime leaves room for the recombination's scale of about 2^100 on two
limbs), working scale 2^50, the new and the composed path alternating round by round:
  evaluate_chebyshev   degree 31, K = 1, coefficients and slots uniform in [-1, 1]
  eval_mod             degree 15, r = 2, K = 4, slots m + I with |m| <= 2^-7, I in {-3 .. 3}
  composed             the same schedule from the older methods (tests/test_gpu_chebyshev_api.py _composed_chebyshev and its doublings):
                       every T_m by multiply_relinearize_rescale and then linear_combination, the leaves by linear_combination + add_plain
The decryption error of both paths against the float64 reference is printed beside the times.

python tools/bench_chebyshev.py [--reps 10] [--rounds 5] [--batches 1,64]"""
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
        raise SystemExit("bench_chebyshev.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    n, log_n, L = 16384, 14, 6
    q = pkg.capi.coeff_modulus_create(n, [50] * 7)
    plan = pkg.Plan(dev, log_n, q)
    gen = torch.Generator(device=dev).manual_seed(11)
    keys = [bench.uniform_residues(torch, (2,), q, n, dev, gen) for _ in range(L)]
    ALPHA, W = 2, 3
    print("# %s; CKKS N=%d, 7 x 50-bit, L=%d; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), n, L, args.reps, args.rounds), flush=True)
    for batch in [int(x) for x in args.batches.split(",")]:
        a = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        b = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        c3 = torch.zeros((batch, 3, L, n), dtype=torch.int64, device=dev)
        c3[:, :2] = bench.uniform_residues(torch, (batch, 2), q[:L], n, dev, gen)
        c = c3[:, :2].contiguous()
        al, bl, cl = list(a), list(b), list(c)
        alpha, weight = [[ALPHA] * L] * batch, [[W] * L] * batch
        o_step = torch.empty((batch, 2, L - 1, n), dtype=torch.int64, device=dev)
        o_comp, o_mrr = torch.empty_like(o_step), torch.empty_like(o_step)
        o_cheap = torch.empty((1, batch, 2, L - 1, n), dtype=torch.int64, device=dev)
        p3, t3 = torch.empty_like(c3), torch.empty_like(c3)
        r2 = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)

        def step():
            plan.multiply_affine_relinearize_rescale(L, al, bl, cl, [L] * batch, alpha, weight, keys, out=o_step)

        def composed():
            plan.dyadic_convolute(a, 2, b, 2, L, out=p3)
            plan.multiply_scalar(p3, ALPHA, L, out=p3)
            plan.multiply_scalar(c3, W, L, out=t3)
            plan.add(p3, t3, L, out=p3)
            plan.relinearize(L, p3, keys, out=r2)
            plan.divide_and_round_q_last_ntt(L, r2, 2, out=o_comp)

        def cheaper():
            plan.ckks_multiply_relinearize_rescale(L, a, b, keys, out=o_mrr)
            plan.scalar_weighted_sums([o_mrr, c], [L - 1, L], [[[ALPHA] * (L - 1), [W] * (L - 1)]], L - 1, 2, out=o_cheap)

        step(); composed(); cheaper()
        torch.cuda.synchronize()
        if not torch.equal(o_step, o_comp):
            raise SystemExit("bench_chebyshev.py: the step and its composition differ at batch %d" % batch)
        variants = [("step", step), ("composed", composed), ("cheaper", cheaper)]
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(bench.timed(torch, fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"batch": batch, "ms": {k: round(med[k] * 1e3, 4) for k in med},
               "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
               "speedup_step_vs_composed": round(med["composed"] / med["step"], 4),
               "speedup_step_vs_cheaper": round(med["cheaper"] / med["step"], 4),
               "gap_recovered": round((med["composed"] - med["step"]) / (med["composed"] - med["cheaper"]), 4) if med["composed"] != med["cheaper"] else None}
        print(json.dumps(rec), flush=True)
        print("batch %3d: step %.3f ms | composed %.3f ms (x%.3f) | cheaper, non-identical %.3f ms (x%.3f)" %
              (batch, med["step"] * 1e3, med["composed"] * 1e3, rec["speedup_step_vs_composed"], med["cheaper"] * 1e3, rec["speedup_step_vs_cheaper"]), flush=True)
        del a, b, c, c3, p3, t3, r2, o_step, o_comp, o_mrr, o_cheap
        torch.cuda.empty_cache()
    evaluators(args)
    return 0


def evaluators(args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "troy-nova_amd"))
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    from numpy.polynomial import chebyshev as npcheb
    import pytroy
    from test_gpu_chebyshev_api import _composed_chebyshev, _interpolant
    n, bits, work = 16384, [60] + [50] * 7 + [60], float(1 << 50)
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
    rng = np.random.default_rng(31)
    encrypt = lambda v, scale: encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(t) for t in v], None, scale))
    decrypt = lambda c: np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c))).real

    # evaluate_chebyshev, degree 31, K = 1
    values = rng.uniform(-1, 1, enc.slot_count())
    coefficients = rng.uniform(-1, 1, 32).tolist()
    x = encrypt(values, work)
    cases = [("evaluate_chebyshev", "degree 31, K = 1", lambda: ev.evaluate_chebyshev_new(x, coefficients, 1.0, rk),
              lambda: _composed_chebyshev(ev, enc, rk, x, coefficients, 1, primes), npcheb.chebval(values, coefficients))]
    # eval_mod, degree 15, r = 2, K = 4
    K, degree, r = 4, 15, 2
    xs = rng.uniform(-2.0 ** -7, 2.0 ** -7, enc.slot_count()) + rng.integers(-3, 4, enc.slot_count())
    xm = encrypt(xs, work / K)
    coeffs = list(_interpolant(K, degree, r))
    ref = npcheb.chebval(xs / K, coeffs)
    for _ in range(r):
        ref = 2 * ref * ref - 1

    def composed_mod():
        c = _composed_chebyshev(ev, enc, rk, xm, coeffs, K, primes)
        for _ in range(r):
            prod = ev.multiply_relinearize_rescale_new(c, c, rk)
            c = ev.linear_combination_new([prod], [2.0], -1.0, prod.scale())
        c.set_scale(c.scale() * 2 * np.pi)
        return c

    cases.append(("eval_mod", "degree 15, r = 2, K = 4", lambda: ev.eval_mod_new(xm, rk, float(K), degree, r), composed_mod, ref / (2 * np.pi)))
    for name, what, one, composed, want in cases:
        err = {k: float(np.max(np.abs(decrypt(fn()) - want))) for k, fn in ((name, one), ("composed", composed))}
        variants = [(name, one), ("composed", composed)]
        times = {k: [] for k, _ in variants}
        for _ in range(args.rounds):
            for k, fn in variants:
                times[k].append(bench.timed(torch, fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"case": name, "what": what, "ms": {k: round(med[k] * 1e3, 4) for k in med},
               "ms_min_max": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
               "decryption_error": err, "speedup_vs_composed": round(med["composed"] / med[name], 4)}
        print(json.dumps(rec), flush=True)
        print("%s (%s), one ciphertext: %.3f ms | composed %.3f ms (x%.3f); error %.2e | %.2e" %
              (name, what, med[name] * 1e3, med["composed"] * 1e3, rec["speedup_vs_composed"], err[name], err["composed"]), flush=True)


if __name__ == "__main__":
    sys.exit(main())
