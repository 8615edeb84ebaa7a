#!/usr/bin/env python3
"""CoeffToSlot on the factored special DFT (troy::CoeffToSlotPlan, Evaluator::coeff_to_slot) at N = 16384, n = 8192, 13 layers.

1. Evaluator::coeff_to_slot through pytroy for groups of 1, 3 and 4 layers ([1] * 13, [3, 3, 3, 2, 2], [4, 3, 3, 3]): the time of one evaluation with
   the number of key switches (rotations and the conjugation) and of levels it costs.  40-bit primes, one per group plus the last level and the key
   prime, ciphertext scale 2^30, weight scale 2^40.
2. The weights of one group (layers [5, 9): 31 diagonals): troyn_ckks_dft_factor_diagonals + troyn_ckks_encode_diagonals, everything on the device,
   against the same table built in numpy (tests/dft_factors_spec.py), uploaded, and encoded by the same entry.  The words are compared first.

Every device timing follows bench.timed: warm-up on the timed call itself, then `reps` back-to-back calls closed by a device synchronise; the median of
the rounds is reported with min..max.  The numpy way is host work: wall time per call, synchronised.

python tools/bench_coeff_to_slot.py [--reps 5] [--rounds 3] > profiles/coeff_to_slot_bench.txt"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "troy-nova_amd"))
import __graft_entry__ as entry
import bench
import dft_factors_spec as S

N, LOG_N, M = 16384, 14, 13


def evaluation(pytroy, groups, reps, rounds):
    p = pytroy.EncryptionParameters(pytroy.SchemeType.CKKS)
    p.set_poly_modulus_degree(N)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(N, [40] * (len(groups) + 2)))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 99)
    ctx.to_device_inplace()
    enc, kg = pytroy.CKKSEncoder(ctx), pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    ev = pytroy.Evaluator(ctx)
    rng = np.random.default_rng(1)
    z = (rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)) / np.sqrt(2)
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z.tolist(), None, 2.0 ** 30))
    t0 = time.perf_counter()
    plan = pytroy.CoeffToSlotPlan(ctx, enc, c.parms_id(), 2.0 ** 40, groups)
    torch.cuda.synchronize()
    build = time.perf_counter() - t0
    gk = kg.create_galois_keys_from_steps(sorted(set(plan.rotation_steps()) | {0}), False)
    times = [bench.timed(torch, lambda: ev.coeff_to_slot_new(c, plan, gk), reps) for _ in range(rounds)]
    rec = {"groups": groups, "levels": plan.levels(), "key_switches": plan.rotations(), "distinct_keys": len(plan.rotation_steps()) + 1,
           "ms": round(statistics.median(times) * 1e3, 3), "ms_min_max": [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)], "plan_build_ms": round(build * 1e3, 1)}
    print(json.dumps(rec), flush=True)
    del gk, plan, c
    pytroy.MemoryPool.destroy_global_pool()


def weights(pkg, dev, reps, rounds):
    L, scale, n, first, count = 7, 2.0 ** 40, N // 2, 5, 4
    plan = pkg.Plan(dev, LOG_N, pkg.capi.coeff_modulus_create(N, [50] * 7))
    enc = plan.ckks_handle()
    tables = enc.tables()
    nd = S.diagonal_count(n, first, count)
    a = torch.arange(nd, dtype=torch.int32, device=dev)
    pairs = torch.stack([a, (a * 257) % n], dim=1).to(torch.int32).contiguous()

    def on_device():
        return enc.encode_diagonals(L, enc.dft_factor_diagonals(first, count, inverse=True, col_mask=1, constant=0.9), pairs, scale, n)

    def kernel_only():
        return enc.dft_factor_diagonals(first, count, inverse=True, col_mask=1, constant=0.9)

    def by_numpy():
        table = S.table(tables, first, count, inverse=True, col_mask=1, constant=0.9)
        return enc.encode_diagonals(L, torch.from_numpy(table).to(dev), pairs, scale, n)

    if not torch.equal(on_device(), by_numpy()):
        raise SystemExit("bench_coeff_to_slot.py: the device table and the numpy table encode to different words")
    dev_t = [bench.timed(torch, on_device, reps * 4) for _ in range(rounds)]
    ker_t = [bench.timed(torch, kernel_only, reps * 4) for _ in range(rounds)]
    host_t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        by_numpy()
        torch.cuda.synchronize()
        host_t.append(time.perf_counter() - t0)
    rec = {"weights_of_layers": [first, first + count], "diagonals": nd, "L": L,
           "device_table_plus_encode_us": round(statistics.median(dev_t) * 1e6, 1), "device_us_min_max": [round(min(dev_t) * 1e6, 1), round(max(dev_t) * 1e6, 1)],
           "table_kernel_alone_us": round(statistics.median(ker_t) * 1e6, 1),
           "numpy_table_upload_encode_us": round(statistics.median(host_t) * 1e6, 1), "numpy_us_min_max": [round(min(host_t) * 1e6, 1), round(max(host_t) * 1e6, 1)]}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coeff_to_slot.py needs an MI355X: there is no CPU path and no timing without the GPU")
    pkg = entry.load_package()
    import pytroy
    print("# %s; CKKS N=%d, n=%d, 40-bit primes, scale 2^30 x 2^40; reps %d, rounds %d (median of rounds; min..max)" %
          (torch.cuda.get_device_name(0), N, N // 2, args.reps, args.rounds), flush=True)
    weights(pkg, torch.device("cuda", 0), args.reps, args.rounds)
    for groups in ([1] * M, S.default_groups(M, 3), S.default_groups(M, 4)):
        evaluation(pytroy, groups, args.reps, args.rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
