#!/usr/bin/env python3
"""The packed sparse CKKS bootstrap (troy::BootstrapPlan with `packed`: real and imaginary parts in ONE EvalMod operand) against the unpacked sparse call of
the same build.  Writes profiles/packed_bootstrap_bench.txt (--out).

Through pytroy, the chain, keys and parameters of tools/bench_sparse_bootstrap.py: CKKS N = 16384, a 60-bit q0, 22 working primes of 50 bits and a 60-bit
special prime, D = 2^50, weights at 2^50, K = 256, degree 79 with 5 double angles.  SUCH A CHAIN IS NOT A SECURE PARAMETER SET at N = 16384: the figures
time the schedule, not a deployable configuration.

  bootstrap   one Evaluator::bootstrap at n = 256 in 4 + 4 and in 3 + 3 + 2, unpacked and packed, on one message and one set of keys.  Before any timing the
              decoded slots of both forms are compared with the message and with each other.
  stages      the same chain as separate Evaluator calls, for both forms: ModRaise, SubSum, CoeffToSlot (the packed one includes its conjugation; the unpacked
              one is followed by split_real_imag, listed on its own), EvalMod (two operands in one schedule / one operand), join_real_imag (unpacked only),
              SlotToCoeff (the packed one includes its rotation by n).  Each stage runs on the true output of the one before it.
  table       troyn_ckks_dft_factor_diagonals_packed alone through the C-ABI binding: n = 256, layers [0, 4), both directions.

The variants alternate round by round in one process; every timing follows bench.timed (at least 50 ms of warm-up on the timed call itself, then `reps`
back-to-back calls closed by a device synchronise); the median over the rounds is reported with its range.

python tools/bench_packed_bootstrap.py [--reps 3] [--rounds 5] [--out profiles/packed_bootstrap_bench.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402

N, BITS = 16384, [60] + [50] * 22 + [60]
DELTA, WEIGHT, K, DEGREE, DOUBLE_ANGLES = float(1 << 50), float(1 << 50), 256.0, 79, 5
SLOTS_N = 256
GROUPINGS = {"4+4": [4, 4], "3+3+2": [3, 3, 2]}


def _median(times):
    return {k: statistics.median(v) for k, v in times.items()}


def _ms(x):
    return round(x * 1e3, 3)


def stages(ev, plan, rk, gk, exhausted):
    """the chain of Evaluator::bootstrap as separate calls -> [(name, call)], each call on the true output of the stage before it"""
    n, out = plan.n(), []
    raised = ev.mod_raise_new(exhausted)
    out.append(("mod_raise", lambda: ev.mod_raise_new(exhausted)))
    summed = ev.sub_sum_new(raised, n, gk, plan.sub_sum_radix())
    out.append(("sub_sum", lambda: ev.sub_sum_new(raised, n, gk, plan.sub_sum_radix())))
    summed.set_scale(plan.q0())
    down, up = plan.coeff_to_slot_plan(), plan.slot_to_coeff_plan()
    slots = ev.coeff_to_slot_new(summed, down, gk)
    out.append(("coeff_to_slot", lambda: ev.coeff_to_slot_new(summed, down, gk)))
    relabel = slots.scale() * (2.0 * plan.coeff_to_slot_constant() * plan.sub_sum_factor())
    args = (rk, plan.half_width(), plan.degree(), plan.double_angles())
    if plan.packed():
        slots.set_scale(relabel)
        reduced = ev.eval_mod_new_batched([slots], *args)[0]
        out.append(("eval_mod", lambda: ev.eval_mod_new_batched([slots], *args)))
    else:
        re, im = ev.split_real_imag_new(slots, gk)
        out.append(("split_real_imag", lambda: ev.split_real_imag_new(slots, gk)))
        re.set_scale(relabel)
        im.set_scale(relabel)
        parts = ev.eval_mod_new_batched([re, im], *args)
        out.append(("eval_mod", lambda: ev.eval_mod_new_batched([re, im], *args)))
        reduced = ev.join_real_imag_new(parts[0], parts[1])
        out.append(("join_real_imag", lambda: ev.join_real_imag_new(parts[0], parts[1])))
    result = ev.slot_to_coeff_new(reduced, up, gk)
    out.append(("slot_to_coeff", lambda: ev.slot_to_coeff_new(reduced, up, gk)))
    result.set_scale(plan.output_scale())
    return out, result


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
    plans = {}
    for name, g in GROUPINGS.items():
        plans[name, "unpacked"] = pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, g, g, WEIGHT, n=SLOTS_N)
        plans[name, "packed"] = pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, g, g, WEIGHT, n=SLOTS_N, packed=True)
    steps = set()
    for plan in plans.values():
        steps |= set(plan.rotation_steps())
    gk = kg.create_galois_keys_from_steps(sorted(steps), False)
    slots = lambda c: np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c)))      # noqa: E731
    message = np.tile(unit_disc(np.random.default_rng(41), SLOTS_N), slot_count // SLOTS_N)
    fresh = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in message], None, DELTA))
    exhausted = ev.mod_switch_to_new(fresh, ctx.last_parms_id())
    depth = pytroy.chebyshev_depth(DEGREE) + DOUBLE_ANGLES

    # the results first: both forms against the message and against each other
    calls = {key: (lambda plan=plan: ev.bootstrap_new(exhausted, plan, rk, gk)) for key, plan in plans.items()}
    values = {key: slots(call()) for key, call in calls.items()}
    err = {key: float(np.max(np.abs(v - message))) for key, v in values.items()}
    for name in GROUPINGS:
        if not err[name, "packed"] <= 2 * err[name, "unpacked"]:
            raise SystemExit("packed %s: slot error %.3e against %.3e of the unpacked call: not timed" % (name, err[name, "packed"], err[name, "unpacked"]))
    times = {key: [] for key in calls}
    for _ in range(args.rounds):
        for key, call in calls.items():
            times[key].append(bench.timed(torch, call, args.reps))
    med = _median(times)
    for (name, form), plan in plans.items():
        emit({"bootstrap": True, "N": N, "n": SLOTS_N, "groups": name, "form": form, "levels": plan.levels(), "galois_key_switches": plan.key_switches(),
              "eval_mod_operands": 1 if plan.packed() else 2, "eval_mod_depth": depth, "distinct_keys": len(plan.rotation_steps()),
              "ms": _ms(med[name, form]), "ms_min_max": [_ms(min(times[name, form])), _ms(max(times[name, form]))],
              "time_vs_unpacked": round(med[name, form] / med[name, "unpacked"], 3), "slot_error": err[name, form],
              "slot_difference_from_unpacked": float(np.max(np.abs(values[name, form] - values[name, "unpacked"]))), "secure_parameter_set": False})

    # stage by stage
    for name in GROUPINGS:
        for form in ("unpacked", "packed"):
            parts, result = stages(ev, plans[name, form], rk, gk, exhausted)
            staged_error = float(np.max(np.abs(slots(result) - message)))
            stage_times = {k: [] for k, _ in parts}
            for _ in range(args.rounds):
                for k, call in parts:
                    stage_times[k].append(bench.timed(torch, call, args.reps))
            smed = _median(stage_times)
            emit({"stages": True, "N": N, "n": SLOTS_N, "groups": name, "form": form, "ms": {k: _ms(v) for k, v in smed.items()}, "ms_sum": _ms(sum(smed.values())),
                  "ms_min_max": {k: [_ms(min(v)), _ms(max(v))] for k, v in stage_times.items()}, "slot_error_of_the_staged_chain": staged_error})

    # the table kernel alone, through the C-ABI binding on a handle of the same ring
    pkg = entry.load_package()
    O = entry.load_oracle()
    plan = pkg.Plan("cuda:0", 14, O.coeff_modulus_create(N, BITS))
    handle = plan.ckks_handle()
    table = {("inverse" if inv else "forward"): (lambda inv=inv: handle.dft_factor_diagonals_packed(SLOTS_N, 0, 4, inverse=inv, constant=0.9)) for inv in (False, True)}
    table["sparse_2n_forward"] = lambda: handle.dft_factor_diagonals_sparse(2 * SLOTS_N, 0, 4, constant=0.9)
    ttimes = {k: [] for k in table}
    for _ in range(args.rounds):
        for k, call in table.items():
            ttimes[k].append(bench.timed(torch, call, 50))
    emit({"table": True, "N": N, "n": SLOTS_N, "layers": [0, 4], "diagonals": 31, "rows": 2 * SLOTS_N, "bytes": 31 * 2 * SLOTS_N * 16,
          "us_per_call_with_allocation": {k: round(v * 1e6, 2) for k, v in _median(ttimes).items()},
          "note": "one launch of 2 x 31 workgroups; the time is the launch and the output allocation, not the arithmetic"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_bootstrap_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_packed_bootstrap.py needs an MI355X: there is no CPU path and no timing without the GPU")
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
