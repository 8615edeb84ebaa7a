"""Sparse packing through pytroy (additions; troy/bootstrap.h "Sparse packing"): Evaluator::sub_sum, the slot plans and BootstrapPlan with
n below the slot count, on the context of tests/test_gpu_bootstrap_api.py -- CKKS N = 1024, a 60-bit q0, seventeen 50-bit primes, a 60-bit special prime,
D = 2^50, K = 64, degree 79 with 3 double angles.

Tolerances, every reference measured in the same run and printed:
  sub_sum            4 x s x the slot error of ONE rotate_vector of the same operand: s terms add, each with the noise of one key switch on top of the
                     operand's own, and the factor 4 is the margin test_split_real_imag_and_join gives a key switch.  The expected slots come from the
                     plaintext polynomial (decoded before encryption): its Y-part times s, through numpy's encoder tables.
  slot plans         the rule of DESIGN 4.5n: 4 x groups x the slot error of Evaluator::linear_transform on the DENSE n x n matrix of the top group
                     (forward), same operand, level and scales.
  sparse bootstrap   e_full is the slot error of the EXISTING full plan (3 + 3 + 3 twice) on the same message tiled, same context and keys.  The sparse
                     plan must stay within 2 x e_full, the margin and the argument of tests/test_gpu_bootstrap_api.py: it shares EvalMod, which dominates,
                     and has fewer groups; SubSum multiplies message and noise alike.  A wrong constant, sign or SubSum factor is an error of order 1.
                     The product with a fresh ciphertext is held against the same product of the full plan's result in the same way.
"""
import math

import numpy as np
import pytest

import ckks_encode_spec as E
import sparse_bootstrap_spec as S
from test_gpu_hoist_api import pytroy  # noqa: F401  (the module's fixture)
from test_gpu_linear_transform_api import _ckks
from test_gpu_bootstrap_api import BITS, DEGREE, DELTA, DOUBLE_ANGLES, K, N, SLOTS
from test_sparse_secret_spec import ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, EPHEMERAL_WEIGHT

pytestmark = pytest.mark.gpu

WEIGHT_SCALE = float(1 << 50)
FULL_GROUPS = [3, 3, 3]
SPARSE = {64: [3, 3], 256: [4, 4]}


@pytest.fixture(scope="module")
def world(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy, N, BITS)
    full = pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, FULL_GROUPS, FULL_GROUPS, WEIGHT_SCALE)
    plans = {n: pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, g, g, WEIGHT_SCALE, n=n) for n, g in SPARSE.items()}
    k_small = math.ceil(pytroy.BootstrapPlan.half_width_for(EPHEMERAL_WEIGHT))
    small = pytroy.BootstrapPlan(ctx, enc, DELTA, k_small, ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, SPARSE[64], SPARSE[64], WEIGHT_SCALE, n=64)
    steps = set(full.rotation_steps()) | set(small.rotation_steps())
    for p in plans.values():
        steps |= set(p.rotation_steps())
    gk = kg.create_galois_keys_from_steps(sorted(steps), False)            # from rotation_steps() alone
    rk = kg.create_relin_keys(False)
    messages = {}
    for n in SPARSE:
        rng = np.random.default_rng(2026 + n)
        z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
        z /= np.maximum(np.abs(z), 1.0)
        z = np.tile(z, SLOTS // n)
        z.setflags(write=False)
        messages[n] = z
    w = {"ctx": ctx, "enc": enc, "kg": kg, "encryptor": encryptor, "dec": dec, "ev": ev, "full": full, "plans": plans, "small": small, "k_small": k_small,
         "gk": gk, "rk": rk, "z": messages, "tables": E.numpy_tables(10)}
    yield w
    w.clear()
    pytroy.MemoryPool.destroy_global_pool()


def _encrypt(world, values, scale=DELTA):
    return world["encryptor"].encrypt_asymmetric_new(world["enc"].encode_complex64_simd_new([complex(v) for v in values], None, scale))


def _slots(world, ct):
    return np.asarray(world["enc"].decode_complex64_simd_new(world["dec"].decrypt_new(ct)))


def _err(world, ct, want):
    return float(np.max(np.abs(_slots(world, ct) - want)))


def _lower(ev, c, limbs):
    while c.coeff_modulus_size() > limbs:
        c = ev.mod_switch_to_next_new(c)
    return c


# ---- SubSum ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 256, 16])
def test_sub_sum_keeps_the_y_part_times_s(pytroy, world, n):
    ev, enc, kg = world["ev"], world["enc"], world["kg"]
    s = SLOTS // n
    rng = np.random.default_rng(7 + n)
    z = rng.uniform(-1, 1, SLOTS) + 1j * rng.uniform(-1, 1, SLOTS)          # not periodic: every monomial is present
    plain = enc.encode_complex64_simd_new([complex(v) for v in z], None, DELTA)
    t = np.asarray(enc.decode_float64_polynomial_new(plain))
    assert t.shape == (N,) and np.count_nonzero(np.abs(t[np.arange(N) % s != 0]) > 1e-3) > (N - 2 * n) // 2 > 0
    kept = np.where(np.arange(N) % s == 0, t * s, 0.0)
    re, im = E.simd_from_coefficients(kept, world["tables"])
    want = np.asarray(re) + 1j * np.asarray(im)
    assert np.max(np.abs(want - np.tile(want[:n], s))) < 1e-9               # the result repeats with period n
    c = _lower(ev, world["encryptor"].encrypt_asymmetric_new(plain), 2)
    e_rot = _err(world, ev.rotate_vector_new(c, 1, kg.create_galois_keys_from_steps([1], False)), np.roll(z, -1))
    bound = 4 * s * e_rot
    results = {}
    for radix in (2, 4, s):
        steps = pytroy.Evaluator.sub_sum_steps(SLOTS, n, radix)
        assert steps == S.sub_sum_steps(SLOTS, n, radix) and pytroy.Evaluator.sub_sum_stages(SLOTS, n, radix) == S.sub_sum_stages(SLOTS, n, radix)
        gk = kg.create_galois_keys_from_steps(steps, False)                 # sub_sum_steps suffices
        got = ev.sub_sum_new(c, n, gk, radix)
        assert got.parms_id() == c.parms_id() and got.scale() == c.scale() and got.is_ntt_form()
        results[radix] = _slots(world, got)
        err = float(np.max(np.abs(results[radix] - want)))
        print("sub_sum n = %d (s = %d) radix %d: %d key switches, slot error %.3e; one rotate %.3e, bound 4 x s x that = %.3e"
              % (n, s, radix, sum(len(st) for st in S.sub_sum_stages(SLOTS, n, radix)), err, e_rot, bound))
        assert err <= bound
    for radix in (4, s):
        assert float(np.max(np.abs(results[radix] - results[2]))) <= bound
    # the default radix is the plan's, and the destination form
    default = pytroy.Evaluator.sub_sum_steps(SLOTS, n)
    assert default == pytroy.Evaluator.sub_sum_steps(SLOTS, n, world["plans"][64].sub_sum_radix())
    dest = pytroy.Ciphertext()
    ev.sub_sum(encrypted=c, n=n, galois_keys=kg.create_galois_keys_from_steps(default, False), destination=dest)
    assert float(np.max(np.abs(_slots(world, dest) - want))) <= bound


def test_sub_sum_identity_and_refusals(pytroy, world):
    ev, kg = world["ev"], world["kg"]
    c = _lower(ev, _encrypt(world, world["z"][64]), 2)
    unrelated = kg.create_galois_keys_from_steps([5], False)
    assert pytroy.Evaluator.sub_sum_steps(SLOTS, SLOTS) == [] and pytroy.Evaluator.sub_sum_stages(SLOTS, SLOTS, 2) == []
    same = ev.sub_sum_new(c, SLOTS, unrelated)                                # n = slot_count: the identity, no key touched
    assert same.data() == c.data() and same.parms_id() == c.parms_id() and same.scale() == c.scale()
    for n, radix, word in ((1, 0, "power of two"), (3, 0, "power of two"), (1024, 0, "power of two"), (0, 0, "power of two"), (64, 3, "radix"), (64, 1, "radix")):
        with pytest.raises(ValueError, match=r"\[Evaluator::sub_sum\].*" + word):
            ev.sub_sum_new(c, n, unrelated, radix)
        with pytest.raises(ValueError, match=r"\[Evaluator::sub_sum\].*" + word):
            pytroy.Evaluator.sub_sum_steps(SLOTS, n, radix)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.sub_sum_new(c, 64, unrelated)


# ---- the slot plans -------------------------------------------------------------------------------------------------------------------------

def _dense(tables, n, first, count, inverse):
    tab = S.table(tables, n, first, count, inverse=inverse)
    mat = np.zeros((n, n), dtype=np.complex128)
    rows = np.arange(n)
    for a, d in enumerate(S.diagonal_indices(n, first, count)):
        mat[rows, (rows + d) % n] = tab[a, :, 0] + 1j * tab[a, :, 1]
    return mat


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_slot_plans_on_n_slots(pytroy, world, n):
    ctx, enc, kg, ev = world["ctx"], world["enc"], world["kg"], world["ev"]
    groups, m, z = SPARSE[n], n.bit_length() - 1, world["z"][n]
    c = _encrypt(world, z)
    # the reference: Evaluator::linear_transform on the dense matrix of the top group, forward, same operand, level and scales
    top = groups[-1]
    mat = _dense(world["tables"], n, m - top, top, False)
    lt = pytroy.LinearTransform(ctx, enc, n, c.parms_id(), WEIGHT_SCALE, mat.reshape(-1).tolist())
    measured = float(np.max(np.abs(_slots(world, ev.linear_transform_new(c, lt, kg.create_galois_keys_from_steps(lt.rotation_steps(), False)))[:n] - mat @ z[:n])))
    del lt
    down = pytroy.CoeffToSlotPlan(ctx, enc, c.parms_id(), WEIGHT_SCALE, groups, 0.8, n=n)
    assert down.n() == n and down.slot_count() == SLOTS and down.groups() == down.levels() == len(groups) and down.layers_per_group() == groups
    assert [down.first_layer(g) for g in range(len(groups))] == [m - sum(groups[:g + 1]) for g in range(len(groups))]
    assert all(down.transform(g).n() == n for g in range(len(groups))) and down.twin().n() == n
    assert all(0 < st < n for st in down.rotation_steps())
    # the top group holds layer m' - 1: 2^count diagonals; the others 2^(count + 1) - 1; the twin and the conjugation
    assert down.rotations() == ((1 << groups[0]) - 1) * 2 + sum((2 << g) - 2 for g in groups[1:]) + 1
    gk = kg.create_galois_keys_from_steps(sorted(set(down.rotation_steps()) | {0}), False)
    middle = ev.coeff_to_slot_new(c, down, gk)
    assert middle.coeff_modulus_size() == c.coeff_modulus_size() - len(groups)
    # the slots hold constant * BR(t'_k + i t'_{k+n}) on log2 n bits, repeated
    t = np.asarray(E.simd_coefficients(z.real, z.imag, 1.0, world["tables"]))[::SLOTS // n]
    w = np.tile(S.D.bit_reverse(t[:n] + 1j * t[n:], n), SLOTS // n)
    e_down = _err(world, middle, 0.8 * w)
    up = pytroy.SlotToCoeffPlan(ctx, enc, middle.parms_id(), WEIGHT_SCALE, groups, 1.0 / 0.8, n=n)
    assert up.n() == n and up.boundary_group() == len(groups) - 1 and [up.first_layer(g) for g in range(len(groups))] == [sum(groups[:g]) for g in range(len(groups))]
    back = ev.slot_to_coeff_new(middle, up, kg.create_galois_keys_from_steps(sorted(set(up.rotation_steps()) | {0}), False))
    err = _err(world, back, z)
    bound = 4 * 2 * len(groups) * measured
    print("n = %d groups %s: dense top group %.3e; coeff_to_slot error %.3e (bound %.3e), round trip %.3e (bound 4 x %d x dense = %.3e); %d + %d rotations"
          % (n, groups, measured, e_down, 4 * len(groups) * measured, err, 2 * len(groups), bound, down.rotations(), up.rotations()))
    assert e_down <= 4 * len(groups) * measured
    assert err <= bound
    for cls, name in ((pytroy.CoeffToSlotPlan, "CoeffToSlotPlan"), (pytroy.SlotToCoeffPlan, "SlotToCoeffPlan")):
        with pytest.raises(ValueError, match=r"\[%s::%s\].*sum to log2 n" % (name, name)):
            cls(ctx, enc, c.parms_id(), WEIGHT_SCALE, [3, 3, 3], 1.0, n=n)
        for bad in (1, 3, 1024):
            with pytest.raises(ValueError, match=r"\[%s::%s\].*power of two" % (name, name)):
                cls(ctx, enc, c.parms_id(), WEIGHT_SCALE, [], 1.0, n=bad)


def test_the_plans_count_levels_key_switches_and_steps(pytroy, world):
    full = world["full"]
    depth = pytroy.chebyshev_depth(DEGREE) + DOUBLE_ANGLES
    assert full.n() == full.slot_count() == SLOTS and full.sub_sum_key_switches() == 0 and full.sub_sum_factor() == 1.0 and full.levels() == 3 + depth + 3
    for n, groups in SPARSE.items():
        plan = world["plans"][n]
        down, up = plan.coeff_to_slot_plan(), plan.slot_to_coeff_plan()
        assert plan.n() == down.n() == up.n() == n and plan.slot_count() == SLOTS and plan.sub_sum_factor() == SLOTS // n
        assert plan.levels() == len(groups) + depth + len(groups) == down.groups() + plan.eval_mod_depth() + up.groups() == full.levels() - 2
        stages = S.sub_sum_stages(SLOTS, n, plan.sub_sum_radix())
        assert plan.sub_sum_radix() == 4 and plan.sub_sum_key_switches() == sum(len(st) for st in stages)
        # (groups of four layers have 16 + 31 diagonals where groups of three have 8 + 15: at N = 1024 the 4 + 4 plan of n = 256 spends MORE key switches than
        # the full 3 + 3 + 3 plan and buys its two levels with them; the count is printed, not ranked)
        assert plan.key_switches() == plan.sub_sum_key_switches() + down.rotations() + 1 + up.rotations()
        assert plan.rotation_steps() == sorted(set(down.rotation_steps()) | set(up.rotation_steps()) | {0} | set(S.sub_sum_steps(SLOTS, n, 4)))
        assert plan.coeff_to_slot_constant() * plan.sub_sum_factor() == pytest.approx(full.coeff_to_slot_constant(), rel=1e-3)   # c1 / s; the groups' primes differ
        print("n = %d: levels %d (full %d), key switches %d (full %d; SubSum %d), keys %d (full %d)"
              % (n, plan.levels(), full.levels(), plan.key_switches(), full.key_switches(), plan.sub_sum_key_switches(), len(plan.rotation_steps()), len(full.rotation_steps())))
    ctx, enc = world["ctx"], world["enc"]
    two = pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, [3, 3], [3, 3], WEIGHT_SCALE, n=64, sub_sum_radix=2)
    assert two.sub_sum_radix() == 2 and two.sub_sum_key_switches() == 3
    P = r"\[BootstrapPlan::BootstrapPlan\]"
    for bad in (1, 3, 1024):
        with pytest.raises(ValueError, match=P + ".*power of two"):
            pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, [], [], WEIGHT_SCALE, n=bad)
    with pytest.raises(ValueError, match=P + ".*sub_sum_radix"):
        pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, [3, 3], [3, 3], WEIGHT_SCALE, n=64, sub_sum_radix=3)
    with pytest.raises(ValueError, match=r"sum to log2 n"):
        pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, [3, 3, 3], [3, 3, 3], WEIGHT_SCALE, n=64)


# ---- the bootstrap --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_errors(world):
    """n -> (e_full, e_prod_full): the existing full plan on the tiled message of that n, and one more product with a fresh ciphertext"""
    ev, gk, rk, ctx = world["ev"], world["gk"], world["rk"], world["ctx"]
    out = {}
    for n, z in world["z"].items():
        res = ev.bootstrap_new(ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id()), world["full"], rk, gk)
        e_full = _err(world, res, z)
        other = _lower(ev, _encrypt(world, np.conj(z)), res.coeff_modulus_size())
        e_prod = _err(world, ev.rescale_to_next_new(ev.relinearize_new(ev.multiply_new(res, other), rk)), z * np.conj(z))
        print("full plan on the message of n = %d tiled: slot error e_full %.3e, after one more product %.3e" % (n, e_full, e_prod))
        out[n] = e_full, e_prod
    return out


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_sparse_bootstrap_against_the_full_one(pytroy, world, full_errors, n):
    ev, gk, rk, ctx, plan, z = world["ev"], world["gk"], world["rk"], world["ctx"], world["plans"][n], world["z"][n]
    e_full, e_prod_full = full_errors[n]
    exhausted = ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id())
    assert exhausted.coeff_modulus_size() == 1
    out = ev.bootstrap_new(exhausted, plan, rk, gk)
    # the extra levels the plan promises: two groups fewer than the full plan's six
    assert out.parms_id() == plan.output_parms_id() and out.scale() == DELTA and out.coeff_modulus_size() == len(BITS) - 1 - plan.levels() == 4
    err = _err(world, out, z)
    print("sparse bootstrap n = %d groups %s: slot error %.3e, full plan e_full %.3e, bound 2 x e_full = %.3e" % (n, SPARSE[n], err, e_full, 2 * e_full))
    assert err <= 2 * e_full
    other = _lower(ev, _encrypt(world, np.conj(z)), out.coeff_modulus_size())
    prod = ev.rescale_to_next_new(ev.relinearize_new(ev.multiply_new(out, other), rk))
    assert prod.coeff_modulus_size() == 3
    e_prod = _err(world, prod, z * np.conj(z))
    print("sparse bootstrap n = %d, then one product: slot error %.3e, full plan %.3e, bound 2 x that" % (n, e_prod, e_prod_full))
    assert e_prod <= 2 * e_prod_full


def test_sparse_bootstrap_behind_the_encapsulation(pytroy, world, full_errors):
    """h = 32, K = 12 at n = 64: sub_sum runs after the to_dense switch"""
    ev, gk, rk, ctx, small, z = world["ev"], world["gk"], world["rk"], world["ctx"], world["small"], world["z"][64]
    assert world["k_small"] == 12 and small.n() == 64
    keys = world["kg"].create_sparse_encapsulation_keys(EPHEMERAL_WEIGHT)
    out = ev.bootstrap_new(ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id()), small, rk, gk, encapsulation_keys=keys)
    assert out.parms_id() == small.output_parms_id() and out.scale() == DELTA
    err = _err(world, out, z)
    print("sparse bootstrap n = 64 behind the encapsulation (h = %d, K = %d): slot error %.3e, bound 2 x e_full = %.3e" % (EPHEMERAL_WEIGHT, world["k_small"], err, 2 * full_errors[64][0]))
    assert err <= 2 * full_errors[64][0]


def test_n_zero_and_n_slot_count_are_todays_plan(pytroy, world):
    ctx, enc, ev, gk, rk = world["ctx"], world["enc"], world["ev"], world["gk"], world["rk"]
    exhausted = ev.mod_switch_to_new(_encrypt(world, world["z"][256]), ctx.last_parms_id())
    want = ev.bootstrap_new(exhausted, world["full"], rk, gk)
    for n in (0, SLOTS):
        plan = pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, FULL_GROUPS, FULL_GROUPS, WEIGHT_SCALE, n=n, sub_sum_radix=2)
        assert plan.n() == SLOTS and plan.rotation_steps() == world["full"].rotation_steps() and plan.key_switches() == world["full"].key_switches()
        assert plan.coeff_to_slot_constant() == world["full"].coeff_to_slot_constant() and plan.slot_to_coeff_constant() == world["full"].slot_to_coeff_constant()
        got = ev.bootstrap_new(exhausted, plan, rk, gk)
        assert got.data() == want.data() and got.parms_id() == want.parms_id() and got.scale() == want.scale()
    c = _encrypt(world, world["z"][256])
    old = pytroy.CoeffToSlotPlan(ctx, enc, c.parms_id(), WEIGHT_SCALE, FULL_GROUPS, 0.8)
    new = pytroy.CoeffToSlotPlan(ctx, enc, c.parms_id(), WEIGHT_SCALE, FULL_GROUPS, 0.8, n=SLOTS)
    keys = world["kg"].create_galois_keys_from_steps(sorted(set(old.rotation_steps()) | {0}), False)
    assert new.rotation_steps() == old.rotation_steps() and ev.coeff_to_slot_new(c, new, keys).data() == ev.coeff_to_slot_new(c, old, keys).data()
