"""The packed sparse bootstrap through pytroy (additions; troy/bootstrap.h and troy/slot_transform.h "Packed"): the slot plans and BootstrapPlan
with `packed`, on the context of tests/test_gpu_sparse_bootstrap_api.py -- CKKS N = 1024, a 60-bit q0, seventeen 50-bit primes, a 60-bit special prime,
D = 2^50, K = 64, degree 79 with 3 double angles; n = 64 in 3 + 3 and n = 256 = N/4 in 4 + 4.

Tolerances, every reference measured in the same run and printed:
  slot plans         the rule of tests/test_gpu_sparse_bootstrap_api.py: 4 x groups x the slot error of Evaluator::linear_transform on the DENSE
                     n x n matrix of the top group (forward), same operand, level and scales.  The packed coeff_to_slot is held against [2 Re; 2 Im] of the
                     UNPACKED coeff_to_slot's decoded slots on the same operand; the round trip (2 x groups groups) against the message.
  packed bootstrap   e_unpacked is the slot error of the unpacked sparse plan on the same message, context and keys.  The packed plan must stay within
                     2 x e_unpacked, the project's rule for a second path on the same parameters: it shares SubSum, every group but two, and EvalMod's
                     polynomial, at the same levels and scales.  A wrong quarter turn, half or constant is an error of order 1.  The product with a fresh
                     ciphertext is held against the same product of the unpacked result in the same way.
"""
import math

import numpy as np
import pytest

import ckks_encode_spec as E
from test_gpu_hoist_api import pytroy  # noqa: F401  (the module's fixture)
from test_gpu_linear_transform_api import _ckks
from test_gpu_bootstrap_api import BITS, DEGREE, DELTA, DOUBLE_ANGLES, K, N, SLOTS
from test_gpu_sparse_bootstrap_api import SPARSE, WEIGHT_SCALE, _dense
from test_sparse_secret_spec import ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, EPHEMERAL_WEIGHT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy, N, BITS)
    args = (ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES)
    unpacked = {n: pytroy.BootstrapPlan(*args, g, g, WEIGHT_SCALE, n=n) for n, g in SPARSE.items()}
    packed = {n: pytroy.BootstrapPlan(*args, g, g, WEIGHT_SCALE, n=n, packed=True) for n, g in SPARSE.items()}
    k_small = math.ceil(pytroy.BootstrapPlan.half_width_for(EPHEMERAL_WEIGHT))
    small = (ctx, enc, DELTA, k_small, ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, SPARSE[64], SPARSE[64], WEIGHT_SCALE)
    small_unpacked, small_packed = pytroy.BootstrapPlan(*small, n=64), pytroy.BootstrapPlan(*small, n=64, packed=True)
    steps = set()
    for p in list(unpacked.values()) + list(packed.values()) + [small_unpacked, small_packed]:
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
    w = {"ctx": ctx, "enc": enc, "kg": kg, "encryptor": encryptor, "dec": dec, "ev": ev, "unpacked": unpacked, "packed": packed, "small_unpacked": small_unpacked,
         "small_packed": small_packed, "k_small": k_small, "gk": gk, "rk": rk, "z": messages, "tables": E.numpy_tables(10)}
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


# ---- the slot plans -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sorted(SPARSE))
def test_packed_slot_plans(pytroy, world, n):
    ctx, enc, kg, ev = world["ctx"], world["enc"], world["kg"], world["ev"]
    groups, m, z = SPARSE[n], n.bit_length() - 1, world["z"][n]
    c = _encrypt(world, z)
    # the reference: Evaluator::linear_transform on the dense matrix of the top group, forward, same operand, level and scales
    top = groups[-1]
    mat = _dense(world["tables"], n, m - top, top, False)
    lt = pytroy.LinearTransform(ctx, enc, n, c.parms_id(), WEIGHT_SCALE, mat.reshape(-1).tolist())
    measured = float(np.max(np.abs(_slots(world, ev.linear_transform_new(c, lt, kg.create_galois_keys_from_steps(lt.rotation_steps(), False)))[:n] - mat @ z[:n])))
    del lt
    plain = pytroy.CoeffToSlotPlan(ctx, enc, c.parms_id(), WEIGHT_SCALE, groups, 0.8, n=n)
    down = pytroy.CoeffToSlotPlan(ctx, enc, c.parms_id(), WEIGHT_SCALE, groups, 0.8, n=n, packed=True)
    assert down.packed() and not plain.packed() and down.n() == n and down.groups() == down.levels() == len(groups)
    assert down.packed_group() == len(groups) - 1 != down.boundary_group() and down.first_layer(down.packed_group()) == 0
    last = groups[-1]
    assert down.transform(down.packed_group()).n() == 2 * n and down.transform(0).n() == n and down.twin().n() == n
    # the packed group has the diagonals it had, now mod 2n; the conjugation of v + conj(v) is the one key switch more than the unpacked plan's
    assert down.rotations() == plain.rotations() + 1
    assert all(0 < st < 2 * n for st in down.rotation_steps())
    assert {k for k in range(1, 1 << last)} | {2 * n - k for k in range(1, 1 << last)} <= set(down.rotation_steps())
    gk = kg.create_galois_keys_from_steps(sorted(set(down.rotation_steps()) | set(plain.rotation_steps()) | {0}), False)
    reference = _slots(world, ev.coeff_to_slot_new(c, plain, gk))[:n]
    middle = ev.coeff_to_slot_new(c, down, gk)
    assert middle.coeff_modulus_size() == c.coeff_modulus_size() - len(groups)
    want = np.tile(np.concatenate([2.0 * reference.real, 2.0 * reference.imag]), SLOTS // (2 * n)).astype(np.complex128)
    e_down = _err(world, middle, want)
    up_plain = pytroy.SlotToCoeffPlan(ctx, enc, middle.parms_id(), WEIGHT_SCALE, groups, 1.0 / 1.6, n=n)
    up = pytroy.SlotToCoeffPlan(ctx, enc, middle.parms_id(), WEIGHT_SCALE, groups, 1.0 / 1.6, n=n, packed=True)
    assert up.packed() and up.packed_group() == 0 != up.boundary_group() and up.transform(0).n() == 2 * n and up.transform(len(groups) - 1).n() == n
    assert up.rotations() == up_plain.rotations() + 1 and n in up.rotation_steps() and all(0 < st < 2 * n for st in up.rotation_steps())
    back = ev.slot_to_coeff_new(middle, up, kg.create_galois_keys_from_steps(sorted(set(up.rotation_steps()) | {0}), False))
    assert back.coeff_modulus_size() == middle.coeff_modulus_size() - len(groups)
    err = _err(world, back, z)
    bound = 4 * 2 * len(groups) * measured
    print("n = %d groups %s packed: dense top group %.3e; packed coeff_to_slot against [2 Re; 2 Im] of the unpacked one %.3e (bound %.3e), round trip %.3e "
          "(bound 4 x %d x dense = %.3e); %d + %d rotations (unpacked %d + %d)"
          % (n, groups, measured, e_down, 4 * len(groups) * measured, err, 2 * len(groups), bound, down.rotations(), up.rotations(), plain.rotations(), up_plain.rotations()))
    assert e_down <= 4 * len(groups) * measured
    assert err <= bound


def test_refusals(pytroy, world):
    ctx, enc = world["ctx"], world["enc"]
    first = _encrypt(world, world["z"][64]).parms_id()
    for cls, name in ((pytroy.CoeffToSlotPlan, "CoeffToSlotPlan"), (pytroy.SlotToCoeffPlan, "SlotToCoeffPlan")):
        P = r"\[%s::%s\]" % (name, name)
        for bad, groups in ((SLOTS, [3, 3, 3]), (2, [1]), (0, [3, 3, 3])):          # n = N/2 (also as the default), n = 2
            with pytest.raises(ValueError, match=P + ".*packed plan needs a power of two"):
                cls(ctx, enc, first, WEIGHT_SCALE, groups, 1.0, n=bad, packed=True)
        with pytest.raises(ValueError, match=P + ".*at least two groups"):
            cls(ctx, enc, first, WEIGHT_SCALE, [6], 1.0, n=64, packed=True)
        assert not cls(ctx, enc, first, WEIGHT_SCALE, [6], 1.0, n=64, packed=False).packed()
    P = r"\[BootstrapPlan::BootstrapPlan\]"
    args = (ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES)
    for bad, groups in ((SLOTS, [3, 3, 3]), (2, [1]), (0, [3, 3, 3])):
        with pytest.raises(ValueError, match=P + ".*packed plan needs a power of two"):
            pytroy.BootstrapPlan(*args, groups, groups, WEIGHT_SCALE, n=bad, packed=True)
    with pytest.raises(ValueError, match="at least two groups"):
        pytroy.BootstrapPlan(*args, [6], [3, 3], WEIGHT_SCALE, n=64, packed=True)
    with pytest.raises(ValueError, match="at least two groups"):
        pytroy.BootstrapPlan(*args, [3, 3], [6], WEIGHT_SCALE, n=64, packed=True)


# ---- the bootstrap --------------------------------------------------------------------------------------------------------------------------

def test_the_plans_count_levels_key_switches_and_steps(pytroy, world):
    for n, groups in SPARSE.items():
        plain, plan = world["unpacked"][n], world["packed"][n]
        assert plan.packed() and not plain.packed() and plan.n() == n and plan.slot_count() == SLOTS
        assert plan.levels() == plain.levels() and plan.output_parms_id() == plain.output_parms_id() and plan.eval_mod_depth() == plain.eval_mod_depth()
        assert plan.key_switches() == plain.key_switches() + 1
        down, up = plan.coeff_to_slot_plan(), plan.slot_to_coeff_plan()
        assert down.packed() and up.packed()
        assert plan.key_switches() == plan.sub_sum_key_switches() + down.rotations() + up.rotations()
        assert plan.rotation_steps() == sorted(set(down.rotation_steps()) | set(up.rotation_steps()) | {0} | set(pytroy.Evaluator.sub_sum_steps(SLOTS, n, 4)))
        assert n in plan.rotation_steps()
        assert plan.coeff_to_slot_constant() == plain.coeff_to_slot_constant() and plan.slot_to_coeff_constant() == plain.slot_to_coeff_constant()
        print("n = %d packed: levels %d (unpacked %d), key switches %d (unpacked %d), keys %d (unpacked %d)"
              % (n, plan.levels(), plain.levels(), plan.key_switches(), plain.key_switches(), len(plan.rotation_steps()), len(plain.rotation_steps())))


@pytest.fixture(scope="module")
def unpacked_results(world):
    """n -> (the unpacked sparse plan's result, its slot error, its error after one more product with a fresh ciphertext)"""
    ev, gk, rk, ctx = world["ev"], world["gk"], world["rk"], world["ctx"]
    out = {}
    for n, z in world["z"].items():
        res = ev.bootstrap_new(ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id()), world["unpacked"][n], rk, gk)
        e_plain = _err(world, res, z)
        other = _lower(ev, _encrypt(world, np.conj(z)), res.coeff_modulus_size())
        e_prod = _err(world, ev.rescale_to_next_new(ev.relinearize_new(ev.multiply_new(res, other), rk)), z * np.conj(z))
        print("unpacked sparse plan n = %d: slot error %.3e, after one more product %.3e" % (n, e_plain, e_prod))
        out[n] = res.coeff_modulus_size(), e_plain, e_prod
    return out


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_packed_bootstrap_against_the_unpacked_one(pytroy, world, unpacked_results, n):
    ev, gk, rk, ctx, plan, z = world["ev"], world["gk"], world["rk"], world["ctx"], world["packed"][n], world["z"][n]
    limbs, e_plain, e_prod_plain = unpacked_results[n]
    exhausted = ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id())
    assert exhausted.coeff_modulus_size() == 1
    out = ev.bootstrap_new(exhausted, plan, rk, gk)
    assert out.parms_id() == plan.output_parms_id() and out.scale() == DELTA and out.coeff_modulus_size() == limbs == len(BITS) - 1 - plan.levels()
    err = _err(world, out, z)
    print("packed bootstrap n = %d groups %s: slot error %.3e, unpacked %.3e, bound 2 x that = %.3e" % (n, SPARSE[n], err, e_plain, 2 * e_plain))
    assert err <= 2 * e_plain
    other = _lower(ev, _encrypt(world, np.conj(z)), out.coeff_modulus_size())
    prod = ev.rescale_to_next_new(ev.relinearize_new(ev.multiply_new(out, other), rk))
    e_prod = _err(world, prod, z * np.conj(z))
    print("packed bootstrap n = %d, then one product: slot error %.3e, unpacked %.3e, bound 2 x that" % (n, e_prod, e_prod_plain))
    assert e_prod <= 2 * e_prod_plain


def test_packed_bootstrap_behind_the_encapsulation(pytroy, world):
    """h = 32, K = 12 at n = 64: ModRaise under the sparse secret, to_dense, SubSum, then the packed chain"""
    ev, gk, rk, ctx, z = world["ev"], world["gk"], world["rk"], world["ctx"], world["z"][64]
    assert world["k_small"] == 12 and world["small_packed"].packed() and world["small_packed"].key_switches() == world["small_unpacked"].key_switches() + 1
    keys = world["kg"].create_sparse_encapsulation_keys(EPHEMERAL_WEIGHT)
    exhausted = ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id())
    plain = ev.bootstrap_new(exhausted, world["small_unpacked"], rk, gk, encapsulation_keys=keys)
    out = ev.bootstrap_new(exhausted, world["small_packed"], rk, gk, encapsulation_keys=keys)
    assert out.parms_id() == world["small_packed"].output_parms_id() == plain.parms_id() and out.scale() == DELTA
    e_plain, err = _err(world, plain, z), _err(world, out, z)
    print("packed bootstrap n = 64 behind the encapsulation (h = %d, K = %d): slot error %.3e, unpacked %.3e, bound 2 x that" % (EPHEMERAL_WEIGHT, world["k_small"], err, e_plain))
    assert err <= 2 * e_plain


def test_packed_false_is_the_plan_without_the_argument(pytroy, world):
    ctx, enc, ev, gk, rk = world["ctx"], world["enc"], world["ev"], world["gk"], world["rk"]
    exhausted = ev.mod_switch_to_new(_encrypt(world, world["z"][64]), ctx.last_parms_id())
    want = ev.bootstrap_new(exhausted, world["unpacked"][64], rk, gk)
    plan = pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, SPARSE[64], SPARSE[64], WEIGHT_SCALE, n=64, packed=False)
    assert not plan.packed() and plan.rotation_steps() == world["unpacked"][64].rotation_steps() and plan.key_switches() == world["unpacked"][64].key_switches()
    got = ev.bootstrap_new(exhausted, plan, rk, gk)
    assert got.data() == want.data() and got.parms_id() == want.parms_id() and got.scale() == want.scale()
    c = _encrypt(world, world["z"][64])
    for cls, run in ((pytroy.CoeffToSlotPlan, ev.coeff_to_slot_new), (pytroy.SlotToCoeffPlan, ev.slot_to_coeff_new)):
        old = cls(ctx, enc, c.parms_id(), WEIGHT_SCALE, SPARSE[64], 0.8, n=64)
        new = cls(ctx, enc, c.parms_id(), WEIGHT_SCALE, SPARSE[64], 0.8, n=64, packed=False)
        keys = world["kg"].create_galois_keys_from_steps(sorted(set(old.rotation_steps()) | {0}), False)
        assert new.rotation_steps() == old.rotation_steps() and new.rotations() == old.rotations() and run(c, new, keys).data() == run(c, old, keys).data()
