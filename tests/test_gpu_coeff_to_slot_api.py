"""troy::CoeffToSlotPlan / SlotToCoeffPlan and Evaluator::coeff_to_slot / slot_to_coeff (additions) through pytroy: CKKS N = 1024, eleven 40-bit
primes (ten levels: the nine groups of a 1 + ... + 1 plan, and 3 + 3 groups with room), ciphertext scale 2^30, weight scale 2^40, the context of
tests/test_gpu_linear_transform_api.py.  Keys: plan.rotation_steps() plus step 0, the conjugation.

Tolerance.  Nothing is invented: the fixture `measured` evaluates the already merged Evaluator::linear_transform on the DENSE matrix of one group
-- the three top layers, inverse for what CoeffToSlot is compared with and forward for what SlotToCoeff returns -- on the same context, operand
level, operand and scales, and takes its largest slot error against numpy's matrix-vector product.  A test allows 4 x groups x that error: errors
add per group, the factor 4 covers the conjugate branch and the rescales.  Measured on an MI355X (the test prints every figure): the dense group 2.301e-07 (inverse) and 1.981e-06 (forward); coeff_to_slot 3 + 3 + 3
9.499e-07 under 2.761e-06, the round trip 1.875e-05 under 4.754e-05, nine groups of one layer 1.103e-06 under 8.28e-06.
"""
import random

import numpy as np
import pytest

import ckks_encode_spec as E
import dft_factors_spec as S
from test_gpu_hoist_api import _batching, _params, pytroy  # noqa: F401  (the module's fixture and parameter helpers)
from test_gpu_linear_transform_api import _ckks
from test_gpu_weighted_hoist_api import _disc

pytestmark = pytest.mark.gpu

N, SLOTS, M = 1024, 512, 9
BITS = (40,) * 11
SCALE = float(1 << 30)
WEIGHT_SCALE = float(1 << 40)
CONSTANT = 0.8


@pytest.fixture(scope="module")
def world(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy, N, BITS)
    rnd = random.Random(2024)
    z = np.array(_disc(rnd, SLOTS))
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z.tolist(), None, SCALE))
    tables = E.numpy_tables(10)
    t = E.simd_coefficients(z.real, z.imag, 1.0, tables)
    w = S.bit_reverse(t[:SLOTS] + 1j * t[SLOTS:], SLOTS)
    for a in (z, t, w):
        a.setflags(write=False)
    yield {"ctx": ctx, "enc": enc, "kg": kg, "encryptor": encryptor, "dec": dec, "ev": ev, "z": z, "c": c, "tables": tables, "w": w}
    pytroy.MemoryPool.destroy_global_pool()


def _keys(world, *plans):
    steps = sorted(set(s for p in plans for s in p.rotation_steps()) | {0})        # step 0: the conjugation
    return world["kg"].create_galois_keys_from_steps(steps, False)


def _slots(world, ct):
    return np.asarray(world["enc"].decode_complex64_simd_new(world["dec"].decrypt_new(ct)))


def _dense(tables, first, count, inverse):
    tab = S.table(tables, first, count, inverse=inverse)
    mat = np.zeros((SLOTS, SLOTS), dtype=np.complex128)
    rows = np.arange(SLOTS)
    for a, d in enumerate(S.diagonal_indices(SLOTS, first, count)):
        mat[rows, (rows + d) % SLOTS] = tab[a, :, 0] + 1j * tab[a, :, 1]
    return mat


@pytest.fixture(scope="module")
def measured(pytroy, world):
    """the slot error of Evaluator::linear_transform on the dense matrix of the top group of three layers: (inverse, forward)"""
    out = []
    for inverse in (True, False):
        mat = _dense(world["tables"], M - 3, 3, inverse)
        lt = pytroy.LinearTransform(world["ctx"], world["enc"], SLOTS, world["c"].parms_id(), WEIGHT_SCALE, mat)
        gk = world["kg"].create_galois_keys_from_steps(lt.rotation_steps(), False)
        got = _slots(world, world["ev"].linear_transform_new(world["c"], lt, gk))
        out.append(float(np.max(np.abs(got - mat @ world["z"]))))
        del lt, gk
    print("dense linear_transform of one group at N = 1024, scale 2^30 x 2^40: slot error %.3e (inverse), %.3e (forward)" % tuple(out))
    return tuple(out)


def test_coeff_to_slot_gives_the_bit_reversed_coefficients(pytroy, world, measured):
    """(a) groups 3 + 3 + 3 with a constant: the slots hold constant * BR(t_k + i t_{k+n}), t from the specification's encoder"""
    plan = pytroy.CoeffToSlotPlan(world["ctx"], world["enc"], world["c"].parms_id(), WEIGHT_SCALE, [3, 3, 3], CONSTANT)
    assert plan.groups() == plan.levels() == 3 and plan.layers_per_group() == [3, 3, 3] and plan.needs_conjugate() and plan.boundary_group() == 0
    assert [plan.first_layer(g) for g in range(3)] == [6, 3, 0] and plan.n() == SLOTS and plan.constant() == CONSTANT
    # the stated baby_count rule: 2^first, every diagonal a giant step (8, 15, 15 diagonals)
    assert [plan.transform(g).baby_count() for g in range(3)] == [64, 8, 1] and plan.twin().baby_count() == 64
    assert all(plan.transform(g).baby_steps() == [0] for g in range(3)) and plan.rotations() == 7 + 14 + 14 + 7 + 1
    steps = set()
    for lt in [plan.transform(g) for g in range(3)] + [plan.twin()]:
        steps |= set(lt.rotation_steps())
    assert plan.rotation_steps() == sorted(steps)
    gk = _keys(world, plan)
    got_ct = world["ev"].coeff_to_slot_new(world["c"], plan, gk)
    assert plan.group_parms_id(0) == world["c"].parms_id() and got_ct.is_ntt_form()
    assert got_ct.parms_id() not in [plan.group_parms_id(g) for g in range(3)]            # one level below the last group's
    err = float(np.max(np.abs(_slots(world, got_ct) - CONSTANT * world["w"])))
    bound = 4 * 3 * measured[0]
    print("coeff_to_slot 3+3+3: slot error %.3e, bound 4 x 3 x %.3e = %.3e; %d rotations" % (err, measured[0], bound, plan.rotations()))
    assert err <= bound
    dest = pytroy.Ciphertext()
    world["ev"].coeff_to_slot(encrypted=world["c"], plan=plan, galois_keys=gk, destination=dest)
    assert dest.parms_id() == got_ct.parms_id()


def test_slot_to_coeff_inverts_coeff_to_slot(pytroy, world, measured):
    """(b) 3 + 3 + 3 down and 3 + 3 + 3 up, the constant 0.8 down and 1 / 0.8 up: z again"""
    down = pytroy.CoeffToSlotPlan(world["ctx"], world["enc"], world["c"].parms_id(), WEIGHT_SCALE, [3, 3, 3], CONSTANT)
    middle = world["ev"].coeff_to_slot_new(world["c"], down, _keys(world, down))
    up = pytroy.SlotToCoeffPlan(world["ctx"], world["enc"], middle.parms_id(), WEIGHT_SCALE, [3, 3, 3], 1.0 / CONSTANT)
    assert up.boundary_group() == 2 and [up.first_layer(g) for g in range(3)] == [0, 3, 6]
    gk = _keys(world, up)
    back = world["ev"].slot_to_coeff_new(middle, up, gk)
    err = float(np.max(np.abs(_slots(world, back) - world["z"])))
    bound = 4 * 6 * measured[1]
    print("slot_to_coeff(coeff_to_slot(z)) 3+3+3 twice: slot error %.3e, bound 4 x 6 x %.3e = %.3e" % (err, measured[1], bound))
    assert err <= bound
    dest = pytroy.Ciphertext()
    world["ev"].slot_to_coeff(encrypted=middle, plan=up, galois_keys=gk, destination=dest)
    assert dest.parms_id() == back.parms_id()


def test_groupings_agree(pytroy, world, measured):
    """(c) nine groups of one layer against three of three, and the default grouping is the latter: each within its bound of the truth, hence
    within the sum of the bounds of each other"""
    ones = pytroy.CoeffToSlotPlan(world["ctx"], world["enc"], world["c"].parms_id(), WEIGHT_SCALE, [1] * 9)
    threes = pytroy.CoeffToSlotPlan(world["ctx"], world["enc"], world["c"].parms_id(), WEIGHT_SCALE)
    assert threes.layers_per_group() == [3, 3, 3] == pytroy.default_layers_per_group(9) and ones.levels() == 9
    gk = _keys(world, ones, threes)
    a, b = _slots(world, world["ev"].coeff_to_slot_new(world["c"], ones, gk)), _slots(world, world["ev"].coeff_to_slot_new(world["c"], threes, gk))
    ea, eb, diff = (float(np.max(np.abs(x))) for x in (a - world["w"], b - world["w"], a - b))
    print("coeff_to_slot 1 x 9: error %.3e (%d rotations), 3 + 3 + 3: error %.3e (%d rotations), difference %.3e; per-group figure %.3e"
          % (ea, ones.rotations(), eb, threes.rotations(), diff, measured[0]))
    assert ea <= 4 * 9 * measured[0] and eb <= 4 * 3 * measured[0]
    assert diff <= 4 * (9 + 3) * measured[0]


def test_refusals(pytroy, world):
    ctx, enc, ev, c = world["ctx"], world["enc"], world["ev"], world["c"]
    plan = pytroy.CoeffToSlotPlan(ctx, enc, c.parms_id(), WEIGHT_SCALE, [5, 4])
    back = pytroy.SlotToCoeffPlan(ctx, enc, c.parms_id(), WEIGHT_SCALE, [5, 4])
    gk = _keys(world, plan, back)
    # an operand at another level than the plan's
    lower = ev.mod_switch_to_next_new(c)
    with pytest.raises(ValueError, match=r"\[Evaluator::coeff_to_slot\].*level"):
        ev.coeff_to_slot_new(lower, plan, gk)
    with pytest.raises(ValueError, match=r"\[Evaluator::slot_to_coeff\].*level"):
        ev.slot_to_coeff_new(lower, back, gk)
    # a context that is not CKKS
    _, encoder, kg3, encryptor3, _, ev3 = _batching(pytroy, pytroy.SchemeType.BFV, 7)
    c3 = encryptor3.encrypt_asymmetric_new(encoder.encode_simd_new([1, 2, 3]))
    gk3 = kg3.create_galois_keys_from_steps([1], False)
    with pytest.raises(ValueError, match=r"\[Evaluator::coeff_to_slot\].*CKKS"):
        ev3.coeff_to_slot_new(c3, plan, gk3)
    with pytest.raises(ValueError, match=r"\[Evaluator::slot_to_coeff\].*CKKS"):
        ev3.slot_to_coeff_new(c3, back, gk3)
    # sparse packing (n below the slot count) is out of scope: a CKKS context of another ring degree is refused by name
    ctx2, enc2, kg2, encryptor2, _, ev2 = _ckks(pytroy, 4096, (36, 36, 37))
    c2 = encryptor2.encrypt_asymmetric_new(enc2.encode_complex64_simd_new([1.0, 2.0], None, SCALE))
    with pytest.raises(ValueError, match=r"\[Evaluator::coeff_to_slot\].*Sparse packing"):
        ev2.coeff_to_slot_new(c2, plan, kg2.create_galois_keys_from_steps([1], False))
    # the constructors' own
    for cls, name in ((pytroy.CoeffToSlotPlan, "CoeffToSlotPlan"), (pytroy.SlotToCoeffPlan, "SlotToCoeffPlan")):
        with pytest.raises(ValueError, match=r"\[%s::%s\].*sum to log2 n" % (name, name)):
            cls(ctx, enc, c.parms_id(), WEIGHT_SCALE, [3, 3])
        with pytest.raises(ValueError, match=r"\[%s::%s\].*at least one layer" % (name, name)):
            cls(ctx, enc, c.parms_id(), WEIGHT_SCALE, [9, 0])
        with pytest.raises(ValueError, match=r"\[%s::%s\].*constant" % (name, name)):
            cls(ctx, enc, c.parms_id(), WEIGHT_SCALE, [3, 3, 3], 0.0)
        with pytest.raises(ValueError, match=r"\[%s::%s\].*fewer levels" % (name, name)):
            cls(ctx, enc, ctx.last_parms_id(), WEIGHT_SCALE, [9])
    bfv = pytroy.HeContext(_params(pytroy, pytroy.SchemeType.BFV, 4096, [36, 36, 37]), True, pytroy.SecurityLevel.Nil, 7)
    bfv.to_device_inplace()
    with pytest.raises(ValueError, match=r"\[CoeffToSlotPlan::CoeffToSlotPlan\].*CKKS"):
        pytroy.CoeffToSlotPlan(bfv, enc, bfv.first_parms_id(), WEIGHT_SCALE)
    with pytest.raises(ValueError, match=r"\[SlotToCoeffPlan::SlotToCoeffPlan\].*parms_id"):
        pytroy.SlotToCoeffPlan(bfv, enc, c.parms_id(), WEIGHT_SCALE)
