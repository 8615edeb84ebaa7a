"""troy::BootstrapPlan, Evaluator::bootstrap, split_real_imag / join_real_imag and eval_mod_batched (additions) through pytroy: CKKS N = 1024, K = 64,
a 60-bit q0, seventeen 50-bit working primes and a 60-bit special prime, D = 2^50, degree 79 with 3 double angles (tests/test_bootstrap_spec.py confirms
the choice): levels 3 + (7 + 3) + 3 = 16, seventeen levels in the chain, so the result keeps one level to spend.

Tolerance of the bootstrap.  Measured in the same run: e_ref is the largest slot error of the staged form (tests/bootstrap_staged.py: mod_raise,
coeff_to_slot, complex_conjugate, add / sub, multiply_plain by 1 and i with rescale_to_next, two eval_mod calls, multiply_plain by 1 and i, add,
slot_to_coeff) on a chain with two more primes, same message, same K, degree, double angles, groups and scales.  bootstrap must stay within 2 x e_ref:
the two forms share every noise source but two roundings and draw independent key-switch noise; a factor 2 between two maxima over 512 slots of one
distribution is rare, a wrong sign, constant or level shows as an error of order 1.  The product with a fresh ciphertext is held against the same product
of the staged result in the same way.  The test prints every figure (DESIGN 4.5o records one run).
"""
import numpy as np
import pytest

from test_gpu_hoist_api import _params, pytroy  # noqa: F401  (the module's fixture and parameter helper)
from test_gpu_linear_transform_api import _ckks
from bootstrap_staged import Staged

pytestmark = pytest.mark.gpu

N, SLOTS = 1024, 512
BITS = (60,) + (50,) * 17 + (60,)
BITS_STAGED = (60,) + (50,) * 19 + (60,)      # two more primes: the division and the multiplication by i each spend a level
DELTA = float(1 << 50)
K, DEGREE, DOUBLE_ANGLES = 64, 79, 3


@pytest.fixture(scope="module")
def world(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy, N, BITS)
    rng = np.random.default_rng(2026)
    z = rng.uniform(-1, 1, SLOTS) + 1j * rng.uniform(-1, 1, SLOTS)
    z /= np.maximum(np.abs(z), 1.0)
    z.setflags(write=False)
    plan = pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, DOUBLE_ANGLES, [3, 3, 3], [3, 3, 3], float(1 << 50))
    gk = kg.create_galois_keys_from_steps(plan.rotation_steps(), False)       # from rotation_steps() alone
    rk = kg.create_relin_keys(False)
    yield {"ctx": ctx, "enc": enc, "kg": kg, "encryptor": encryptor, "dec": dec, "ev": ev, "z": z, "plan": plan, "gk": gk, "rk": rk}
    pytroy.MemoryPool.destroy_global_pool()


def _encrypt(world, values, scale=DELTA):
    return world["encryptor"].encrypt_asymmetric_new(world["enc"].encode_complex64_simd_new([complex(v) for v in values], None, scale))


def _slots(world, ct):
    return np.asarray(world["enc"].decode_complex64_simd_new(world["dec"].decrypt_new(ct)))


def _lower(ev, c, limbs):
    while c.coeff_modulus_size() > limbs:
        c = ev.mod_switch_to_next_new(c)
    return c


def test_the_plan_counts_its_levels(pytroy, world):
    plan = world["plan"]
    down, up = plan.coeff_to_slot_plan(), plan.slot_to_coeff_plan()
    assert plan.eval_mod_depth() == pytroy.chebyshev_depth(DEGREE) + DOUBLE_ANGLES == 10
    assert plan.levels() == down.groups() + plan.eval_mod_depth() + up.groups() == 16
    assert plan.key_switches() == down.rotations() + 1 + up.rotations()
    assert plan.rotation_steps() == sorted(set(down.rotation_steps()) | set(up.rotation_steps()) | {0})
    assert plan.output_scale() == DELTA and plan.q0() / DELTA >= 2


def test_eval_mod_batched_equals_two_single_calls(pytroy, world):
    ev, rk = world["ev"], world["rk"]
    rng = np.random.default_rng(3)
    scale = float(1 << 50) / 4.0
    a = _lower(ev, _encrypt(world, rng.integers(-3, 4, SLOTS) + rng.uniform(-2.0 ** -8, 2.0 ** -8, SLOTS), scale), 9)
    b = _lower(ev, _encrypt(world, rng.integers(-3, 4, SLOTS) + rng.uniform(-2.0 ** -8, 2.0 ** -8, SLOTS), scale), 9)
    both = ev.eval_mod_new_batched([a, b], rk, 4.0, 15, 2)
    for got, single in zip(both, (ev.eval_mod_new(a, rk, 4.0, 15, 2), ev.eval_mod_new(b, rk, 4.0, 15, 2))):
        assert got.data() == single.data() and got.scale() == single.scale() and got.parms_id() == single.parms_id()
    cheb = ev.evaluate_chebyshev_new_batched([a, b], [0.5, 0.25, -0.125, 0.3, 0.0, 0.1], 4.0, rk)
    for got, x in zip(cheb, (a, b)):
        assert got.data() == ev.evaluate_chebyshev_new(x, [0.5, 0.25, -0.125, 0.3, 0.0, 0.1], 4.0, rk).data()
    with pytest.raises(ValueError, match=r"\[Evaluator::eval_mod_batched\].*parms_id"):
        ev.eval_mod_new_batched([a, ev.mod_switch_to_next_new(b)], rk, 4.0, 15, 2)
    with pytest.raises(ValueError, match=r"\[Evaluator::eval_mod_batched\].*Empty"):
        ev.eval_mod_new_batched([], rk, 4.0, 15, 2)


def test_split_real_imag_and_join(pytroy, world):
    ev, gk, z = world["ev"], world["gk"], world["z"]
    c = _encrypt(world, z)
    e_conj = float(np.max(np.abs(_slots(world, ev.complex_conjugate_new(c, gk)) - np.conj(z))))
    re2, im2 = ev.split_real_imag_new(c, gk)
    sign = np.where(np.arange(SLOTS) % 2 == 0, 1.0, -1.0)
    e_re = float(np.max(np.abs(_slots(world, re2) - 2 * z.real)))
    e_im = float(np.max(np.abs(_slots(world, im2) - sign * 2 * z.imag)))
    print("complex_conjugate error %.3e; split: real %.3e, imaginary %.3e (bound 4 x conjugate)" % (e_conj, e_re, e_im))
    assert e_re <= 4 * e_conj and e_im <= 4 * e_conj
    assert re2.parms_id() == c.parms_id() and re2.scale() == c.scale() and im2.scale() == c.scale()
    back = ev.join_real_imag_new(re2, im2)
    assert float(np.max(np.abs(_slots(world, back) - 2 * z))) <= 8 * e_conj
    with pytest.raises(ValueError, match=r"\[Evaluator::join_real_imag\].*parms_id"):
        ev.join_real_imag_new(re2, ev.mod_switch_to_next_new(im2))
    other = ev.mod_switch_to_next_new(im2)
    other.set_scale(im2.scale() * 2)
    with pytest.raises(ValueError, match=r"\[Evaluator::join_real_imag\].*scales"):
        ev.join_real_imag_new(ev.mod_switch_to_next_new(re2), other)
    with pytest.raises(ValueError, match=r"\[Evaluator::split_real_imag\].*two polynomials"):
        ev.split_real_imag_new(ev.multiply_new(c, c), gk)


@pytest.fixture(scope="module")
def reference(pytroy, world):
    """e_ref: the staged form on a chain with two more primes, same message; (slot error, error of one more product with a fresh ciphertext)"""
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy, N, BITS_STAGED)
    primes = [int(m.value()) for m in pytroy.CoeffModulus.create(N, list(BITS_STAGED))][:-1]
    staged = Staged(pytroy, ctx, enc, kg, primes, DELTA, K, DEGREE, DOUBLE_ANGLES, [3, 3, 3], [3, 3, 3], float(1 << 50))
    assert staged.levels == world["plan"].levels() + 2
    rk, z = kg.create_relin_keys(False), world["z"]
    encrypt = lambda v: encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(t) for t in v], None, DELTA))
    slots = lambda c: np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c)))
    out = staged.run(ev, rk, ev.mod_switch_to_new(encrypt(z), ctx.last_parms_id()))
    assert out.coeff_modulus_size() == 2 and out.scale() == DELTA
    e_ref = float(np.max(np.abs(slots(out) - z)))
    prod = ev.rescale_to_next_new(ev.relinearize_new(ev.multiply_new(out, _lower(ev, encrypt(np.conj(z)), 2)), rk))
    e_prod = float(np.max(np.abs(slots(prod) - z * np.conj(z))))
    print("staged form (two more primes): slot error e_ref %.3e, after one more product %.3e" % (e_ref, e_prod))
    del staged
    return e_ref, e_prod


def test_bootstrap_of_an_exhausted_ciphertext(pytroy, world, reference):
    ev, gk, rk, plan, z, ctx = world["ev"], world["gk"], world["rk"], world["plan"], world["z"], world["ctx"]
    e_ref, e_prod_ref = reference
    fresh = _encrypt(world, z)
    exhausted = ev.mod_switch_to_new(fresh, ctx.last_parms_id())
    assert exhausted.coeff_modulus_size() == 1
    out = ev.bootstrap_new(exhausted, plan, rk, gk)
    assert out.parms_id() == plan.output_parms_id() and out.scale() == DELTA and out.coeff_modulus_size() == len(BITS) - 1 - plan.levels() == 2
    err = float(np.max(np.abs(_slots(world, out) - z)))
    print("bootstrap: slot error %.3e, staged form e_ref %.3e, bound 2 x e_ref = %.3e" % (err, e_ref, 2 * e_ref))
    assert err <= 2 * e_ref
    # the spare level: one more product with a fresh ciphertext
    other = _lower(ev, _encrypt(world, np.conj(z)), 2)
    prod = ev.rescale_to_next_new(ev.relinearize_new(ev.multiply_new(out, other), rk))
    e_prod = float(np.max(np.abs(_slots(world, prod) - z * np.conj(z))))
    print("bootstrap, then one product: slot error %.3e, staged form %.3e, bound 2 x that" % (e_prod, e_prod_ref))
    assert e_prod <= 2 * e_prod_ref
    # from above the last level the call lowers the operand itself
    dest = pytroy.Ciphertext()
    ev.bootstrap(encrypted=_lower(ev, fresh, 3), plan=plan, relin_keys=rk, galois_keys=gk, destination=dest)
    assert dest.parms_id() == plan.output_parms_id() and float(np.max(np.abs(_slots(world, dest) - z))) <= 2 * e_ref


def test_refusals(pytroy, world):
    ctx, enc, ev, plan, gk, rk = world["ctx"], world["enc"], world["ev"], world["plan"], world["gk"], world["rk"]
    P = r"\[BootstrapPlan::BootstrapPlan\]"
    for args, word in (((DELTA, K, DEGREE, 9), "data levels"), ((DELTA, 0.0, DEGREE, 3), "half width"), ((DELTA, K, 0, 3), "degree"), ((DELTA, K, 128, 3), "degree"),
                       ((DELTA, K, DEGREE, 17), "double_angles"), ((0.0, K, DEGREE, 3), "message scale"), ((float("inf"), K, DEGREE, 3), "message scale"),
                       ((float(1 << 60), K, DEGREE, 3), "q0 / message_scale")):
        with pytest.raises(ValueError, match=P + ".*" + word):
            pytroy.BootstrapPlan(ctx, enc, *args)
    bfv = pytroy.HeContext(_params(pytroy, pytroy.SchemeType.BFV, 4096, [36, 36, 37]), True, pytroy.SecurityLevel.Nil, 7)
    bfv.to_device_inplace()
    with pytest.raises(ValueError, match=P + ".*CKKS"):
        pytroy.BootstrapPlan(bfv, enc, DELTA, K, DEGREE, 3)
    with pytest.raises(ValueError, match=P + ".*weight scale"):
        pytroy.BootstrapPlan(ctx, enc, DELTA, K, DEGREE, 3, [], [], 0.0)
    good = _encrypt(world, world["z"])
    with pytest.raises(ValueError, match=r"\[Evaluator::bootstrap\].*NTT form"):
        ev.bootstrap_new(ev.transform_from_ntt_new(good), plan, rk, gk)
    with pytest.raises(ValueError, match=r"\[Evaluator::bootstrap\].*two polynomials"):
        ev.bootstrap_new(ev.multiply_new(good, good), plan, rk, gk)
    with pytest.raises(ValueError, match=r"\[Evaluator::split_real_imag\].*NTT form"):
        ev.split_real_imag_new(ev.transform_from_ntt_new(good), gk)
    wrong = _encrypt(world, world["z"], DELTA * 2)
    with pytest.raises(ValueError, match=r"\[Evaluator::bootstrap\].*scale"):
        ev.bootstrap_new(wrong, plan, rk, gk)
