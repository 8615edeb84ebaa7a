"""Sparse secrets and the sparse-secret encapsulation of the CKKS bootstrap (additions; troy/bootstrap.h) through pytroy: the chain, the
message distribution and D = 2^50 of tests/test_gpu_bootstrap_api.py (N = 1024, a 60-bit q0, seventeen 50-bit primes, a 60-bit special prime).

Encapsulated bootstrap: the ephemeral secret has h = 32, K = ceil(BootstrapPlan.half_width_for(32)) = 12, degree 39 with 2 double angles -- the pair
tests/test_sparse_secret_spec.py derives from the float64 specification (depth 8: levels 3 + 8 + 3 = 14 against 16 of the dense plan).
Tolerance.  e_dense is the slot error of the existing bootstrap in the same run: same context, message and groupings, K = 64, degree 79, 3 double angles.
The encapsulated call must stay within 2 x e_dense: its two extra key switches act where the payload is D m against q0, and t against the whole chain, so
they add nothing visible, and the smaller K can only lower the amplified error; twice a same-run maximum over 512 slots is the margin of the existing
bootstrap test.  Control: the same K = 12 plan WITHOUT encapsulation, under the dense secret, is wrong by more than 0.1: I overflows K.
to_sparse at the last level: 4 x the slot error of complex_conjugate (a dense-key switch of the same shape) on the same ciphertext at the same level, the
margin of test_split_real_imag_and_join.  The tests print every figure (DESIGN 4.5p records one run).
"""
import math

import numpy as np
import pytest

from test_gpu_hoist_api import pytroy  # noqa: F401  (the module's fixture)
from test_gpu_linear_transform_api import _ckks
from test_gpu_bootstrap_api import BITS, DELTA, N, SLOTS
from test_gpu_bootstrap_api import DEGREE as DENSE_DEGREE, DOUBLE_ANGLES as DENSE_DOUBLE_ANGLES, K as DENSE_K
from test_sparse_secret_spec import ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, EPHEMERAL_WEIGHT

pytestmark = pytest.mark.gpu

GROUPS = [3, 3, 3]


@pytest.fixture(scope="module")
def world(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy, N, BITS)
    rng = np.random.default_rng(2026)
    z = rng.uniform(-1, 1, SLOTS) + 1j * rng.uniform(-1, 1, SLOTS)
    z /= np.maximum(np.abs(z), 1.0)
    z.setflags(write=False)
    k_small = math.ceil(pytroy.BootstrapPlan.half_width_for(EPHEMERAL_WEIGHT))
    dense = pytroy.BootstrapPlan(ctx, enc, DELTA, DENSE_K, DENSE_DEGREE, DENSE_DOUBLE_ANGLES, GROUPS, GROUPS, float(1 << 50))
    small = pytroy.BootstrapPlan(ctx, enc, DELTA, k_small, ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, GROUPS, GROUPS, float(1 << 50))
    gk = kg.create_galois_keys_from_steps(sorted(set(dense.rotation_steps()) | set(small.rotation_steps())), False)
    rk = kg.create_relin_keys(False)
    sparse_kg = pytroy.KeyGenerator.create_sparse(ctx, EPHEMERAL_WEIGHT)
    held = kg.create_sparse_encapsulation_keys(sparse_secret_key=sparse_kg.secret_key())      # the caller holds s'
    w = {"ctx": ctx, "enc": enc, "kg": kg, "encryptor": encryptor, "dec": dec, "ev": ev, "z": z, "dense": dense, "small": small, "k_small": k_small,
         "gk": gk, "rk": rk, "sparse_kg": sparse_kg, "held": held}
    yield w
    w.clear()
    pytroy.MemoryPool.destroy_global_pool()


def _encrypt(world, values, encryptor=None, scale=DELTA):
    plain = world["enc"].encode_complex64_simd_new([complex(v) for v in values], None, scale)
    return (encryptor or world["encryptor"]).encrypt_asymmetric_new(plain)


def _slots(world, ct, dec=None):
    return np.asarray(world["enc"].decode_complex64_simd_new((dec or world["dec"]).decrypt_new(ct)))


def _err(world, ct, want, dec=None):
    return float(np.max(np.abs(_slots(world, ct, dec) - want)))


def test_half_width_for(pytroy):
    f = pytroy.BootstrapPlan.half_width_for
    for h in (1, 32, 192, 1024, 16384):
        assert f(h) == pytest.approx(1.0 + 6.5 * math.sqrt((h + 1) / 12.0), rel=1e-15)
    assert math.ceil(f(32)) == 12 and math.ceil(f(1024)) == 62 and math.ceil(f(16384)) == 242


def test_sparse_key_generator(O, pytroy, world):
    ctx, ev, z, kgs = world["ctx"], world["ev"], world["z"], world["sparse_kg"]
    q = [int(m.value()) for m in pytroy.CoeffModulus.create(N, list(BITS))]
    sk = np.array(kgs.secret_key().data(), dtype=np.uint64).reshape(len(q), N)
    for i in (0, len(q) - 1):
        s = O.ntt_inverse(sk[i].copy(), 1, 1, 10, [O.NTTTables(10, q[i])])
        assert int(np.count_nonzero(s)) == EPHEMERAL_WEIGHT and set(np.unique(s).tolist()) <= {0, 1, q[i] - 1}
        assert i == 0 or np.array_equal(s != 0, first != 0)
        first = s
    # everything the key generator offers works on that secret: encrypt / decrypt, one multiply + relinearize + rescale.  Held against the same steps
    # under the dense generator in the same run: the same operations under independent noise (the sparse secret's e1 s term is the smaller one), so
    # 4 x, the margin of test_split_real_imag_and_join
    def round_trip(kg, encryptor, dec):
        c = _encrypt(world, z, encryptor)
        prod = ev.rescale_to_next_new(ev.relinearize_new(ev.multiply_new(c, _encrypt(world, np.conj(z), encryptor)), kg.create_relin_keys(False)))
        return _err(world, c, z, dec), _err(world, prod, z * np.conj(z), dec)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kgs.create_public_key(False))
    e_fresh, e_prod = round_trip(kgs, encryptor, pytroy.Decryptor(ctx, kgs.secret_key()))
    d_fresh, d_prod = round_trip(world["kg"], world["encryptor"], world["dec"])
    print("sparse secret h = %d: fresh slot error %.3e (dense secret %.3e), after multiply + relinearize + rescale %.3e (dense %.3e); bound 4 x dense"
          % (EPHEMERAL_WEIGHT, e_fresh, d_fresh, e_prod, d_prod))
    assert e_fresh <= 4 * d_fresh and e_prod <= 4 * d_prod
    # a second generator draws another secret (the context's generator moved on)
    other = np.array(pytroy.KeyGenerator.create_sparse(ctx, EPHEMERAL_WEIGHT).secret_key().data(), dtype=np.uint64)
    assert not np.array_equal(other.reshape(len(q), N), sk)


def test_to_sparse_at_the_last_level(pytroy, world):
    ctx, ev, z, gk, held = world["ctx"], world["ev"], world["z"], world["gk"], world["held"]
    exhausted = ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id())
    assert exhausted.coeff_modulus_size() == 1
    e_conj = _err(world, ev.complex_conjugate_new(exhausted, gk), np.conj(z))
    switched = ev.apply_keyswitching_new(exhausted, held.to_sparse)
    e_sparse = _err(world, switched, z, pytroy.Decryptor(ctx, world["sparse_kg"].secret_key()))
    e_wrong_key = _err(world, switched, z)
    print("last level: complex_conjugate (dense key switch) %.3e, to_sparse then decrypt under s' %.3e (bound 4 x), under s %.3e" % (e_conj, e_sparse, e_wrong_key))
    assert e_sparse <= 4 * e_conj
    assert e_wrong_key > 0.1                      # it really is under s' now
    assert held.hamming_weight == EPHEMERAL_WEIGHT


def test_to_sparse_keeps_only_the_rows_of_the_last_level(pytroy, world):
    held, limbs = world["held"], len(BITS)
    assert held.digit_count() == limbs - 1 and held.to_sparse.parms_id() == world["ctx"].key_parms_id() == held.to_dense.parms_id()
    for digit in range(held.digit_count()):
        words = held.obtain_data(True, digit).reshape(2, limbs, N)
        for poly in range(2):
            for limb in range(limbs):
                kept = digit == 0 and limb in (0, limbs - 1)
                nonzero = int(np.count_nonzero(words[poly, limb]))
                assert (nonzero > N // 2) if kept else (nonzero == 0), (digit, poly, limb, nonzero)
        assert int(np.count_nonzero(held.obtain_data(False, digit))) > N * limbs          # to_dense is an ordinary key
    # save_seed never reaches to_sparse
    seeded = world["kg"].create_sparse_encapsulation_keys(sparse_secret_key=world["sparse_kg"].secret_key(), save_seed=True)
    assert int(np.count_nonzero(seeded.obtain_data(True, 0).reshape(2, limbs, N)[1, 0])) > N // 2       # c1 is there, not a seed


@pytest.fixture(scope="module")
def dense_error(world):
    """e_dense: the existing bootstrap, dense secret, K = 64, degree 79, 3 double angles, same context and message"""
    ev, ctx, z = world["ev"], world["ctx"], world["z"]
    exhausted = ev.mod_switch_to_new(_encrypt(world, z), ctx.last_parms_id())
    out = ev.bootstrap_new(exhausted, world["dense"], world["rk"], world["gk"])
    return exhausted, _err(world, out, z)


def test_encapsulated_bootstrap(pytroy, world, dense_error):
    ev, z, gk, rk, small, dense = world["ev"], world["z"], world["gk"], world["rk"], world["small"], world["dense"]
    exhausted, e_dense = dense_error
    assert world["k_small"] == 12 and small.levels() == 14 < dense.levels() == 16
    # the ephemeral form: s' is drawn inside and dropped
    keys = world["kg"].create_sparse_encapsulation_keys(EPHEMERAL_WEIGHT)
    assert keys.hamming_weight == EPHEMERAL_WEIGHT
    out = ev.bootstrap_new(exhausted, small, rk, gk, encapsulation_keys=keys)
    assert out.parms_id() == small.output_parms_id() and out.scale() == DELTA and out.coeff_modulus_size() == len(BITS) - 1 - small.levels() == 4
    e_new = _err(world, out, z)
    # the caller-held form, into a destination, from above the last level
    dest = pytroy.Ciphertext()
    high = _encrypt(world, z)
    while high.coeff_modulus_size() > 3:
        high = ev.mod_switch_to_next_new(high)
    ev.bootstrap(encrypted=high, plan=small, relin_keys=rk, galois_keys=gk, encapsulation_keys=world["held"], destination=dest)
    e_held = _err(world, dest, z)
    print("encapsulated bootstrap (h = %d, K = %d, degree %d, %d double angles, %d levels): slot error %.3e (ephemeral s'), %.3e (held s'); "
          "dense bootstrap (K = %d, degree %d, %d double angles, %d levels) e_dense %.3e, bound 2 x e_dense = %.3e"
          % (EPHEMERAL_WEIGHT, world["k_small"], ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, small.levels(), e_new, e_held,
             DENSE_K, DENSE_DEGREE, DENSE_DOUBLE_ANGLES, dense.levels(), e_dense, 2 * e_dense))
    assert dest.parms_id() == small.output_parms_id() and dest.scale() == DELTA
    assert e_new <= 2 * e_dense and e_held <= 2 * e_dense


def test_small_k_without_encapsulation_is_wrong(world, dense_error):
    """the control: the dense secret's I does not fit K = 12 (a wrong answer, not a fault)"""
    exhausted, e_dense = dense_error
    out = world["ev"].bootstrap_new(exhausted, world["small"], world["rk"], world["gk"])
    e_control = _err(world, out, world["z"])
    print("K = %d under the dense secret, no encapsulation: slot error %.3e (e_dense %.3e)" % (world["k_small"], e_control, e_dense))
    assert e_control > 0.1


def test_refusals(pytroy, world):
    ctx, ev, kg, small, rk, gk = world["ctx"], world["ev"], world["kg"], world["small"], world["rk"], world["gk"]
    for h in (0, N + 1):
        with pytest.raises(ValueError, match=r"\[KeyGenerator::create_sparse\]"):
            pytroy.KeyGenerator.create_sparse(ctx, h)
        with pytest.raises(ValueError, match=r"\[KeyGenerator::create_sparse_encapsulation_keys\]"):
            kg.create_sparse_encapsulation_keys(h)
    good = _encrypt(world, world["z"])
    with pytest.raises(ValueError, match=r"\[Evaluator::bootstrap\].*empty"):
        ev.bootstrap_new(good, small, rk, gk, encapsulation_keys=pytroy.SparseEncapsulationKeys())
    # keys of another context: its key level has another parms_id
    other_ctx, _, other_kg, _, _, _ = _ckks(pytroy, N, BITS[:-2] + (60,))
    foreign = other_kg.create_sparse_encapsulation_keys(EPHEMERAL_WEIGHT)
    with pytest.raises(ValueError, match=r"\[Evaluator::bootstrap\].*parms_id"):
        ev.bootstrap_new(good, small, rk, gk, encapsulation_keys=foreign)
    with pytest.raises(ValueError, match=r"\[Evaluator::bootstrap\].*scale"):
        ev.bootstrap_new(_encrypt(world, world["z"], scale=DELTA * 2), small, rk, gk, encapsulation_keys=world["held"])
