"""troy::LinearTransform and Evaluator::linear_transform (additions) through pytroy: CKKS N = 8192 {40,40,40,40}, scale 2^30, the context of
tests/test_gpu_bsgs_double_api.py.  The transform's device-encoded weights are the hand-encoded ones word for word, the result has the orientation of
M z, its key list suffices, and the refusals carry the method's name."""
import random

import numpy as np
import pytest

import linear_transform_spec as S
from test_gpu_hoist_api import _batching, _params, pytroy  # noqa: F401  (the module's fixture and parameter helpers)
from test_gpu_weighted_hoist_api import _disc

pytestmark = pytest.mark.gpu

SCALE = float(1 << 30)


def _ckks(pytroy, n=8192, bits=(40, 40, 40, 40)):
    p = _params(pytroy, pytroy.SchemeType.CKKS, n, list(bits))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil if n < 8192 else pytroy.SecurityLevel.Classical128, 99)
    ctx.to_device_inplace()
    enc = pytroy.CKKSEncoder(ctx)
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    return ctx, enc, kg, encryptor, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx)


def test_identical_words_and_keys(pytroy, dev):
    """n = slots, the diagonals 0..15, baby_count = 4: the same weights in, the same call -- no tolerance"""
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy)
    slots = enc.slot_count()
    rnd = random.Random(8)
    z = _disc(rnd, slots)
    diag = {k: np.array(_disc(rnd, slots)) for k in range(16)}
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, SCALE))
    lt = pytroy.LinearTransform(ctx, enc, slots, c.parms_id(), SCALE, diag, baby_count=4)
    babies, giants = S.split(sorted(diag), slots, 4)
    assert (babies, giants) == ([0, 1, 2, 3], [0, 4, 8, 12])
    assert lt.n() == slots and lt.baby_count() == 4 and lt.scale() == SCALE and lt.parms_id() == c.parms_id()
    assert lt.baby_steps() == babies and lt.giant_steps() == giants
    # (iii) the key list is the specification's, and a key set made from it suffices
    assert lt.rotation_steps() == S.rotation_steps(sorted(diag), slots, 4) == [1, 2, 3, 4, 8, 12]
    gk = kg.create_galois_keys_from_steps(lt.rotation_steps(), False)
    # the weights by hand: the specification's pre-rotated diagonals through the existing batched encoder
    where, pairs = S.pairs(sorted(diag), slots, 4)
    values = S.values_of(np.stack([diag[k] for k in sorted(diag)]), pairs, slots, 2 * slots, False)
    flat = enc.encode_complex64_simd_new_batched([v.tolist() for v in values], ctx.key_parms_id(), SCALE)
    pw = [[None] * len(babies) for _ in giants]
    for t, (g, b) in enumerate(where):
        pw[g][b] = flat[t]
    mine = lt.weights()
    for g in range(len(giants)):
        for b in range(len(babies)):
            w = mine[g][b]
            assert w.is_ntt_form() and w.parms_id() == ctx.key_parms_id() and w.scale() == SCALE
            assert w.data() == pw[g][b].data(), (g, b)
    # (i) identical words, both hoisting levels
    got = ev.linear_transform_new(c, lt, gk)
    assert got.data() == ev.rotate_bsgs_sum_double_hoisted_new(c, babies, giants, gk, pw).data()
    assert got.is_ntt_form() and got.parms_id() == c.parms_id() and got.scale() == c.scale() * SCALE
    single = ev.linear_transform_single_hoisted_new(c, lt, gk)
    assert single.data() == ev.rotate_bsgs_sum_new(c, babies, giants, gk, pw).data()
    assert single.data() != got.data()
    dest = pytroy.Ciphertext()
    ev.linear_transform(c, lt, gk, dest)
    assert dest.data() == got.data()
    dest = pytroy.Ciphertext()
    ev.linear_transform_single_hoisted(encrypted=c, lt=lt, galois_keys=gk, destination=dest)
    assert dest.data() == single.data()
    pytroy.MemoryPool.destroy_global_pool()


def test_orientation_dense_sparse_packed(pytroy, dev):
    """a dense n = 16 transform on sparsely packed slots: M = permutation x unit-modulus phases, z on the unit disc, replicated.  Every slot within 2e-2 of
    M z: 10 x the 1.799e-03 DESIGN 4.5h records for this chain and scale with 16 diagonals; a wrong row, column or rotation sign errs by order 1.  The
    sparse constructor on the matrix's diagonals gives the dense one's words."""
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy)
    slots, n = enc.slot_count(), 16
    rnd = random.Random(21)
    perm = list(range(n))
    rnd.shuffle(perm)
    assert any(perm[i] != i for i in range(n))
    M = np.zeros((n, n), dtype=np.complex128)
    for i in range(n):
        M[i, perm[i]] = np.exp(2j * np.pi * rnd.random())
    z = np.array(_disc(rnd, n))
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(np.tile(z, slots // n).tolist(), None, SCALE))
    lt = pytroy.LinearTransform(ctx, enc, n, c.parms_id(), SCALE, M)
    assert lt.baby_steps() == [0, 1, 2, 3] and lt.giant_steps() == [0, 4, 8, 12] and lt.rotation_steps() == [1, 2, 3, 4, 8, 12]
    gk = kg.create_galois_keys_from_steps(lt.rotation_steps(), False)
    want = np.tile(M @ z, slots // n)
    errors = []
    for got in (ev.linear_transform_new(c, lt, gk), ev.linear_transform_single_hoisted_new(c, lt, gk)):
        errors.append(float(np.max(np.abs(np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(got))) - want))))
    print("linear transform n = 16 sparse-packed: max error %.3e double-hoisted, %.3e single-hoisted (bound 2e-2)" % tuple(errors))
    assert max(errors) <= 2e-2
    by_diagonals = pytroy.LinearTransform(ctx, enc, n, c.parms_id(), SCALE, S.diagonals_of(M))
    a, b = lt.weights(), by_diagonals.weights()
    assert all(a[g][k].data() == b[g][k].data() for g in range(4) for k in range(4))
    pytroy.MemoryPool.destroy_global_pool()


def test_sparse_diagonals_leave_null_weights(pytroy, dev):
    """present {0, 1, 5, 8, 15} of n = 16: the split of the specification, null weights where G + B is absent, and the product"""
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy)
    slots, n = enc.slot_count(), 16
    rnd = random.Random(3)
    present = [0, 1, 5, 8, 15]
    diag = {k: np.array(_disc(rnd, n)) for k in present}
    z = np.array(_disc(rnd, n))
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(np.tile(z, slots // n).tolist(), None, SCALE))
    lt = pytroy.LinearTransform(ctx, enc, n, c.parms_id(), SCALE, diag)
    assert (lt.baby_steps(), lt.giant_steps()) == S.split(present, n) and lt.rotation_steps() == S.rotation_steps(present, n)
    where, _ = S.pairs(present, n)
    w = lt.weights()
    assert [(g, b) for g in range(len(w)) for b in range(len(w[g])) if w[g][b] is not None] == where
    gk = kg.create_galois_keys_from_steps(lt.rotation_steps(), False)
    want = np.tile(sum(diag[k] * S.rot(z, k) for k in present), slots // n)
    got = np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(ev.linear_transform_new(c, lt, gk))))
    assert np.max(np.abs(got - want)) <= 2e-2
    pytroy.MemoryPool.destroy_global_pool()


def test_refusals(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy)
    slots = enc.slot_count()
    rnd = random.Random(1)
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(_disc(rnd, slots), None, SCALE))
    lt = pytroy.LinearTransform(ctx, enc, slots, c.parms_id(), SCALE, {0: np.array(_disc(rnd, slots)), 1: np.array(_disc(rnd, slots))})
    gk = kg.create_galois_keys_from_steps(lt.rotation_steps(), False)
    assert ev.linear_transform_new(c, lt, gk).parms_id() == c.parms_id()
    # an operand at another level than the transform's
    lower = ev.mod_switch_to_next_new(c)
    for call in (ev.linear_transform_new, ev.linear_transform_single_hoisted_new):
        with pytest.raises(ValueError, match=r"\[Evaluator::linear_transform\].*level"):
            call(lower, lt, gk)
    # a transform larger than the slot count of the evaluator's context (n = 4096 on N = 4096)
    ctx2, enc2, kg2, encryptor2, _, ev2 = _ckks(pytroy, 4096, (36, 36, 37))
    c2 = encryptor2.encrypt_asymmetric_new(enc2.encode_complex64_simd_new([1.0, 2.0], None, SCALE))
    gk2 = kg2.create_galois_keys_from_steps([1], False)
    with pytest.raises(ValueError, match=r"\[Evaluator::linear_transform\].*does not divide the slot count"):
        ev2.linear_transform_new(c2, lt, gk2)
    # a context that is not CKKS
    t, encoder, kg3, encryptor3, _, ev3 = _batching(pytroy, pytroy.SchemeType.BFV, 7)
    c3 = encryptor3.encrypt_asymmetric_new(encoder.encode_simd_new([1, 2, 3]))
    gk3 = kg3.create_galois_keys_from_steps([1], False)
    with pytest.raises(ValueError, match=r"\[Evaluator::linear_transform\].*CKKS"):
        ev3.linear_transform_new(c3, lt, gk3)
    # the constructor's own
    with pytest.raises(ValueError, match=r"\[LinearTransform::LinearTransform\].*power of two"):
        pytroy.LinearTransform(ctx, enc, 12, c.parms_id(), SCALE, {0: np.zeros(12, dtype=np.complex128)})
    with pytest.raises(ValueError, match=r"\[LinearTransform::LinearTransform\].*n values"):
        pytroy.LinearTransform(ctx, enc, 16, c.parms_id(), SCALE, {0: np.zeros(15, dtype=np.complex128)})
    with pytest.raises(ValueError, match=r"\[LinearTransform::LinearTransform\].*below n"):
        pytroy.LinearTransform(ctx, enc, 16, c.parms_id(), SCALE, {16: np.zeros(16, dtype=np.complex128)})
    with pytest.raises(ValueError, match=r"\[LinearTransform::LinearTransform\].*n \* n"):
        pytroy.LinearTransform(ctx, enc, 16, c.parms_id(), SCALE, np.zeros((16, 15), dtype=np.complex128))
    pytroy.MemoryPool.destroy_global_pool()
