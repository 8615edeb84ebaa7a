"""Evaluator::rotate_bsgs_sum / apply_galois_bsgs_sum / rotate_sum_each / apply_galois_sum_each (additions: the baby-step/giant-step linear
transform, giant steps summed before ONE division by the special prime) through pytroy, with genuine Galois keys: the results decrypt to
the matrix-vector product, and the refusals."""
import random

import pytest

from test_gpu_hoist_api import _batching, _params, pytroy  # noqa: F401  (the module's fixture and parameter helpers)
from test_gpu_weighted_hoist_api import _ckks, _disc

pytestmark = pytest.mark.gpu

BABY, GIANT = [0, 1, 2, 3], [0, 4, 8, 12]


def test_bfv_bsgs_product(pytroy, dev):
    """a random 16-diagonal matrix times an encrypted vector: diagonal d multiplies the rotation by d = giant + baby; the weight of (giant, baby)
    is that diagonal rotated back by the giant step"""
    n = 4096
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BFV, 7)
    key_id = ev.context().key_parms_id()
    row = n // 2
    rnd = random.Random(15)
    v = [rnd.randrange(t) for _ in range(n)]
    rows = lambda x, k: [x[(i + k) % row] for i in range(row)] + [x[row + (i + k) % row] for i in range(row)]
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v))
    gk = kg.create_galois_keys_from_steps([1, 2, 3, 4, 8, 12], False)
    diag = [[rnd.randrange(t) for _ in range(n)] for _ in range(16)]
    weight = lambda x: ev.transform_plain_to_ntt_new(encoder.encode_simd_new(x), key_id)
    pw = [[weight(rows(diag[g + b], -g)) for b in BABY] for g in GIANT]
    dec = lambda c: encoder.decode_simd_new(decryptor.decrypt_new(c)).tolist()
    rotated = [rows(v, d) for d in range(16)]
    want = [sum(diag[d][i] * rotated[d][i] for d in range(16)) % t for i in range(n)]
    got = ev.rotate_bsgs_sum_new(ct, BABY, GIANT, gk, pw)
    assert got.polynomial_count() == 2 and got.parms_id() == ct.parms_id() and not got.is_ntt_form()
    assert dec(got) == want
    # the spelling with a destination and keyword arguments; Galois elements (1 = the identity)
    dest = pytroy.Ciphertext()
    ev.rotate_bsgs_sum(encrypted=ct, baby_steps=BABY, giant_steps=GIANT, galois_keys=gk, weights=pw, destination=dest)
    assert dest.data() == got.data()
    assert ev.apply_galois_bsgs_sum_new(ct, [1, 3], [1, 3], gk, [pw[0][:2], pw[1][:2]]).data() == ev.rotate_bsgs_sum_new(ct, [0, 1], [0, 1], gk, [pw[0][:2], pw[1][:2]]).data()
    # the sum of rotations of four DIFFERENT ciphertexts
    vs = [[rnd.randrange(t) for _ in range(n)] for _ in range(4)]
    cts = [encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(x)) for x in vs]
    each = ev.rotate_sum_each_new(cts, GIANT, gk)
    assert each.parms_id() == ct.parms_id() and not each.is_ntt_form()
    assert dec(each) == [sum(rows(x, g)[i] for x, g in zip(vs, GIANT)) % t for i in range(n)]
    dest = pytroy.Ciphertext()
    ev.rotate_sum_each(encrypted=cts, steps=GIANT, galois_keys=gk, destination=dest)
    assert dest.data() == each.data()
    assert ev.apply_galois_sum_each_new(cts[:2], [1, 3], gk).data() == ev.rotate_sum_each_new(cts[:2], [0, 1], gk).data()
    # refusals, each with the method's name
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum\].*Galois key not present"):
        ev.rotate_bsgs_sum_new(ct, [0, 1], [0, 5], gk, [pw[0][:2], pw[1][:2]])          # no NAF chain
    with pytest.raises(ValueError, match=r"rotate_sum_each\].*Galois key not present"):
        ev.rotate_sum_each_new(cts[:2], [1, 5], gk)
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum\].*key level"):
        ev.rotate_bsgs_sum_new(ct, [1], [4], gk, [[ev.transform_plain_to_ntt_new(encoder.encode_simd_new(diag[0]), ct.parms_id())]])
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum\].*NTT form"):
        ev.rotate_bsgs_sum_new(ct, [1], [4], gk, [[encoder.encode_simd_new(diag[0])]])
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum\].*giant step has no weight"):
        ev.rotate_bsgs_sum_new(ct, [0, 1], [0, 4], gk, [pw[0][:2], [None, None]])
    with pytest.raises(ValueError, match=r"apply_galois_bsgs_sum\]"):
        ev.apply_galois_bsgs_sum_new(ct, [3], [9], gk, [])                               # one weight row per giant step
    with pytest.raises(ValueError, match=r"apply_galois_sum_each\]"):
        ev.apply_galois_sum_each_new(cts[:2], [3], gk)                                   # one ciphertext per element
    with pytest.raises(ValueError, match=r"rotate_sum_each\].*different levels"):
        ev.rotate_sum_each_new([cts[0], ev.mod_switch_to_next_new(cts[1])], [1, 2], gk)
    pytroy.MemoryPool.destroy_global_pool()


def test_bgv_is_refused(pytroy, dev):
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BGV, 17)
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new([1, 2, 3]))
    gk = kg.create_galois_keys_from_steps([1], False)
    pw = ev.transform_plain_to_ntt_new(encoder.encode_simd_new([1, 1, 1]), ct.parms_id())
    for name, call in (("rotate_bsgs_sum", lambda: ev.rotate_bsgs_sum_new(ct, [1], [1], gk, [[pw]])),
                       ("apply_galois_bsgs_sum", lambda: ev.apply_galois_bsgs_sum_new(ct, [3], [3], gk, [[pw]])),
                       ("rotate_sum_each", lambda: ev.rotate_sum_each_new([ct], [1], gk)),
                       ("apply_galois_sum_each", lambda: ev.apply_galois_sum_each_new([ct], [3], gk))):
        with pytest.raises(ValueError, match=name + r"\].*BGV"):
            call()
    pytroy.MemoryPool.destroy_global_pool()


def test_ckks_bsgs_product(pytroy, dev):
    """the same 16-diagonal product on complex slots, the weights from CKKSEncoder's batched device path at the key level.  The composed form
    (rotate_weighted_sums + rotate_vector + add, one division per giant step more) is measured against the float product in the same test:
    the one-call result's error must be within 4 x that -- the roundings happen at different points under the same kind of noise bound."""
    ctx, enc, gk, encryptor, dec, ev = _ckks(pytroy, [1, 2, 3, 4, 8, 12])
    scale = float(1 << 30)
    rnd = random.Random(8)
    slots = enc.slot_count()
    z = _disc(rnd, slots)
    diag = [_disc(rnd, slots) for _ in range(16)]
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, scale))
    back = lambda x, g: [x[(i - g) % slots] for i in range(slots)]          # rot_g(back(x) * y) = x * rot_g(y)
    flat = enc.encode_complex64_simd_new_batched([back(diag[g + b], g) for g in GIANT for b in BABY], ctx.key_parms_id(), scale)
    assert len(flat) == 16 and all(p.is_ntt_form() and p.parms_id() == ctx.key_parms_id() for p in flat)
    pw = [flat[4 * i:4 * i + 4] for i in range(4)]
    got = ev.rotate_bsgs_sum_new(c, BABY, GIANT, gk, pw)
    assert got.is_ntt_form() and got.parms_id() == c.parms_id() and got.scale() == c.scale() * scale
    sums = ev.rotate_weighted_sums_new(c, BABY, gk, pw)
    composed = sums[0]
    for s, g in zip(sums[1:], GIANT[1:]):
        composed = ev.add_new(composed, ev.rotate_vector_new(s, g, gk))
    want = [sum(diag[d][i] * z[(i + d) % slots] for d in range(16)) for i in range(slots)]
    a = enc.decode_complex64_simd_new(dec.decrypt_new(got)).tolist()
    b = enc.decode_complex64_simd_new(dec.decrypt_new(composed)).tolist()
    ea = max(abs(a[i] - want[i]) for i in range(slots))
    eb = max(abs(b[i] - want[i]) for i in range(slots))
    print("ckks bsgs: one call max error %.3e, composed %.3e (bound 4 x composed)" % (ea, eb))
    assert ea <= 4 * eb
    # the sum over different ciphertexts, and operands with different scales
    c2 = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(diag[0], None, scale))
    each = enc.decode_complex64_simd_new(dec.decrypt_new(ev.rotate_sum_each_new([c, c2], [0, 4], gk))).tolist()
    assert max(abs(each[i] - (z[i] + diag[0][(i + 4) % slots])) for i in range(slots)) < 2 * 2e-2      # the project's per-rotation tolerance, per term
    c3 = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(diag[0], None, float(1 << 20)))
    with pytest.raises(ValueError, match=r"rotate_sum_each\].*different scales"):
        ev.rotate_sum_each_new([c, c3], [0, 4], gk)
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum\].*different scales"):
        ev.rotate_bsgs_sum_new(c, [0, 1], [4], gk, [[pw[0][0], enc.encode_complex64_simd_new(diag[1], ctx.key_parms_id(), float(1 << 20))]])
    pytroy.MemoryPool.destroy_global_pool()
