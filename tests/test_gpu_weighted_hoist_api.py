"""Evaluator::rotate_weighted_sum(s) / apply_galois_weighted_sum(s) (additions: the diagonal method, plaintext weights applied before the one
division by the special prime) through pytroy, with genuine Galois keys: the results decrypt to SUM_k w_k * rotate(v, k), and the refusals."""
import random

import pytest

from test_gpu_hoist_api import _batching, _params, pytroy  # noqa: F401  (the module's fixture and parameter helpers)

pytestmark = pytest.mark.gpu


def test_bfv_weighted_rotations(pytroy, dev):
    n = 4096
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BFV, 7)
    ctx = ev.context()
    key_id = ctx.key_parms_id()
    row = n // 2
    rnd = random.Random(14)
    v = [rnd.randrange(t) for _ in range(n)]
    rot = lambda k: [v[(i + k) % row] for i in range(row)] + [v[row + (i + k) % row] for i in range(row)]
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v))
    steps = [0, 1, 2, 5]
    gk = kg.create_galois_keys_from_steps([1, 2, 5], False)
    w = [[rnd.randrange(t) for _ in range(n)] for _ in steps]
    weight = lambda x: ev.transform_plain_to_ntt_new(encoder.encode_simd_new(x), key_id)
    pw = [weight(x) for x in w]
    assert all(p.is_ntt_form() and p.parms_id() == key_id for p in pw)
    dec = lambda c: encoder.decode_simd_new(decryptor.decrypt_new(c)).tolist()
    want = lambda ks: [sum(w[k][i] * rot(steps[k])[i] for k in ks) % t for i in range(n)]
    got = ev.rotate_weighted_sum_new(ct, steps, gk, pw)
    assert got.polynomial_count() == 2 and got.parms_id() == ct.parms_id() and not got.is_ntt_form()
    assert dec(got) == want(range(4))
    # the spelling with a destination and keyword arguments; the plural form with an absent term; Galois elements (3 = one step, 1 = identity)
    dest = pytroy.Ciphertext()
    ev.rotate_weighted_sum(encrypted=ct, steps=steps, galois_keys=gk, weights=pw, destination=dest)
    assert dest.data() == got.data()
    two = ev.rotate_weighted_sums_new(ct, steps, gk, [pw, [None, pw[1], None, pw[3]]])
    assert len(two) == 2 and two[0].data() == got.data() and dec(two[1]) == want([1, 3])
    dests = [pytroy.Ciphertext(), pytroy.Ciphertext()]
    ev.rotate_weighted_sums(ct, steps, gk, [pw, [None, pw[1], None, pw[3]]], dests)
    assert [d.data() for d in dests] == [c.data() for c in two]
    assert ev.apply_galois_weighted_sum_new(ct, [1, 3], gk, pw[:2]).data() == ev.rotate_weighted_sum_new(ct, [0, 1], gk, pw[:2]).data()
    assert ev.apply_galois_weighted_sums_new(ct, [3], gk, [[pw[1]]])[0].data() == ev.rotate_weighted_sum_new(ct, [1], gk, [pw[1]]).data()
    # refusals, each with the method's name
    with pytest.raises(ValueError, match=r"rotate_weighted_sum\].*Galois key not present"):
        ev.rotate_weighted_sum_new(ct, [1, 3], gk, pw[:2])                   # no NAF chain
    with pytest.raises(ValueError, match=r"rotate_weighted_sum\].*key level"):
        ev.rotate_weighted_sum_new(ct, [1], gk, [ev.transform_plain_to_ntt_new(encoder.encode_simd_new(w[0]), ct.parms_id())])
    with pytest.raises(ValueError, match=r"rotate_weighted_sum\].*NTT form"):
        ev.rotate_weighted_sum_new(ct, [1], gk, [encoder.encode_simd_new(w[0])])
    with pytest.raises(ValueError, match=r"rotate_weighted_sums\].*slot has no weight"):
        ev.rotate_weighted_sums_new(ct, [1, 2], gk, [pw[:2], [None, None]])
    with pytest.raises(ValueError, match=r"apply_galois_weighted_sums\]"):
        ev.apply_galois_weighted_sums_new(ct, [3], gk, [])
    with pytest.raises(ValueError, match=r"apply_galois_weighted_sum\]"):
        ev.apply_galois_weighted_sum_new(ct, [3, 9], gk, pw[:1])             # one weight per term
    pytroy.MemoryPool.destroy_global_pool()


def test_bgv_is_refused(pytroy, dev):
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BGV, 17)
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new([1, 2, 3]))
    gk = kg.create_galois_keys_from_steps([1], False)
    pw = ev.transform_plain_to_ntt_new(encoder.encode_simd_new([1, 1, 1]), ct.parms_id())
    for name, call in (("rotate_weighted_sum", lambda: ev.rotate_weighted_sum_new(ct, [1], gk, [pw])),
                       ("rotate_weighted_sums", lambda: ev.rotate_weighted_sums_new(ct, [1], gk, [[pw]])),
                       ("apply_galois_weighted_sum", lambda: ev.apply_galois_weighted_sum_new(ct, [3], gk, [pw])),
                       ("apply_galois_weighted_sums", lambda: ev.apply_galois_weighted_sums_new(ct, [3], gk, [[pw]]))):
        with pytest.raises(ValueError, match=name + r"\].*BGV"):
            call()
    pytroy.MemoryPool.destroy_global_pool()


def _ckks(pytroy, steps):
    p = _params(pytroy, pytroy.SchemeType.CKKS, 8192, [40, 40, 40, 40])
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Classical128, 99)
    ctx.to_device_inplace()
    enc = pytroy.CKKSEncoder(ctx)
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    return ctx, enc, kg.create_galois_keys_from_steps(steps, False), encryptor, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx)


def _disc(rnd, count):
    out = []
    while len(out) < count:
        z = complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1))
        if abs(z) <= 1:
            out.append(z)
    return out


def test_ckks_weighted_rotations(pytroy, dev):
    """the parameters and scale of the project's CKKS rotate check; its per-rotation tolerance 2e-2, summed over the terms (|w| <= 1)"""
    steps = [0, 1, 2, 5]
    ctx, enc, gk, encryptor, dec, ev = _ckks(pytroy, [1, 2, 5])
    scale = float(1 << 30)
    rnd = random.Random(4)
    slots = enc.slot_count()
    z = _disc(rnd, slots)
    w = [_disc(rnd, slots) for _ in steps]
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, scale))
    pw = [enc.encode_complex64_simd_new(x, ctx.key_parms_id(), scale) for x in w]
    assert all(p.is_ntt_form() and p.parms_id() == ctx.key_parms_id() for p in pw)
    got = ev.rotate_weighted_sum_new(c, steps, gk, pw)
    assert got.is_ntt_form() and got.parms_id() == c.parms_id() and got.scale() == c.scale() * scale
    r = enc.decode_complex64_simd_new(dec.decrypt_new(got)).tolist()
    err = max(abs(r[i] - sum(w[k][i] * z[(i + st) % slots] for k, st in enumerate(steps))) for i in range(slots))
    print("ckks weighted sum: max error %.3e (bound %.1e)" % (err, len(steps) * 2e-2))
    assert err < len(steps) * 2e-2
    # a weight with another scale is refused
    with pytest.raises(ValueError, match=r"rotate_weighted_sum\].*different scales"):
        ev.rotate_weighted_sum_new(c, [1, 2], gk, [pw[1], enc.encode_complex64_simd_new(w[2], ctx.key_parms_id(), float(1 << 20))])
    pytroy.MemoryPool.destroy_global_pool()


def test_ckks_bsgs_product(pytroy, dev):
    """an 8-diagonal product by baby steps [0, 1, 2, 3] and giant steps {0, 4}: the giant-step slot's weights are the diagonals rotated back by 4,
    its sum is rotated by 4 with the existing rotate_vector and added; it equals the direct 8-diagonal weighted sum and the plain product"""
    baby, giant = [0, 1, 2, 3], 4
    ctx, enc, gk, encryptor, dec, ev = _ckks(pytroy, [1, 2, 3, 4, 5, 6, 7])
    scale = float(1 << 30)
    rnd = random.Random(6)
    slots = enc.slot_count()
    z = _disc(rnd, slots)
    diag = [_disc(rnd, slots) for _ in range(8)]
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, scale))
    plain = lambda x: enc.encode_complex64_simd_new(x, ctx.key_parms_id(), scale)
    back = lambda x, g: [x[(i - g) % slots] for i in range(slots)]          # rot_g(back(x) * y) = x * rot_g(y)
    sums = ev.rotate_weighted_sums_new(c, baby, gk, [[plain(diag[k]) for k in baby], [plain(back(diag[giant + k], giant)) for k in baby]])
    bsgs = ev.add_new(sums[0], ev.rotate_vector_new(sums[1], giant, gk))
    direct = ev.rotate_weighted_sum_new(c, list(range(8)), gk, [plain(d) for d in diag])
    a = enc.decode_complex64_simd_new(dec.decrypt_new(bsgs)).tolist()
    b = enc.decode_complex64_simd_new(dec.decrypt_new(direct)).tolist()
    want = [sum(diag[k][i] * z[(i + k) % slots] for k in range(8)) for i in range(slots)]
    ea = max(abs(a[i] - want[i]) for i in range(slots))
    eb = max(abs(b[i] - want[i]) for i in range(slots))
    print("ckks bsgs: max error %.3e, direct %.3e (bound %.1e)" % (ea, eb, 8 * 2e-2))
    assert ea < 8 * 2e-2 and eb < 8 * 2e-2
    pytroy.MemoryPool.destroy_global_pool()
