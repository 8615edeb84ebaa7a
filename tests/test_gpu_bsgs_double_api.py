"""Evaluator::rotate_bsgs_sum_double_hoisted / apply_galois_bsgs_sum_double_hoisted (additions: the BSGS linear transform with the second
hoisting level, the inner c0 never divided) through pytroy, with genuine Galois keys: the results decrypt to the matrix-vector product and to
what rotate_bsgs_sum decrypts to, and the refusals carry the new names."""
import random

import pytest

from test_gpu_bsgs_api import BABY, GIANT
from test_gpu_hoist_api import _batching, _params, pytroy  # noqa: F401  (the module's fixture and parameter helpers)
from test_gpu_weighted_hoist_api import _ckks, _disc

pytestmark = pytest.mark.gpu


def test_bfv_bsgs_product(pytroy, dev):
    """a random 16-diagonal matrix times an encrypted vector over the slots modulo t: exactly the integer product, and exactly what
    rotate_bsgs_sum decrypts to (the ciphertext words differ)"""
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
    got = ev.rotate_bsgs_sum_double_hoisted_new(ct, BABY, GIANT, gk, pw)
    assert got.polynomial_count() == 2 and got.parms_id() == ct.parms_id() and not got.is_ntt_form()
    assert dec(got) == want
    single = ev.rotate_bsgs_sum_new(ct, BABY, GIANT, gk, pw)
    assert dec(single) == dec(got)
    assert single.data() != got.data()
    # the spelling with a destination and keyword arguments; Galois elements (1 = the identity)
    dest = pytroy.Ciphertext()
    ev.rotate_bsgs_sum_double_hoisted(encrypted=ct, baby_steps=BABY, giant_steps=GIANT, galois_keys=gk, weights=pw, destination=dest)
    assert dest.data() == got.data()
    small = [pw[0][:2], pw[1][:2]]
    by_elements = ev.apply_galois_bsgs_sum_double_hoisted_new(ct, [1, 3], [1, 3], gk, small)
    assert by_elements.data() == ev.rotate_bsgs_sum_double_hoisted_new(ct, [0, 1], [0, 1], gk, small).data()
    dest = pytroy.Ciphertext()
    ev.apply_galois_bsgs_sum_double_hoisted(encrypted=ct, baby_elements=[1, 3], giant_elements=[1, 3], galois_keys=gk, weights=small, destination=dest)
    assert dest.data() == by_elements.data()
    # refusals, each with the method's name
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum_double_hoisted\].*Galois key not present"):
        ev.rotate_bsgs_sum_double_hoisted_new(ct, [0, 1], [0, 5], gk, small)               # no NAF chain
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum_double_hoisted\].*key level"):
        ev.rotate_bsgs_sum_double_hoisted_new(ct, [1], [4], gk, [[ev.transform_plain_to_ntt_new(encoder.encode_simd_new(diag[0]), ct.parms_id())]])
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum_double_hoisted\].*NTT form"):
        ev.rotate_bsgs_sum_double_hoisted_new(ct, [1], [4], gk, [[encoder.encode_simd_new(diag[0])]])
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum_double_hoisted\].*giant step has no weight"):
        ev.rotate_bsgs_sum_double_hoisted_new(ct, [0, 1], [0, 4], gk, [pw[0][:2], [None, None]])
    with pytest.raises(ValueError, match=r"apply_galois_bsgs_sum_double_hoisted\]"):
        ev.apply_galois_bsgs_sum_double_hoisted_new(ct, [3], [9], gk, [])                  # one weight row per giant step
    with pytest.raises(ValueError, match=r"apply_galois_bsgs_sum_double_hoisted\].*Empty element list"):
        ev.apply_galois_bsgs_sum_double_hoisted_new(ct, [], [3], gk, [[]])
    pytroy.MemoryPool.destroy_global_pool()


def test_bgv_is_refused(pytroy, dev):
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BGV, 17)
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new([1, 2, 3]))
    gk = kg.create_galois_keys_from_steps([1], False)
    pw = ev.transform_plain_to_ntt_new(encoder.encode_simd_new([1, 1, 1]), ct.parms_id())
    for name, call in (("rotate_bsgs_sum_double_hoisted", lambda: ev.rotate_bsgs_sum_double_hoisted_new(ct, [1], [1], gk, [[pw]])),
                       ("apply_galois_bsgs_sum_double_hoisted", lambda: ev.apply_galois_bsgs_sum_double_hoisted_new(ct, [3], [3], gk, [[pw]]))):
        with pytest.raises(ValueError, match=name + r"\].*BGV is not supported: its key switch divides by the special prime differently"):
            call()
    pytroy.MemoryPool.destroy_global_pool()


def test_ckks_bsgs_product(pytroy, dev):
    """N = 8192 {40,40,40,40}: the 16-diagonal product on complex slots.  rotate_bsgs_sum's error against the float product is measured in the
    same test; the double-hoisted result's error must be within 4 x that -- the roundings happen at different points (here one per giant step
    fewer) under the same kind of noise bound, the margin tests/test_gpu_bsgs_api.py uses for the same reason."""
    ctx, enc, gk, encryptor, dec, ev = _ckks(pytroy, [1, 2, 3, 4, 8, 12])
    scale = float(1 << 30)
    rnd = random.Random(8)
    slots = enc.slot_count()
    z = _disc(rnd, slots)
    diag = [_disc(rnd, slots) for _ in range(16)]
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, scale))
    back = lambda x, g: [x[(i - g) % slots] for i in range(slots)]          # rot_g(back(x) * y) = x * rot_g(y)
    flat = enc.encode_complex64_simd_new_batched([back(diag[g + b], g) for g in GIANT for b in BABY], ctx.key_parms_id(), scale)
    pw = [flat[4 * i:4 * i + 4] for i in range(4)]
    got = ev.rotate_bsgs_sum_double_hoisted_new(c, BABY, GIANT, gk, pw)
    assert got.is_ntt_form() and got.parms_id() == c.parms_id() and got.scale() == c.scale() * scale
    single = ev.rotate_bsgs_sum_new(c, BABY, GIANT, gk, pw)
    want = [sum(diag[d][i] * z[(i + d) % slots] for d in range(16)) for i in range(slots)]
    a = enc.decode_complex64_simd_new(dec.decrypt_new(got)).tolist()
    b = enc.decode_complex64_simd_new(dec.decrypt_new(single)).tolist()
    ea = max(abs(a[i] - want[i]) for i in range(slots))
    eb = max(abs(b[i] - want[i]) for i in range(slots))
    print("ckks bsgs: double-hoisted max error %.3e, single-hoisted %.3e (bound 4 x single-hoisted)" % (ea, eb))
    assert ea <= 4 * eb
    dest = pytroy.Ciphertext()
    ev.rotate_bsgs_sum_double_hoisted(c, BABY, GIANT, gk, pw, dest)
    assert dest.data() == got.data()
    with pytest.raises(ValueError, match=r"rotate_bsgs_sum_double_hoisted\].*different scales"):
        ev.rotate_bsgs_sum_double_hoisted_new(c, [0, 1], [4], gk, [[pw[0][0], enc.encode_complex64_simd_new(diag[1], ctx.key_parms_id(), float(1 << 20))]])
    pytroy.MemoryPool.destroy_global_pool()
