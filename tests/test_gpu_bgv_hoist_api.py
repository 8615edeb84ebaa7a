"""Evaluator::bgv_rotate_many / _sum / _weighted_sum(s) / _sum_each / _bsgs_sum and their apply_galois spellings (additions: the hoisted family on
BGV contexts, one digit decomposition and one mod-t tail for many Galois keys) through pytroy, with genuine Galois keys.  BGV is exact: the
composed path (rotate_rows_new, multiply_plain_new, add_new) is first checked against the expected vector, then every new method must decrypt
to exactly that vector.  No tolerance anywhere."""
import random

import pytest

from test_gpu_hoist_api import _batching, pytroy  # noqa: F401  (the module's fixture and parameter helpers)
from test_gpu_weighted_hoist_api import _ckks

pytestmark = pytest.mark.gpu

N = 4096
BABY, GIANT = [0, 1, 2, 3], [0, 4, 8, 12]
KEY_STEPS = [1, 2, 3, 4, 8, 12]


def _rows(x, k):
    row = N // 2
    return [x[(i + k) % row] for i in range(row)] + [x[row + (i + k) % row] for i in range(row)]


def _setup(pytroy, seed):
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BGV, seed)
    gk = kg.create_galois_keys_from_steps(KEY_STEPS, False)
    dec = lambda c: encoder.decode_simd_new(decryptor.decrypt_new(c)).tolist()
    enc = lambda x: encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(x))
    key_id = ev.context().key_parms_id()
    weight = lambda x: ev.transform_plain_to_ntt_new(encoder.encode_simd_new(x), key_id)     # the key-level preparation of the BFV methods
    return t, encoder, enc, dec, gk, ev, weight


def _add_all(ev, cts):
    acc = cts[0]
    for c in cts[1:]:
        acc = ev.add_new(acc, c)
    return acc


def test_bgv_rotations_and_sums(pytroy, dev):
    t, encoder, enc, dec, gk, ev, weight = _setup(pytroy, 23)
    rnd = random.Random(31)
    v = [rnd.randrange(t) for _ in range(N)]
    ct = enc(v)
    assert ct.is_ntt_form() and ct.correction_factor() == 1
    steps = [1, 2, 3]
    # the composed path first: one key switch per rotation
    single = [ev.rotate_rows_new(ct, k, gk) for k in steps]
    assert [dec(c) for c in single] == [_rows(v, k) for k in steps]
    want_sum = [sum(_rows(v, k)[i] for k in steps) % t for i in range(N)]
    assert dec(_add_all(ev, single)) == want_sum
    # many / sum
    many = ev.bgv_rotate_many_new(ct, steps, gk)
    assert len(many) == 3 and [dec(c) for c in many] == [_rows(v, k) for k in steps]
    assert all(c.polynomial_count() == 2 and c.parms_id() == ct.parms_id() and c.is_ntt_form() and c.correction_factor() == 1 for c in many)
    summed = ev.bgv_rotate_sum_new(ct, steps, gk)
    assert summed.is_ntt_form() and summed.parms_id() == ct.parms_id() and dec(summed) == want_sum
    # the spellings: destination and keywords, Galois elements (rotate_rows by one step is the generator 3)
    dest = pytroy.Ciphertext()
    ev.bgv_rotate_sum(encrypted=ct, steps=steps, galois_keys=gk, destination=dest)
    assert dest.data() == summed.data()
    dests = [pytroy.Ciphertext() for _ in steps]
    ev.bgv_rotate_many(encrypted=ct, steps=steps, galois_keys=gk, destination=dests)
    assert [d.data() for d in dests] == [c.data() for c in many]
    assert ev.bgv_apply_galois_sum_new(encrypted=ct, galois_elements=[3, 9, 27], galois_keys=gk).data() == summed.data()
    assert [c.data() for c in ev.bgv_apply_galois_many_new(ct, [3, 9, 27], gk)] == [c.data() for c in many]
    dest = pytroy.Ciphertext()
    ev.bgv_apply_galois_sum(encrypted=ct, galois_elements=[3, 9, 27], galois_keys=gk, destination=dest)
    assert dest.data() == summed.data()
    dests = [pytroy.Ciphertext() for _ in steps]
    ev.bgv_apply_galois_many(encrypted=ct, galois_elements=[3, 9, 27], galois_keys=gk, destination=dests)
    assert [d.data() for d in dests] == [c.data() for c in many]
    # a step of 0 contributes the ciphertext itself, duplicates count twice
    assert dec(ev.bgv_rotate_sum_new(ct, [0, 1, 1], gk)) == [(v[i] + 2 * _rows(v, 1)[i]) % t for i in range(N)]
    z = ev.bgv_rotate_many_new(ct, [0, 2, 2], gk)
    assert z[0].data() == ct.data() and dec(z[1]) == _rows(v, 2) and z[2].data() == z[1].data()
    # the correction factor is carried: the same payload under a factor of 3 decrypts to v / 3 per slot on both paths
    c3 = ct.clone()
    c3.set_correction_factor(3)
    composed3 = _add_all(ev, [ev.rotate_rows_new(c3, k, gk) for k in steps])
    inv3 = pow(3, -1, t)
    assert composed3.correction_factor() == 3 and dec(composed3) == [x * inv3 % t for x in want_sum]
    s3 = ev.bgv_rotate_sum_new(c3, steps, gk)
    assert s3.correction_factor() == 3 and s3.data() == summed.data() and dec(s3) == dec(composed3)
    assert all(c.correction_factor() == 3 for c in ev.bgv_rotate_many_new(c3, [0, 1], gk))
    # the sum of rotations of four DIFFERENT ciphertexts
    vs = [[rnd.randrange(t) for _ in range(N)] for _ in range(4)]
    cts = [enc(x) for x in vs]
    want_each = [sum(_rows(x, g)[i] for x, g in zip(vs, GIANT)) % t for i in range(N)]
    assert dec(_add_all(ev, [cts[0]] + [ev.rotate_rows_new(c, g, gk) for c, g in zip(cts[1:], GIANT[1:])])) == want_each
    each = ev.bgv_rotate_sum_each_new(cts, GIANT, gk)
    assert each.parms_id() == ct.parms_id() and each.is_ntt_form() and each.correction_factor() == 1 and dec(each) == want_each
    dest = pytroy.Ciphertext()
    ev.bgv_rotate_sum_each(encrypted=cts, steps=GIANT, galois_keys=gk, destination=dest)
    assert dest.data() == each.data()
    assert ev.bgv_apply_galois_sum_each_new(cts[:2], [1, 3], gk).data() == ev.bgv_rotate_sum_each_new(cts[:2], [0, 1], gk).data()
    dest = pytroy.Ciphertext()
    ev.bgv_apply_galois_sum_each(encrypted=cts[:2], galois_elements=[1, 3], galois_keys=gk, destination=dest)
    assert dest.data() == ev.bgv_rotate_sum_each_new(cts[:2], [0, 1], gk).data()
    for c in cts:
        c.set_correction_factor(5)
    each5 = ev.bgv_rotate_sum_each_new(cts, GIANT, gk)
    assert each5.correction_factor() == 5 and each5.data() == each.data()
    pytroy.MemoryPool.destroy_global_pool()


def test_bgv_weighted_sums_and_bsgs_product(pytroy, dev):
    """a random 16-diagonal matrix times an encrypted vector, as tests/test_gpu_bsgs_api.py::test_bfv_bsgs_product: diagonal d multiplies the
    rotation by d = giant + baby; the weight of (giant, baby) is that diagonal rotated back by the giant step"""
    t, encoder, enc, dec, gk, ev, weight = _setup(pytroy, 29)
    rnd = random.Random(37)
    v = [rnd.randrange(t) for _ in range(N)]
    ct = enc(v)
    diag = [[rnd.randrange(t) for _ in range(N)] for _ in range(16)]
    back = [[_rows(diag[g + b], -g) for b in BABY] for g in GIANT]
    pw = [[weight(x) for x in row] for row in back]
    rotated = [_rows(v, d) for d in range(16)]
    want = [sum(diag[d][i] * rotated[d][i] for d in range(16)) % t for i in range(N)]
    # the composed path: per baby step one rotate_rows, per weight one multiply_plain, per giant step one more rotate_rows, and the adds
    level_plain = lambda x: ev.transform_plain_to_ntt_new(encoder.encode_simd_new(x), ct.parms_id())
    babies = [ct] + [ev.rotate_rows_new(ct, b, gk) for b in BABY[1:]]
    inner = [_add_all(ev, [ev.multiply_plain_new(babies[b], level_plain(back[g][b])) for b in range(4)]) for g in range(4)]
    want_inner = [[sum(back[g][b][i] * rotated[b][i] for b in range(4)) % t for i in range(N)] for g in range(4)]
    assert [dec(c) for c in inner] == want_inner
    composed = _add_all(ev, [inner[0]] + [ev.rotate_rows_new(inner[g], GIANT[g], gk) for g in range(1, 4)])
    assert dec(composed) == want
    # the weighted sums: every slot from one decomposition; None = the term is absent from the slot
    sums = ev.bgv_rotate_weighted_sums_new(ct, BABY, gk, pw)
    assert len(sums) == 4 and [dec(c) for c in sums] == want_inner
    assert all(c.polynomial_count() == 2 and c.parms_id() == ct.parms_id() and c.is_ntt_form() and c.correction_factor() == 1 for c in sums)
    sparse = ev.bgv_rotate_weighted_sum_new(ct, BABY, gk, [pw[1][0], None, pw[1][2], None])
    assert dec(sparse) == [(back[1][0][i] * rotated[0][i] + back[1][2][i] * rotated[2][i]) % t for i in range(N)]
    # spellings
    dests = [pytroy.Ciphertext() for _ in GIANT]
    ev.bgv_rotate_weighted_sums(encrypted=ct, steps=BABY, galois_keys=gk, weights=pw, destination=dests)
    assert [d.data() for d in dests] == [c.data() for c in sums]
    dest = pytroy.Ciphertext()
    ev.bgv_rotate_weighted_sum(encrypted=ct, steps=BABY, galois_keys=gk, weights=pw[2], destination=dest)
    assert dest.data() == sums[2].data()
    assert ev.bgv_apply_galois_weighted_sum_new(ct, [1, 3, 9, 27], gk, pw[3]).data() == sums[3].data()
    dest = pytroy.Ciphertext()
    ev.bgv_apply_galois_weighted_sum(encrypted=ct, galois_elements=[1, 3, 9, 27], galois_keys=gk, weights=pw[3], destination=dest)
    assert dest.data() == sums[3].data()
    assert [c.data() for c in ev.bgv_apply_galois_weighted_sums_new(ct, [1, 3, 9, 27], gk, pw)] == [c.data() for c in sums]
    dests = [pytroy.Ciphertext() for _ in GIANT]
    ev.bgv_apply_galois_weighted_sums(encrypted=ct, galois_elements=[1, 3, 9, 27], galois_keys=gk, weights=pw, destination=dests)
    assert [d.data() for d in dests] == [c.data() for c in sums]
    # the transform: one decomposition of ct, giants + 1 divisions; its words are weighted_sums followed by sum_each
    got = ev.bgv_rotate_bsgs_sum_new(ct, BABY, GIANT, gk, pw)
    assert got.polynomial_count() == 2 and got.parms_id() == ct.parms_id() and got.is_ntt_form() and got.correction_factor() == 1
    assert dec(got) == want
    assert got.data() == ev.bgv_rotate_sum_each_new(sums, GIANT, gk).data()
    dest = pytroy.Ciphertext()
    ev.bgv_rotate_bsgs_sum(encrypted=ct, baby_steps=BABY, giant_steps=GIANT, galois_keys=gk, weights=pw, destination=dest)
    assert dest.data() == got.data()
    g_el = [1, pow(3, 4, 2 * N), pow(3, 8, 2 * N), pow(3, 12, 2 * N)]
    assert ev.bgv_apply_galois_bsgs_sum_new(ct, [1, 3, 9, 27], g_el, gk, pw).data() == got.data()
    dest = pytroy.Ciphertext()
    ev.bgv_apply_galois_bsgs_sum(encrypted=ct, baby_elements=[1, 3, 9, 27], giant_elements=g_el, galois_keys=gk, weights=pw, destination=dest)
    assert dest.data() == got.data()
    # the correction factor is carried through the weights
    c7 = ct.clone()
    c7.set_correction_factor(7)
    g7 = ev.bgv_rotate_bsgs_sum_new(c7, BABY, GIANT, gk, pw)
    assert g7.correction_factor() == 7 and g7.data() == got.data() and dec(g7) == [x * pow(7, -1, t) % t for x in want]
    assert all(c.correction_factor() == 7 for c in ev.bgv_rotate_weighted_sums_new(c7, BABY, gk, pw))
    pytroy.MemoryPool.destroy_global_pool()


def test_bgv_refusals(pytroy, dev):
    t, encoder, enc, dec, gk, ev, weight = _setup(pytroy, 41)
    ct, other = enc([1, 2, 3]), enc([4, 5, 6])
    w = weight([1] * N)
    with pytest.raises(ValueError, match="Galois key not present"):                       # (apply_galois's own check and wording, as for rotate_sum)
        ev.bgv_rotate_sum_new(ct, [1, 5], gk)                                             # no NAF chain
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.bgv_rotate_many_new(ct, [5], gk)
    with pytest.raises(ValueError, match=r"bgv_rotate_weighted_sum\].*Galois key not present"):
        ev.bgv_rotate_weighted_sum_new(ct, [5], gk, [w])
    with pytest.raises(ValueError, match=r"bgv_rotate_sum_each\].*Galois key not present"):
        ev.bgv_rotate_sum_each_new([ct, other], [1, 5], gk)
    with pytest.raises(ValueError, match=r"bgv_rotate_bsgs_sum\].*Galois key not present"):
        ev.bgv_rotate_bsgs_sum_new(ct, [0, 1], [0, 5], gk, [[w, w], [w, w]])
    with pytest.raises(ValueError, match=r"bgv_rotate_sum\].*Empty element list"):
        ev.bgv_rotate_sum_new(ct, [], gk)
    with pytest.raises(ValueError, match=r"bgv_apply_galois_many\].*Empty element list"):
        ev.bgv_apply_galois_many_new(ct, [], gk)
    with pytest.raises(ValueError):
        ev.bgv_apply_galois_sum_new(ct, [1], gk)          # the identity is a step of 0, not a Galois element with a key
    with pytest.raises(ValueError, match=r"bgv_rotate_sum_each\].*different correction factors"):
        c2 = other.clone()
        c2.set_correction_factor(2)
        ev.bgv_rotate_sum_each_new([ct, c2], [1, 2], gk)
    with pytest.raises(ValueError, match=r"bgv_apply_galois_sum_each\]"):
        ev.bgv_apply_galois_sum_each_new([ct, other], [3], gk)                            # one ciphertext per element
    with pytest.raises(ValueError, match=r"bgv_rotate_sum\].*NTT form"):
        ev.bgv_rotate_sum_new(ev.transform_from_ntt_new(ct), [1], gk)
    with pytest.raises(ValueError, match=r"bgv_rotate_bsgs_sum\].*key level"):
        ev.bgv_rotate_bsgs_sum_new(ct, [1], [4], gk, [[ev.transform_plain_to_ntt_new(encoder.encode_simd_new([1]), ct.parms_id())]])
    with pytest.raises(ValueError, match=r"bgv_rotate_bsgs_sum\].*giant step has no weight"):
        ev.bgv_rotate_bsgs_sum_new(ct, [0, 1], [0, 4], gk, [[w, w], [None, None]])
    with pytest.raises(ValueError, match=r"bgv_rotate_weighted_sums\]"):
        ev.bgv_rotate_weighted_sums_new(ct, [0, 1], gk, [[w]])                            # one weight (or None) per term
    pytroy.MemoryPool.destroy_global_pool()


def _bgv_calls(ev, ct, gk, w):
    return (("rotate_many", lambda: ev.bgv_rotate_many_new(ct, [1], gk)), ("rotate_sum", lambda: ev.bgv_rotate_sum_new(ct, [1], gk)),
            ("apply_galois_many", lambda: ev.bgv_apply_galois_many_new(ct, [3], gk)), ("apply_galois_sum", lambda: ev.bgv_apply_galois_sum_new(ct, [3], gk)),
            ("rotate_weighted_sums", lambda: ev.bgv_rotate_weighted_sums_new(ct, [1], gk, [[w]])),
            ("rotate_weighted_sum", lambda: ev.bgv_rotate_weighted_sum_new(ct, [1], gk, [w])),
            ("apply_galois_weighted_sums", lambda: ev.bgv_apply_galois_weighted_sums_new(ct, [3], gk, [[w]])),
            ("apply_galois_weighted_sum", lambda: ev.bgv_apply_galois_weighted_sum_new(ct, [3], gk, [w])),
            ("rotate_sum_each", lambda: ev.bgv_rotate_sum_each_new([ct], [1], gk)), ("apply_galois_sum_each", lambda: ev.bgv_apply_galois_sum_each_new([ct], [3], gk)),
            ("rotate_bsgs_sum", lambda: ev.bgv_rotate_bsgs_sum_new(ct, [1], [1], gk, [[w]])),
            ("apply_galois_bsgs_sum", lambda: ev.bgv_apply_galois_bsgs_sum_new(ct, [3], [3], gk, [[w]])))


def test_other_schemes_are_refused(pytroy, dev):
    """a BFV or CKKS context is sent to the unprefixed method by name"""
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BFV, 43)
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new([1, 2, 3]))
    gk = kg.create_galois_keys_from_steps([1], False)
    w = ev.transform_plain_to_ntt_new(encoder.encode_simd_new([1, 1, 1]), ev.context().key_parms_id())
    for name, call in _bgv_calls(ev, ct, gk, w):
        with pytest.raises(ValueError, match=r"bgv_" + name + r"\].*BGV contexts only.*Evaluator::" + name + r"\."):
            call()
    assert encoder.decode_simd_new(decryptor.decrypt_new(ev.rotate_sum_new(ct, [1], gk))).tolist()[:2] == [2, 3]     # the method it names
    pytroy.MemoryPool.destroy_global_pool()
    ctx, enc, gk, encryptor, dec, ev = _ckks(pytroy, [1])
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([1.0, 2.0], None, float(1 << 30)))
    w = enc.encode_complex64_simd_new([1.0, 1.0], ctx.key_parms_id(), float(1 << 20))
    for name, call in _bgv_calls(ev, c, gk, w):
        with pytest.raises(ValueError, match=r"bgv_" + name + r"\].*BGV contexts only.*Evaluator::" + name + r"\."):
            call()
    pytroy.MemoryPool.destroy_global_pool()
