"""Evaluator::mod_raise (addition: the exact centred base extension of an exhausted CKKS ciphertext to the top of the chain, troy/troy.h) through
pytroy: level and metadata of the result, the round trip back down (needs no key), the decryption m + Q_l * I with its bound, the forms, and the
refusals.  CKKS N = 8192, {60, 40 x 6, 60}, scale 2^40."""
import numpy as np
import pytest

from test_gpu_hoist_api import _params, pytroy  # noqa: F401  (the module's fixture and parameter helper)

pytestmark = pytest.mark.gpu

N, BITS, SCALE = 8192, [60, 40, 40, 40, 40, 40, 40, 60], float(1 << 40)
_STATE = {}


def _setup(pytroy):
    if "ckks" not in _STATE:
        p = _params(pytroy, pytroy.SchemeType.CKKS, N, BITS)
        ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 47)
        ctx.to_device_inplace()
        enc = pytroy.CKKSEncoder(ctx)
        kg = pytroy.KeyGenerator(ctx)
        encryptor = pytroy.Encryptor(ctx)
        encryptor.set_public_key(kg.create_public_key(False))
        primes = [int(m.value()) for m in pytroy.CoeffModulus.create(N, BITS)][:-1]
        _STATE["ckks"] = (ctx, enc, kg, encryptor, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx), primes)
    return _STATE["ckks"]


def _fresh(enc, encryptor, seed):
    values = np.random.default_rng(seed).uniform(-1, 1, enc.slot_count())
    return encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in values], None, SCALE))


def _down_to(ev, c, limbs):
    while c.coeff_modulus_size() > limbs:
        c = ev.mod_switch_to_next_new(c)
    return c


def _same(a, b):
    return (a.data() == b.data() and a.parms_id() == b.parms_id() and a.scale() == b.scale() and a.is_ntt_form() == b.is_ntt_form() and
            a.polynomial_count() == b.polynomial_count() and a.coeff_modulus_size() == b.coeff_modulus_size())


@pytest.mark.parametrize("limbs", [1, 2])
def test_mod_raise_round_trip_and_decryption(pytroy, dev, limbs):
    ctx, enc, kg, encryptor, dec, ev, primes = _setup(pytroy)
    low = _down_to(ev, _fresh(enc, encryptor, 10 + limbs), limbs)
    assert low.coeff_modulus_size() == limbs
    raised = ev.mod_raise_new(low)
    assert raised.parms_id() == ctx.first_parms_id() and raised.coeff_modulus_size() == 7
    assert raised.scale() == low.scale() and raised.is_ntt_form() and raised.polynomial_count() == 2
    # back down: the input's words exactly (no key involved)
    back = ev.mod_switch_to_new(raised, low.parms_id())
    assert _same(back, low)
    # c0' + c1' s = c0 + c1 s modulo each of the input's primes, in NTT form as well: the plaintext's first rows are the original plaintext
    plain_raised, plain_low = dec.decrypt_new(raised), dec.decrypt_new(low)
    rows_raised = np.array(plain_raised.data(), dtype=np.uint64).reshape(7, N)
    rows_low = np.array(plain_low.data(), dtype=np.uint64).reshape(limbs, N)
    assert np.array_equal(rows_raised[:limbs], rows_low)
    # m + Q_l * I with |I| <= (h + 1) / 2, h <= N: a bound from the contract, not a measurement
    Q = 1
    for q in primes[:limbs]:
        Q *= q
    coeffs = np.asarray(enc.decode_float64_polynomial_new(plain_raised)) * SCALE
    top = float(np.max(np.abs(coeffs)))
    print("mod_raise l=%d: max |coefficient| = %.6e = %.3f Q_l (bound %.1f Q_l)" % (limbs, top, top / float(Q), (N + 1) / 2))
    assert top <= float(Q) * (N + 1) / 2
    assert top > float(Q) / 2                                               # the raise was real: some I != 0


def test_forms_give_identical_ciphertexts(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev, primes = _setup(pytroy)
    lows = [_down_to(ev, _fresh(enc, encryptor, 30 + i), 2) for i in range(5)]
    want = [ev.mod_raise_new(c) for c in lows]
    dest = pytroy.Ciphertext()
    ev.mod_raise(encrypted=lows[0], destination=dest)
    assert _same(dest, want[0])
    inplace = lows[1].clone()
    ev.mod_raise_inplace(encrypted=inplace)
    assert _same(inplace, want[1])
    outs = [pytroy.Ciphertext() for _ in lows]
    ev.mod_raise_batched(encrypted=lows, destination=outs)                   # five items: the one-step batched path
    assert all(_same(o, w) for o, w in zip(outs, want))
    outs2 = [pytroy.Ciphertext() for _ in lows[:2]]
    ev.mod_raise_batched(lows[:2], outs2)                                    # below the batching threshold: object by object
    assert all(_same(o, w) for o, w in zip(outs2, want))
    # an explicit target below the top of the chain
    mid = ev.mod_switch_to_next_new(_fresh(enc, encryptor, 1)).parms_id()
    to_mid = ev.mod_raise_new(lows[0], parms_id=mid)
    assert to_mid.parms_id() == mid and to_mid.coeff_modulus_size() == 6
    assert _same(to_mid, ev.mod_switch_to_new(want[0], mid))                 # the rows of a raise do not depend on the target
    outs3 = [pytroy.Ciphertext() for _ in lows]
    ev.mod_raise_batched(lows, outs3, mid)
    assert all(_same(o, ev.mod_switch_to_new(w, mid)) for o, w in zip(outs3, want))


def test_three_polynomials(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev, primes = _setup(pytroy)
    a = _fresh(enc, encryptor, 50)
    prod = ev.multiply_new(a, a)                                             # three polynomials at scale 2^80
    low = _down_to(ev, prod, 2)
    raised = ev.mod_raise_new(low)
    assert raised.polynomial_count() == 3 and raised.coeff_modulus_size() == 7 and raised.scale() == low.scale()
    assert _same(ev.mod_switch_to_new(raised, low.parms_id()), low)
    rows_raised = np.array(dec.decrypt_new(raised).data(), dtype=np.uint64).reshape(7, N)
    rows_low = np.array(dec.decrypt_new(low).data(), dtype=np.uint64).reshape(2, N)
    assert np.array_equal(rows_raised[:2], rows_low)


def test_refusals(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev, primes = _setup(pytroy)
    fresh = _fresh(enc, encryptor, 70)
    low = _down_to(ev, fresh, 2)
    with pytest.raises(ValueError, match=r"\[Evaluator::mod_raise\].*strictly above"):
        ev.mod_raise_new(fresh)                                             # already at the target
    with pytest.raises(ValueError, match=r"\[Evaluator::mod_raise\].*strictly above"):
        ev.mod_raise_new(low, low.parms_id())
    with pytest.raises(ValueError, match=r"\[Evaluator::mod_raise\].*strictly above"):
        ev.mod_raise_new(low, _down_to(ev, fresh, 1).parms_id())
    with pytest.raises(ValueError, match=r"\[Evaluator::mod_raise\].*key level"):
        ev.mod_raise_new(low, ctx.key_parms_id())
    # a BFV context; its parms id is not in the CKKS chain
    p = _params(pytroy, pytroy.SchemeType.BFV, 4096, [36, 36, 37])
    bctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 3)
    bctx.to_device_inplace()
    benc = pytroy.BatchEncoder(bctx)
    benc.to_device_inplace()
    bkg = pytroy.KeyGenerator(bctx)
    bencryptor = pytroy.Encryptor(bctx)
    bencryptor.set_public_key(bkg.create_public_key(False))
    bct = pytroy.Evaluator(bctx).mod_switch_to_next_new(bencryptor.encrypt_asymmetric_new(benc.encode_simd_new([1, 2, 3])))
    with pytest.raises(ValueError, match=r"\[Evaluator::mod_raise\].*CKKS only"):
        pytroy.Evaluator(bctx).mod_raise_new(bct)
    with pytest.raises(ValueError, match=r"\[Evaluator::mod_raise\].*not in the modulus chain"):
        ev.mod_raise_new(low, bctx.first_parms_id())
    # 17 input limbs
    wp = _params(pytroy, pytroy.SchemeType.CKKS, 4096, [30] * 19)
    wctx = pytroy.HeContext(wp, True, pytroy.SecurityLevel.Nil, 5)
    wctx.to_device_inplace()
    wenc = pytroy.CKKSEncoder(wctx)
    wkg = pytroy.KeyGenerator(wctx)
    wencryptor = pytroy.Encryptor(wctx)
    wencryptor.set_public_key(wkg.create_public_key(False))
    wev = pytroy.Evaluator(wctx)
    wide = wev.mod_switch_to_next_new(wencryptor.encrypt_asymmetric_new(wenc.encode_float64_single_new(0.5, None, float(1 << 20))))
    assert wide.coeff_modulus_size() == 17
    with pytest.raises(ValueError, match=r"\[Evaluator::mod_raise\].*More than 16 input limbs"):
        wev.mod_raise_new(wide)
    ok = wev.mod_raise_new(wev.mod_switch_to_next_new(wide))                # 16 limbs are the limit
    assert ok.coeff_modulus_size() == 18 and ok.parms_id() == wctx.first_parms_id()
