"""Evaluator::multiply_relinearize_mod_switch (an addition: BGV multiply -> relinearize -> mod_switch_to_next as one library call) through
pytroy with genuine keys at N = 4096, t = 65537: identical to the three reference methods, decrypts to the slot-wise product, the batched form,
and the refusals."""
import os
import random
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "troy-nova_amd")
N, T = 4096, 65537
NAME = "multiply_relinearize_mod_switch"


@pytest.fixture(scope="module")
def pytroy():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch  # noqa: F401  (first: one HIP runtime per process -- torch bundles its own libamdhip64)
    try:
        import pytroy as m
    except ImportError as e:
        pytest.fail("pytroy_raw is not built (python -c 'import __graft_entry__ as g; g.build()'): %s" % e)
    return m


def _context(pytroy, scheme, bits, seed):
    p = pytroy.EncryptionParameters(scheme)
    p.set_poly_modulus_degree(N)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(N, bits))
    if scheme != pytroy.SchemeType.CKKS:
        p.set_plain_modulus(T)
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, seed)
    ctx.to_device_inplace()
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    return ctx, kg, encryptor, pytroy.Evaluator(ctx)


def _same(x, y):
    return (x.data() == y.data() and x.parms_id() == y.parms_id() and x.correction_factor() == y.correction_factor() and
            x.is_ntt_form() == y.is_ntt_form() and x.polynomial_count() == y.polynomial_count() == 2)


@pytest.fixture(scope="module")
def bgv(pytroy, dev):
    ctx, kg, encryptor, ev = _context(pytroy, pytroy.SchemeType.BGV, [36, 36, 36, 36, 37], 23)
    encoder = pytroy.BatchEncoder(ctx)
    encoder.to_device_inplace()
    rnd = random.Random(3)
    vs = [[rnd.randrange(T) for _ in range(N)] for _ in range(4)]
    cts = [encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v)) for v in vs]
    return dict(ctx=ctx, kg=kg, ev=ev, encoder=encoder, dec=pytroy.Decryptor(ctx, kg.secret_key()), rk=kg.create_relin_keys(False), vs=vs, cts=cts)


def _three_methods(ev, rk, x, y):
    return ev.mod_switch_to_next_new(ev.relinearize_new(ev.multiply_new(x, y), rk))


def test_equals_the_three_methods_and_decrypts(pytroy, bgv):
    ev, rk, cts, vs = bgv["ev"], bgv["rk"], bgv["cts"], bgv["vs"]
    want = _three_methods(ev, rk, cts[0], cts[1])
    got = ev.multiply_relinearize_mod_switch_new(cts[0], cts[1], rk)
    assert got.parms_id() != cts[0].parms_id() and got.coeff_modulus_size() == cts[0].coeff_modulus_size() - 1
    assert _same(got, want)
    dest = pytroy.Ciphertext()
    ev.multiply_relinearize_mod_switch(encrypted1=cts[0], encrypted2=cts[1], relin_keys=rk, destination=dest)
    assert _same(dest, want)
    assert list(bgv["encoder"].decode_simd_new(bgv["dec"].decrypt_new(got))) == [a * b % T for a, b in zip(vs[0], vs[1])]
    # one level further down: operands below the first level, a correction factor that is already not 1
    low = [ev.mod_switch_to_next_new(c) for c in cts[:2]]
    assert low[0].correction_factor() != 1
    got = ev.multiply_relinearize_mod_switch_new(low[0], low[1], rk)
    assert _same(got, _three_methods(ev, rk, low[0], low[1]))
    assert list(bgv["encoder"].decode_simd_new(bgv["dec"].decrypt_new(got))) == [a * b % T for a, b in zip(vs[0], vs[1])]


def test_batched_equals_single_calls(pytroy, bgv):
    ev, rk, cts = bgv["ev"], bgv["rk"], bgv["cts"]
    xs, ys = [cts[0], cts[1], cts[2]], [cts[1], cts[2], cts[3]]
    outs = [pytroy.Ciphertext() for _ in range(3)]
    ev.multiply_relinearize_mod_switch_batched(xs, ys, rk, outs)
    for x, y, o in zip(xs, ys, outs):
        assert _same(o, ev.multiply_relinearize_mod_switch_new(x, y, rk))
        assert _same(o, _three_methods(ev, rk, x, y))


def test_refusals_name_the_method(pytroy, bgv, dev):
    ev, rk, cts = bgv["ev"], bgv["rk"], bgv["cts"]
    # the last level has no next level: mod_switch_to_next's message
    last = cts[0]
    while last.parms_id() != bgv["ctx"].last_parms_id():
        last = ev.mod_switch_to_next_new(last)
    with pytest.raises(ValueError, match=r"multiply_relinearize_mod_switch\].*End of modulus switching chain reached"):
        ev.multiply_relinearize_mod_switch_new(last, last, rk)
    # a three-polynomial operand, operands at different levels (multiply's own refusal behind the prefix)
    with pytest.raises(ValueError, match=NAME):
        ev.multiply_relinearize_mod_switch_new(ev.multiply_new(cts[0], cts[1]), cts[1], rk)
    with pytest.raises(ValueError, match=NAME + r"\].*\[Evaluator::multiply\]"):
        ev.multiply_relinearize_mod_switch_new(ev.mod_switch_to_next_new(cts[0]), cts[1], rk)
    # CKKS and BFV contexts
    for scheme, bits in ((pytroy.SchemeType.CKKS, [36, 36, 37]), (pytroy.SchemeType.BFV, [36, 36, 37])):
        ctx, kg, encryptor, ev2 = _context(pytroy, scheme, bits, 5)
        if scheme == pytroy.SchemeType.CKKS:
            enc = pytroy.CKKSEncoder(ctx)
            c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(0.5, 0.25)] * enc.slot_count(), None, float(1 << 20)))
        else:
            enc = pytroy.BatchEncoder(ctx)
            enc.to_device_inplace()
            c = encryptor.encrypt_asymmetric_new(enc.encode_simd_new([1, 2, 3]))
        rk2 = kg.create_relin_keys(False)
        with pytest.raises(ValueError, match=NAME):
            ev2.multiply_relinearize_mod_switch_new(c, c, rk2)
        with pytest.raises(ValueError, match=NAME):
            ev2.multiply_relinearize_mod_switch_batched([c, c, c], [c, c, c], rk2, [pytroy.Ciphertext() for _ in range(3)])
    pytroy.MemoryPool.destroy_global_pool()
