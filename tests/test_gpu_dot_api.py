"""Evaluator::multiply_accumulate / multiply_accumulate_relinearize_rescale (additions: a sum of ciphertext products, relinearized and
rescaled once) through pytroy: word-identical to folding the reference's per-pair methods, and the refusals."""
import os
import random
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "troy-nova_amd")


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


def _params(pytroy, scheme, n, bits, t_bits=20):
    p = pytroy.EncryptionParameters(scheme)
    p.set_poly_modulus_degree(n)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(n, bits))
    if scheme != pytroy.SchemeType.CKKS:
        p.set_plain_modulus(pytroy.PlainModulus.batching(n, t_bits))
    return p


def _ckks(pytroy):
    p = _params(pytroy, pytroy.SchemeType.CKKS, 8192, [40, 40, 40, 40])
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Classical128, 99)
    ctx.to_device_inplace()
    enc = pytroy.CKKSEncoder(ctx)
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    return ctx, enc, kg, encryptor, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx)


def _same(x, y):
    return x.data() == y.data() and x.scale() == y.scale() and x.parms_id() == y.parms_id() and x.polynomial_count() == y.polynomial_count()


def test_ckks_dot_product(pytroy, dev):
    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy)
    rnd = random.Random(5)
    scale = float(1 << 30)
    slots = enc.slot_count()
    zs1 = [[complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(slots)] for _ in range(4)]
    zs2 = [[complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(slots)] for _ in range(4)]
    c1 = [encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, scale)) for z in zs1]
    c2 = [encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, scale)) for z in zs2]
    rk = kg.create_relin_keys(False)
    # the reference's methods, pair by pair
    folded = ev.multiply_new(c1[0], c2[0])
    for x, y in zip(c1[1:], c2[1:]):
        ev.add_inplace(folded, ev.multiply_new(x, y))
    acc = ev.multiply_accumulate_new(c1, c2)
    assert acc.polynomial_count() == 3 and _same(acc, folded)
    dest = pytroy.Ciphertext()
    ev.multiply_accumulate(encrypted1=c1, encrypted2=c2, destination=dest)
    assert _same(dest, folded)
    low = ev.relinearize_new(folded, rk)
    ev.rescale_to_next_inplace(low)
    chain = ev.multiply_accumulate_relinearize_rescale_new(c1, c2, rk)
    assert chain.polynomial_count() == 2 and _same(chain, low)
    dest = pytroy.Ciphertext()
    ev.multiply_accumulate_relinearize_rescale(encrypted1=c1, encrypted2=c2, relin_keys=rk, destination=dest)
    assert _same(dest, low)
    # one term is the fused single-pair method
    assert _same(ev.multiply_accumulate_relinearize_rescale_new(c1[:1], c2[:1], rk), ev.multiply_relinearize_rescale_new(c1[0], c2[0], rk))
    # meaning: SUM z1 z2 per slot; tests/test_pytroy.py allows one product 1e-2 at this scale, four independent terms of the same noise get 4 x that
    got = enc.decode_complex64_simd_new(dec.decrypt_new(chain)).tolist()
    want = [sum(zs1[t][i] * zs2[t][i] for t in range(4)) for i in range(slots)]
    assert max(abs(g - w) for g, w in zip(got, want)) < 4 * 1e-2
    pytroy.MemoryPool.destroy_global_pool()


def test_bgv_dot_product(pytroy, dev):
    p = _params(pytroy, pytroy.SchemeType.BGV, 8192, [40, 40, 40])
    assert p.plain_modulus().value() == 1032193
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Classical128, 17)
    ctx.to_device_inplace()
    encoder = pytroy.BatchEncoder(ctx)
    encoder.to_device_inplace()
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    dec = pytroy.Decryptor(ctx, kg.secret_key())
    ev = pytroy.Evaluator(ctx)
    rnd = random.Random(11)
    v1 = [[rnd.randrange(1000) for _ in range(64)] for _ in range(3)]
    v2 = [[rnd.randrange(1000) for _ in range(64)] for _ in range(3)]
    c1 = [encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v)) for v in v1]
    c2 = [encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v)) for v in v2]
    folded = ev.multiply_new(c1[0], c2[0])
    for x, y in zip(c1[1:], c2[1:]):
        ev.add_inplace(folded, ev.multiply_new(x, y))
    acc = ev.multiply_accumulate_new(c1, c2)
    assert acc.polynomial_count() == 3 and acc.data() == folded.data() and acc.parms_id() == folded.parms_id()
    assert acc.correction_factor() == folded.correction_factor()
    got = encoder.decode_simd_new(dec.decrypt_new(ev.relinearize_new(acc, kg.create_relin_keys(False))))[:64]
    assert list(got) == [sum(v1[t][i] * v2[t][i] for t in range(3)) % 1032193 for i in range(64)]
    # products with different correction factors are refused (folding them would rescale an operand)
    odd = c1[1].clone()
    odd.set_correction_factor(3)
    with pytest.raises(ValueError):
        ev.multiply_accumulate_new([c1[0], odd], [c2[0], c2[1]])
    pytroy.MemoryPool.destroy_global_pool()


def test_refusals(pytroy, dev):
    # BFV: the BEHZ multiply rounds per product
    p = _params(pytroy, pytroy.SchemeType.BFV, 4096, [36, 36, 37])
    bctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 7)
    bctx.to_device_inplace()
    benc = pytroy.BatchEncoder(bctx)
    benc.to_device_inplace()
    bkg = pytroy.KeyGenerator(bctx)
    bencryptor = pytroy.Encryptor(bctx)
    bencryptor.set_public_key(bkg.create_public_key(False))
    bev = pytroy.Evaluator(bctx)
    bc = bencryptor.encrypt_asymmetric_new(benc.encode_simd_new([1, 2, 3]))
    with pytest.raises(ValueError):
        bev.multiply_accumulate_new([bc, bc], [bc, bc])
    with pytest.raises(ValueError):
        bev.multiply_accumulate_relinearize_rescale_new([bc, bc], [bc, bc], bkg.create_relin_keys(False))

    ctx, enc, kg, encryptor, dec, ev = _ckks(pytroy)
    rk = kg.create_relin_keys(False)
    scale = float(1 << 30)
    z = [complex(0.5, -0.25)] * enc.slot_count()
    c = [encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, scale)) for _ in range(3)]
    for call in (lambda a, b: ev.multiply_accumulate_new(a, b), lambda a, b: ev.multiply_accumulate_relinearize_rescale_new(a, b, rk)):
        assert call(c[:2], c[1:]).polynomial_count() in (2, 3)               # the well-formed call goes through
        with pytest.raises(ValueError):                                      # lists of unequal length
            call(c[:2], c[:3])
        with pytest.raises(ValueError):                                      # empty lists
            call([], [])
        lower = ev.mod_switch_to_next_new(c[2])                              # a pair at a different level
        with pytest.raises(ValueError):
            call([c[0], lower], [c[1], lower])
        small = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, float(1 << 20)))
        with pytest.raises(ValueError):                                      # a pair encoded at scale 2^20 beside pairs at 2^30
            call([c[0], small], [c[1], small])
        host = c[2].clone()
        host.to_host_inplace()
        with pytest.raises(ValueError):                                      # multiply's own checks reach every pair, not only the first
            call([c[0], host], [c[1], c[2]])
    pytroy.MemoryPool.destroy_global_pool()
