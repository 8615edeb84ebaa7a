"""Evaluator::bfv_multiply_accumulate / bfv_multiply_accumulate_relinearize (additions: a sum of BEHZ tensor products scaled down once, and
relinearized once) through pytroy: the meaning of the result, its relation to the per-pair methods, and the refusals."""
import os
import random
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "troy-nova_amd")
CAP = 1024


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


def _context(pytroy, scheme, n, bits):
    p = pytroy.EncryptionParameters(scheme)
    p.set_poly_modulus_degree(n)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(n, bits))
    if scheme != pytroy.SchemeType.CKKS:
        p.set_plain_modulus(pytroy.PlainModulus.batching(n, 20))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 7)
    ctx.to_device_inplace()
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    return p, ctx, kg, encryptor


def _bfv(pytroy, bits=(36, 36, 37)):
    p, ctx, kg, encryptor = _context(pytroy, pytroy.SchemeType.BFV, 4096, list(bits))
    encoder = pytroy.BatchEncoder(ctx)
    encoder.to_device_inplace()
    return p, ctx, kg, encryptor, encoder, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx)


def _same(x, y):
    return x.data() == y.data() and x.parms_id() == y.parms_id() and x.polynomial_count() == y.polynomial_count() and x.is_ntt_form() == y.is_ntt_form()


def test_bfv_dot_product(pytroy, dev):
    p, ctx, kg, encryptor, encoder, dec, ev = _bfv(pytroy)
    t = p.plain_modulus().value()
    rnd = random.Random(3)
    v1 = [[rnd.randrange(t) for _ in range(64)] for _ in range(4)]
    v2 = [[rnd.randrange(t) for _ in range(64)] for _ in range(4)]
    c1 = [encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v)) for v in v1]
    c2 = [encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v)) for v in v2]
    rk = kg.create_relin_keys(False)
    acc = ev.bfv_multiply_accumulate_new(c1, c2)
    assert acc.polynomial_count() == 3 and not acc.is_ntt_form()
    low = ev.relinearize_new(acc, rk)
    got = encoder.decode_simd_new(dec.decrypt_new(low))[:64]
    assert list(got) == [sum(v1[k][i] * v2[k][i] for k in range(4)) % t for i in range(64)]
    fused = ev.bfv_multiply_accumulate_relinearize_new(c1, c2, rk)
    assert fused.polynomial_count() == 2 and _same(fused, low)
    # one term is the reference's multiply
    assert _same(ev.bfv_multiply_accumulate_new(c1[:1], c2[:1]), ev.multiply_new(c1[0], c2[0]))
    # the destination forms
    dest = pytroy.Ciphertext()
    ev.bfv_multiply_accumulate(encrypted1=c1, encrypted2=c2, destination=dest)
    assert _same(dest, acc)
    dest = pytroy.Ciphertext()
    ev.bfv_multiply_accumulate_relinearize(encrypted1=c1, encrypted2=c2, relin_keys=rk, destination=dest)
    assert _same(dest, low)
    pytroy.MemoryPool.destroy_global_pool()


def test_refusals(pytroy, dev):
    # a CKKS context
    cp, cctx, ckg, cencryptor = _context(pytroy, pytroy.SchemeType.CKKS, 8192, [40, 40, 40, 40])
    cenc = pytroy.CKKSEncoder(cctx)
    cev = pytroy.Evaluator(cctx)
    cc = cencryptor.encrypt_asymmetric_new(cenc.encode_complex64_simd_new([complex(0.5, 0.25)] * cenc.slot_count(), None, float(1 << 30)))
    with pytest.raises(ValueError):
        cev.bfv_multiply_accumulate_new([cc], [cc])
    with pytest.raises(ValueError):
        cev.bfv_multiply_accumulate_relinearize_new([cc], [cc], ckg.create_relin_keys(False))

    p, ctx, kg, encryptor, encoder, dec, ev = _bfv(pytroy, (36, 36, 36, 37))
    rk = kg.create_relin_keys(False)
    c = [encryptor.encrypt_asymmetric_new(encoder.encode_simd_new([k + 1, 2, 3])) for k in range(3)]
    # multiply_accumulate keeps refusing BFV
    with pytest.raises(ValueError):
        ev.multiply_accumulate_new(c[:2], c[1:])
    for call in (lambda a, b: ev.bfv_multiply_accumulate_new(a, b), lambda a, b: ev.bfv_multiply_accumulate_relinearize_new(a, b, rk)):
        assert call(c[:2], c[1:]).polynomial_count() in (2, 3)               # the well-formed call goes through
        with pytest.raises(ValueError):                                      # an NTT-form operand
            call([c[0], ev.transform_to_ntt_new(c[1])], [c[1], c[2]])
        with pytest.raises(ValueError):                                      # a three-polynomial operand
            call([c[0], c[1]], [c[1], ev.multiply_new(c[0], c[1])])
        host = c[2].clone()
        host.to_host_inplace()
        for a, b in (([host, c[0]], [c[1], c[2]]), ([c[0], host], [c[1], c[2]]), ([c[0], c[1]], [host, c[2]]), ([c[0], c[1]], [c[2], host])):
            with pytest.raises(ValueError):                                  # a host operand in any position
                call(a, b)
        with pytest.raises(ValueError):                                      # lists of unequal length
            call(c[:2], c[:3])
        with pytest.raises(ValueError):                                      # empty lists
            call([], [])
        lower = ev.mod_switch_to_next_new(c[2])                              # a pair at a different level
        with pytest.raises(ValueError):
            call([c[0], lower], [c[1], lower])
        with pytest.raises(ValueError):                                      # one term more than the cap
            call([c[0]] * (CAP + 1), [c[1]] * (CAP + 1))
    pytroy.MemoryPool.destroy_global_pool()
