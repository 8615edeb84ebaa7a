"""Evaluator::rotate_many / rotate_sum / apply_galois_many / apply_galois_sum (additions: one digit decomposition for many Galois keys)
through pytroy, with genuine Galois keys: the results decrypt to what the reference's per-rotation methods decrypt to, and the refusals."""
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


def _batching(pytroy, scheme, seed):
    p = _params(pytroy, scheme, 4096, [36, 36, 37])
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, seed)
    ctx.to_device_inplace()
    encoder = pytroy.BatchEncoder(ctx)
    encoder.to_device_inplace()
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    return p.plain_modulus().value(), encoder, kg, encryptor, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx)


def test_bfv_rotate_many_and_sum(pytroy, dev):
    n = 4096
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BFV, 7)
    row = n // 2
    rnd = random.Random(13)
    v = [rnd.randrange(t) for _ in range(n)]
    rot = lambda k: [v[(i + k) % row] for i in range(row)] + [v[row + (i + k) % row] for i in range(row)]
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new(v))
    gk = kg.create_galois_keys_from_steps([1, 2, 5], False)
    dec = lambda c: encoder.decode_simd_new(decryptor.decrypt_new(c)).tolist()
    steps = [1, 2, 5]
    single = [dec(ev.rotate_rows_new(ct, k, gk)) for k in steps]
    assert single == [rot(k) for k in steps]
    many = ev.rotate_many_new(ct, steps, gk)
    assert len(many) == 3 and [dec(c) for c in many] == single
    assert all(c.polynomial_count() == 2 and c.parms_id() == ct.parms_id() and not c.is_ntt_form() for c in many)
    summed = ev.rotate_sum_new(ct, steps, gk)
    assert dec(summed) == [sum(s[i] for s in single) % t for i in range(n)]
    # the spellings with a destination and keyword arguments
    dest = pytroy.Ciphertext()
    ev.rotate_sum(encrypted=ct, steps=steps, galois_keys=gk, destination=dest)
    assert dest.data() == summed.data()
    dests = [pytroy.Ciphertext() for _ in steps]
    ev.rotate_many(encrypted=ct, steps=steps, galois_keys=gk, destination=dests)
    assert [d.data() for d in dests] == [c.data() for c in many]
    # the same through Galois elements: rotate_rows by one step is the generator 3
    assert ev.apply_galois_sum_new(encrypted=ct, galois_elements=[3], galois_keys=gk).data() == ev.rotate_sum_new(ct, [1], gk).data()
    assert ev.apply_galois_many_new(ct, [3, 9], gk)[1].data() == many[1].data()
    # a step of 0 contributes the ciphertext itself, duplicates count twice
    assert dec(ev.rotate_sum_new(ct, [0, 1, 1], gk)) == [(v[i] + 2 * single[0][i]) % t for i in range(n)]
    assert dec(ev.rotate_sum_new(ct, [0, 0], gk)) == [2 * x % t for x in v]
    z = ev.rotate_many_new(ct, [0, 2, 2], gk)
    assert z[0].data() == ct.data() and dec(z[1]) == single[1] and z[2].data() == z[1].data()
    # a missing key: no NAF chain to fall back to
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.rotate_sum_new(ct, [1, 3], gk)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.rotate_many_new(ct, [3], gk)
    with pytest.raises(ValueError):
        ev.rotate_sum_new(ct, [], gk)
    with pytest.raises(ValueError):
        ev.apply_galois_sum_new(ct, [1], gk)          # the identity is a step of 0, not a Galois element with a key
    pytroy.MemoryPool.destroy_global_pool()


def test_bgv_is_refused(pytroy, dev):
    t, encoder, kg, encryptor, decryptor, ev = _batching(pytroy, pytroy.SchemeType.BGV, 17)
    ct = encryptor.encrypt_asymmetric_new(encoder.encode_simd_new([1, 2, 3]))
    gk = kg.create_galois_keys_from_steps([1], False)
    assert encoder.decode_simd_new(decryptor.decrypt_new(ev.rotate_rows_new(ct, 1, gk))).tolist()[:2] == [2, 3]
    for name, call in (("rotate_sum", lambda: ev.rotate_sum_new(ct, [1], gk)), ("rotate_many", lambda: ev.rotate_many_new(ct, [1], gk)),
                       ("apply_galois_sum", lambda: ev.apply_galois_sum_new(ct, [3], gk)), ("apply_galois_many", lambda: ev.apply_galois_many_new(ct, [3], gk))):
        with pytest.raises(ValueError, match=name):
            call()
    pytroy.MemoryPool.destroy_global_pool()


def test_ckks_rotate_sum(pytroy, dev):
    """the parameters, the scale and the tolerance of the project's CKKS rotate check (tests/test_pytroy.py::test_ckks_flow_in_python: 2e-2 at scale 2^30)"""
    p = _params(pytroy, pytroy.SchemeType.CKKS, 8192, [40, 40, 40, 40])
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Classical128, 99)
    ctx.to_device_inplace()
    enc = pytroy.CKKSEncoder(ctx)
    kg = pytroy.KeyGenerator(ctx)
    encryptor = pytroy.Encryptor(ctx)
    encryptor.set_public_key(kg.create_public_key(False))
    dec = pytroy.Decryptor(ctx, kg.secret_key())
    ev = pytroy.Evaluator(ctx)
    rnd = random.Random(3)
    slots = enc.slot_count()
    z = [complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(slots)]
    c = encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new(z, None, float(1 << 30)))
    steps = [1, 2, 5]
    gk = kg.create_galois_keys_from_steps(steps, False)
    summed = ev.rotate_sum_new(c, steps, gk)
    assert summed.is_ntt_form() and summed.scale() == c.scale() and summed.parms_id() == c.parms_id()
    got = enc.decode_complex64_simd_new(dec.decrypt_new(summed)).tolist()
    assert max(abs(got[i] - sum(z[(i + k) % slots] for k in steps)) for i in range(slots)) < 2e-2
    many = ev.rotate_many_new(c, steps, gk)
    for k, m in zip(steps, many):
        r = enc.decode_complex64_simd_new(dec.decrypt_new(m)).tolist()
        assert max(abs(r[i] - z[(i + k) % slots]) for i in range(slots)) < 2e-2
    pytroy.MemoryPool.destroy_global_pool()
