"""CKKSEncoder's batched methods (pytroy): the words of the device path equal the words of the per-plaintext host path; batched decoding
meets the round-trip bound of tests/ckks_encode_spec.py and agrees with the per-plaintext decoder within it."""
import os
import sys

import numpy as np
import pytest

import ckks_encode_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "troy-nova_amd")
N, BITS, SCALE = 8192, [60, 40, 40, 60], 2.0 ** 40


@pytest.fixture(scope="module")
def env(dev):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import pytroy
    p = pytroy.EncryptionParameters(pytroy.SchemeType.CKKS)
    p.set_poly_modulus_degree(N)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(N, BITS))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Classical128, 11)
    ctx.to_device_inplace()
    return pytroy, ctx, pytroy.CKKSEncoder(ctx)


def _items(seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-2, 2, c) + 1j * rng.uniform(-2, 2, c) for c in (N // 2, 100, N // 2)]


@pytest.mark.parametrize("level", ["data", "key"])
def test_batched_words_equal_the_per_plaintext_words(env, level):
    pytroy, ctx, enc = env
    pid = ctx.first_parms_id() if level == "data" else ctx.key_parms_id()
    values = _items(1)
    batched = enc.encode_complex64_simd_new_batched([v.tolist() for v in values], pid, SCALE)
    assert len(batched) == 3
    for v, b in zip(values, batched):
        one = enc.encode_complex64_simd_new(v.tolist(), pid, SCALE)
        assert b.data() == one.data() and b.parms_id() == one.parms_id() and b.scale() == one.scale() and b.is_ntt_form()
    rng = np.random.default_rng(2)
    coeffs = [rng.uniform(-50, 50, c) for c in (N, 3, 1000)]
    dests = [pytroy.Plaintext() for _ in coeffs]
    enc.encode_float64_polynomial_batched([c.tolist() for c in coeffs], pid, SCALE, dests)
    for c, d in zip(coeffs, dests):
        assert d.data() == enc.encode_float64_polynomial_new(c.tolist(), pid, SCALE).data()


def test_batched_decode_meets_the_bound_and_the_per_plaintext_decoder(env):
    pytroy, ctx, enc = env
    values = _items(3)
    plains = enc.encode_complex64_simd_new_batched([v.tolist() for v in values], None, SCALE)
    got = enc.decode_complex64_simd_batched(plains)
    for v, p, g in zip(values, plains, got):
        full = np.zeros(N // 2, dtype=np.complex128)
        full[:len(v)] = v
        bound = S.round_trip_bound(N, SCALE, np.sum(np.abs(v)))
        err, diff = np.max(np.abs(np.asarray(g) - full)), np.max(np.abs(np.asarray(g) - np.asarray(enc.decode_complex64_simd_new(p))))
        print("round trip %.3e, against the per-plaintext decoder %.3e, bound %.3e" % (err, diff, bound))
        assert err <= bound and diff <= bound
    # separate plaintexts (not windows of one buffer) and the polynomial form
    singles = [enc.encode_float64_polynomial_new([1.5, -2.25, 1000.0], None, SCALE) for _ in range(2)]
    for g in enc.decode_float64_polynomial_batched(singles):
        assert np.max(np.abs(np.asarray(g)[:3] - [1.5, -2.25, 1000.0])) <= 1.0 / SCALE and not np.asarray(g)[3:].any()
        assert np.max(np.abs(np.asarray(g) - np.asarray(enc.decode_float64_polynomial_new(singles[0])))) <= 1.0 / SCALE


def test_device_resident_slices_give_the_same_words(env, dev):
    import torch
    pytroy, ctx, enc = env
    values = _items(4)[:2]
    want = [enc.encode_complex64_simd_new(v.tolist(), None, SCALE).data() for v in values]
    tensors = [torch.from_numpy(np.stack([v.real, v.imag], axis=1).copy()).to(dev) for v in values]       # [count][2] = complex layout
    torch.cuda.synchronize()
    views = [(t.data_ptr(), t.shape[0], True) for t in tensors]
    got = enc.encode_complex64_simd_slice_new_batched(views, None, SCALE)
    assert [g.data() for g in got] == want
    host = np.ascontiguousarray(np.stack([values[0].real, values[0].imag], axis=1))
    mixed = enc.encode_complex64_simd_slice_new_batched([(host.ctypes.data, host.shape[0], False), views[1]], None, SCALE)
    assert [g.data() for g in mixed] == want
    c = torch.arange(16, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert enc.encode_float64_polynomial_slice_new_batched([(c.data_ptr(), 16, True)], None, SCALE)[0].data() == \
        enc.encode_float64_polynomial_new([float(i) for i in range(16)], None, SCALE).data()


def test_too_large_and_bad_arguments_throw(env):
    pytroy, ctx, enc = env
    good = [1.0 + 0j] * 4
    with pytest.raises(Exception, match="encoded values are too large"):
        enc.encode_complex64_simd_new_batched([good, [1e30 + 0j] * (N // 2), good], ctx.key_parms_id(), 2.0 ** 100)
    with pytest.raises(Exception, match="scale out of bounds"):
        enc.encode_complex64_simd_new_batched([good], None, 2.0 ** 200)
    with pytest.raises(Exception, match="Too many input values"):
        enc.encode_complex64_simd_new_batched([[0j] * (N // 2 + 1)], None, SCALE)
    assert enc.encode_complex64_simd_new_batched([], None, SCALE) == []


def test_a_non_ckks_context_is_refused(env):
    pytroy, _, _ = env
    p = pytroy.EncryptionParameters(pytroy.SchemeType.BFV)
    p.set_poly_modulus_degree(N)
    p.set_coeff_modulus(pytroy.CoeffModulus.create(N, BITS))
    p.set_plain_modulus(pytroy.PlainModulus.batching(N, 20))
    ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Classical128, 5)
    ctx.to_device_inplace()
    with pytest.raises(Exception, match="Unsupported scheme"):
        pytroy.CKKSEncoder(ctx)
