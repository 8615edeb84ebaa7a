"""The CKKS encoder's C-ABI entries (troyn_ckks_*) against the numpy specification (tests/ckks_encode_spec.py), bit for bit.

The specification is fed the tables of troyn_ckks_get_tables, so it transforms with the doubles the device reads; the forward / inverse NTT
around it is the oracle's.  Sizes: N = 1024, N = 8192 (the largest one-workgroup transform) and N = 16384 (the first two-pass size)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ckks_encode_spec as S

pytestmark = pytest.mark.gpu

SIZES = [10, 13, 14]
_cache = {}


def _setup(O, pkg, dev, log_n, bits):
    key = (log_n, tuple(bits))
    if key not in _cache:
        n = 1 << log_n
        moduli = O.coeff_modulus_create(n, list(bits))
        plan = pkg.Plan(dev, log_n, moduli)
        enc = plan.ckks_handle()
        _cache[key] = (plan, enc, moduli, enc.tables(), [O.NTTTables(log_n, q) for q in moduli])
    return _cache[key]


def _ntt(O, rows, log_n, tabs, inverse=False):
    L = rows.shape[0]
    fn = O.ntt_inverse if inverse else O.ntt_forward
    return fn(np.ascontiguousarray(rows, dtype=np.uint64).copy().reshape(-1), 1, L, log_n, tabs[:L]).reshape(L, 1 << log_n)


def _values(rng, batch, count, lo=-3.0, hi=3.0):
    return rng.uniform(lo, hi, (batch, count, 2))


def _spec_simd(O, v, scale, moduli, L, tables, log_n, tabs):
    res, too_large = S.residues(S.simd_coefficients(v[:, 0], v[:, 1], scale, tables), moduli[:L])
    return _ntt(O, res, log_n, tabs), too_large


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.mark.parametrize("log_n", SIZES)
def test_tables_are_the_formulas(O, pkg, dev, log_n):
    _, _, _, (index_map, roots, inv_roots), _ = _setup(O, pkg, dev, log_n, (60, 40, 40, 60))
    want_map, want_roots, want_inv = S.numpy_tables(log_n)
    assert np.array_equal(index_map, want_map)
    assert np.max(np.abs(roots - want_roots)) <= 2.0 ** -52 and np.max(np.abs(inv_roots - want_inv)) <= 2.0 ** -52
    assert not roots[0].any() and not inv_roots[0].any()


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("L", [3, 4])
def test_encode_simd_matches_spec(O, pkg, dev, log_n, L):
    """chain {60,40,40,60}: data level (L = 3) and key level (L = 4); distinct items, negative values, count < N/2"""
    plan, enc, moduli, tables, tabs = _setup(O, pkg, dev, log_n, (60, 40, 40, 60))
    n = 1 << log_n
    rng = np.random.default_rng(100 + log_n + L)
    for count in (n // 2, 37):
        v = _values(rng, 3, count)
        got = pkg.to_host(enc.encode_simd(L, _dev(v, dev), 2.0 ** 40))
        for b in range(3):
            want, _ = _spec_simd(O, v[b], 2.0 ** 40, moduli, L, tables, log_n, tabs)
            assert np.array_equal(got[b], want), (count, b)


@pytest.mark.parametrize("log_n", SIZES)
def test_encode_high_word_and_too_large(O, pkg, dev, log_n):
    """scale 2^70 on two 60-bit primes: coefficients above 2^64 (hi != 0); a too-large item between two good ones"""
    plan, enc, moduli, tables, tabs = _setup(O, pkg, dev, log_n, (60, 60))
    n = 1 << log_n
    rng = np.random.default_rng(7 + log_n)
    v = _values(rng, 3, n // 2)
    got, flags = enc.encode_simd(2, _dev(v, dev), 2.0 ** 70, flags=True)
    got = pkg.to_host(got)
    assert flags.cpu().tolist() == [0, 0, 0]
    for b in range(3):
        coeffs = S.simd_coefficients(v[b][:, 0], v[b][:, 1], 2.0 ** 70, tables)
        assert np.max(np.abs(coeffs)) > 2.0 ** 64
        want, too = _spec_simd(O, v[b], 2.0 ** 70, moduli, 2, tables, log_n, tabs)
        assert not too and np.array_equal(got[b], want), b
    v[1] *= 2.0 ** 68                               # |coefficient| ~ 2^132 .. 2^134 at scale 2^70
    assert S.residues(S.simd_coefficients(v[1][:, 0], v[1][:, 1], 2.0 ** 70, tables), moduli)[1]
    got2, flags = enc.encode_simd(2, _dev(v, dev), 2.0 ** 70, flags=True)
    got2 = pkg.to_host(got2)
    assert flags.cpu().tolist() == [0, 1, 0]
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[2], got[2])
    # without a flag array the call still succeeds and the neighbours are unaffected
    got3 = pkg.to_host(enc.encode_simd(2, _dev(v, dev), 2.0 ** 70))
    assert np.array_equal(got3[0], got[0]) and np.array_equal(got3[2], got[2])


@pytest.mark.parametrize("log_n", [10, 14])
def test_encode_polynomial_and_empty(O, pkg, dev, log_n):
    plan, enc, moduli, tables, tabs = _setup(O, pkg, dev, log_n, (60, 40, 40, 60))
    n = 1 << log_n
    rng = np.random.default_rng(3)
    for count in (n, 5):
        c = rng.uniform(-1000, 1000, (2, count))
        c[0, 0], c[0, 1] = 2.5 / 2.0 ** 30, 3.5 / 2.0 ** 30                     # ties: 2 and 4
        got = pkg.to_host(enc.encode_polynomial(3, _dev(c, dev), 2.0 ** 30))
        for b in range(2):
            res, _ = S.residues(S.polynomial_coefficients(c[b], 2.0 ** 30, n), moduli[:3])
            assert np.array_equal(got[b], _ntt(O, res, log_n, tabs)), (count, b)
    # count == 0 encodes zero, through both entries
    z = torch.empty((2, 0, 2), dtype=torch.float64, device=dev)
    assert not pkg.to_host(enc.encode_simd(3, z, 2.0 ** 30)).any()
    assert not pkg.to_host(enc.encode_polynomial(3, z.reshape(2, 0), 2.0 ** 30)).any()


def test_two_round_strided_pass(O, pkg, dev):
    """N = 65536: the strided pass runs two register rounds with an LDS exchange between them (one round at N = 16384); one encoding and both decoders"""
    log_n, L, scale = 16, 2, 2.0 ** 40
    plan, enc, moduli, tables, tabs = _setup(O, pkg, dev, log_n, (60, 40, 60))
    n = 1 << log_n
    rng = np.random.default_rng(16)
    v = _values(rng, 1, n // 2)
    coeffs = S.simd_coefficients(v[0][:, 0], v[0][:, 1], scale, tables)
    res, too = S.residues(coeffs, moduli[:L])
    plain = enc.encode_simd(L, _dev(v, dev), scale)
    assert not too and np.array_equal(pkg.to_host(plain)[0], _ntt(O, res, log_n, tabs))
    want = S.polynomial_from_residues(res, moduli[:L], scale)
    assert np.array_equal(enc.decode_polynomial(L, plain, scale).cpu().numpy()[0], want)
    wr, wi = S.simd_from_coefficients(want, tables)
    got = enc.decode_simd(L, plain, scale).cpu().numpy()[0]
    assert np.array_equal(got[:, 0], wr) and np.array_equal(got[:, 1], wi)


def _random_plain(O, rng, moduli, L, n, log_n, tabs):
    res = np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in moduli[:L]])
    return res, _ntt(O, res, log_n, tabs)


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("L", [1, 3])
def test_decode_matches_spec(O, pkg, dev, log_n, L):
    """uniformly random canonical residues (multi-word, both signs) and encoded data, both decode entries"""
    plan, enc, moduli, tables, tabs = _setup(O, pkg, dev, log_n, (60, 40, 40, 60))
    n = 1 << log_n
    rng = np.random.default_rng(900 + log_n + L)
    items = [_random_plain(O, rng, moduli, L, n, log_n, tabs) for _ in range(2)]
    v = _values(rng, 1, n // 2)[0]
    enc_res, _ = S.residues(S.simd_coefficients(v[:, 0], v[:, 1], 2.0 ** 30, tables), moduli[:L])
    items.append((enc_res, _ntt(O, enc_res, log_n, tabs)))
    plain = pkg.to_device(np.stack([p for _, p in items]), dev)
    scale = 2.0 ** 30
    got_poly = enc.decode_polynomial(L, plain, scale).cpu().numpy()
    got_simd = enc.decode_simd(L, plain, scale).cpu().numpy()
    for b, (res, _) in enumerate(items):
        want = S.polynomial_from_residues(res, moduli[:L], scale)
        assert np.array_equal(got_poly[b], want), b
        wr, wi = S.simd_from_coefficients(want, tables)
        assert np.array_equal(got_simd[b][:, 0], wr) and np.array_equal(got_simd[b][:, 1], wi), b
    signs = S.compose(items[0][0], moduli[:L])
    assert min(signs) < 0 < max(signs)
    if L == 3:
        assert max(abs(x) for x in signs) > 1 << 128


def test_decode_rounding_boundaries(O, pkg, dev):
    plan, enc, moduli, tables, tabs = _setup(O, pkg, dev, 10, (60, 60))
    Q = moduli[0] * moduli[1]
    cases = [(1 << 53) + 1, (1 << 53) + 3, (1 << 54) + 3, -((1 << 53) + 1), -((1 << 53) + 3), -5, 0, Q // 2, -(Q // 2), (1 << 117) + (1 << 64) + 1, (1 << 117) + (1 << 64),
             (1 << 64) - 1, 1 << 64, -(1 << 64)]
    res = np.zeros((2, 1024), dtype=np.uint64)
    for i, q in enumerate(moduli):
        res[i][:len(cases)] = [x % q for x in cases]
    got = enc.decode_polynomial(2, pkg.to_device(_ntt(O, res, 10, tabs)[None], dev), 3.0).cpu().numpy()[0]
    want = S.polynomial_from_residues(res, moduli, 3.0)
    assert want[:len(cases)].tolist() == [float(x) / 3.0 for x in cases]
    assert np.array_equal(got, want)


def test_batch_zero_errors_and_stream(O, pkg, dev):
    plan, enc, moduli, tables, tabs = _setup(O, pkg, dev, 10, (60, 40, 40, 60))
    lib, h, n = plan.lib, enc.h, 1024
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
    v = _dev(_values(np.random.default_rng(1), 2, 512), dev)
    out = torch.full((2, 3, n), -1, dtype=torch.int64, device=dev)
    nbytes = lib.troyn_ckks_workspace_bytes(h, 3, 2)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def simd(L=3, values=vp(v), count=512, scale=2.0 ** 30, o=vp(out), w=vp(ws), wb=nbytes, batch=2, hh=h):
        return lib.troyn_ckks_encode_simd(hh, L, values, count, scale, o, None, w, wb, batch, st)
    # batch == 0 touches nothing (null buffers are fine)
    assert simd(values=None, o=None, w=None, wb=0, batch=0) == 0
    assert simd(values=None, o=None, w=None, wb=0, batch=0, scale=-1.0, count=10 ** 6) == 0
    assert lib.troyn_ckks_decode_simd(h, 3, None, 1.0, None, None, 0, 0, st) == 0
    torch.cuda.synchronize()
    assert (out == -1).all()
    assert simd(hh=None) == INVALID and simd(L=0) == INVALID and simd(L=5) == INVALID
    assert simd(values=None) == INVALID and simd(o=None) == INVALID
    assert simd(values=C.c_void_p(v.data_ptr() + 8)) == INVALID and simd(o=C.c_void_p(out.data_ptr() + 8)) == INVALID
    assert simd(count=513) == INVALID
    assert lib.troyn_ckks_encode_polynomial(h, 3, vp(v), n + 1, 2.0 ** 30, vp(out), None, vp(ws), nbytes, 1, st) == INVALID
    assert simd(scale=0.0) == INVALID and simd(scale=-1.0) == INVALID
    assert simd(L=1, scale=2.0 ** 59) == INVALID and simd(L=1, scale=2.0 ** 58) == 0        # log2(scale) + 1 < 60 bits
    # an encoding needs the exchange buffer of the two-pass sizes only: nothing at N = 1024, batch * N * 16 bytes at N = 16384
    assert lib.troyn_ckks_encode_workspace_bytes(h, 2) == 0 and simd(w=None, wb=0) == 0
    plan14, enc14, _, _, _ = _setup(O, pkg, dev, 14, (60, 40, 40, 60))
    need14 = lib.troyn_ckks_encode_workspace_bytes(enc14.h, 2)
    assert need14 >= 2 * 16384 * 16 and lib.troyn_ckks_workspace_bytes(enc14.h, 3, 2) >= need14
    out14 = torch.empty((2, 3, 16384), dtype=torch.int64, device=dev)
    ws14 = torch.empty(need14, dtype=torch.uint8, device=dev)
    for w, wb in ((vp(ws14), need14 - 1), (None, need14)):
        assert lib.troyn_ckks_encode_simd(enc14.h, 3, vp(v), 512, 2.0 ** 30, vp(out14), None, w, wb, 2, st) == WORKSPACE
    assert lib.troyn_ckks_encode_simd(enc14.h, 3, vp(v), 512, 2.0 ** 30, vp(out14), None, vp(ws14), need14, 2, st) == 0
    assert lib.troyn_ckks_decode_simd(h, 3, vp(out), 1.0, vp(v), None, nbytes, 2, st) == WORKSPACE
    assert lib.troyn_ckks_decode_polynomial(h, 3, vp(out), 1.0, vp(v), vp(ws), nbytes - 1, 2, st) == WORKSPACE
    assert lib.troyn_ckks_decode_simd(h, 5, vp(out), 1.0, vp(v), vp(ws), nbytes, 2, st) == INVALID
    assert lib.troyn_ckks_workspace_bytes(h, 0, 1) == 0
    # more than 16 moduli: decode is refused, encode is not
    q17 = O.coeff_modulus_create(n, [30] * 17)
    plan17 = pkg.Plan(dev, 10, q17)
    enc17 = plan17.ckks_handle()
    big = torch.zeros((1, 17, n), dtype=torch.int64, device=dev)
    wb17 = lib.troyn_ckks_workspace_bytes(enc17.h, 17, 1)
    ws17 = torch.empty(wb17, dtype=torch.uint8, device=dev)
    dst = torch.zeros((1, n), dtype=torch.float64, device=dev)
    assert lib.troyn_ckks_decode_polynomial(enc17.h, 17, vp(big), 1.0, vp(dst), vp(ws17), wb17, 1, st) == UNSUPPORTED
    assert lib.troyn_ckks_decode_simd(enc17.h, 17, vp(big), 1.0, vp(dst), vp(ws17), wb17, 1, st) == UNSUPPORTED
    assert lib.troyn_ckks_decode_polynomial(enc17.h, 16, vp(big), 1.0, vp(dst), vp(ws17), wb17, 1, st) == 0
    # a non-default stream gives the same words
    want = pkg.to_host(enc.encode_simd(3, v, 2.0 ** 30))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = enc.encode_simd(3, v, 2.0 ** 30)
        dec = enc.decode_simd(3, got, 2.0 ** 30)
    side.synchronize()
    assert np.array_equal(pkg.to_host(got), want)
    back = dec.cpu().numpy()
    vh = v.cpu().numpy()
    bound = S.round_trip_bound(n, 2.0 ** 30, np.sum(np.hypot(vh[0, :, 0], vh[0, :, 1])))
    assert np.max(np.hypot(back[0, :, 0] - vh[0, :, 0], back[0, :, 1] - vh[0, :, 1])) <= bound
