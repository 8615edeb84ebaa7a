"""troyn_ckks_encode_diagonals against its specification, the existing troyn_ckks_encode_simd on the values the header's formulas give
(tests/linear_transform_spec.py): the same words, in both source modes.  Chain {60,40,40,60}, data level (L = 3) and key level (L = 4);
N = 1024 (one tile), N = 8192 (the largest one-workgroup transform) and N = 16384 (the first two-pass size: only the first pass's load is new)."""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_transform_spec as S
from test_gpu_ckks_encode import _dev, _setup

pytestmark = pytest.mark.gpu

SIZES = [10, 13, 14]
BITS = (60, 40, 40, 60)
SCALE = 2.0 ** 40


def _pairs_t(pairs, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)).view(np.int32)).to(dev)


def _ri(z):
    """complex [...] -> float64 [...][2]"""
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def _complex(rng, *shape):
    return rng.uniform(-3, 3, shape) + 1j * rng.uniform(-3, 3, shape)


def _want(enc, L, values, dev):
    return enc.encode_simd(L, _dev(_ri(values), dev), SCALE).cpu().numpy()


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("L", [3, 4])
def test_diagonals_mode_gives_the_words_of_encode_simd(O, pkg, dev, log_n, L):
    """n = N/2 and n = 16 (sparse packing, heavy repetition); 5 items with the shifts {0, 1, n/2, n-1, 7} over mixed rows of a 3-row table"""
    plan, enc, *_ = _setup(O, pkg, dev, log_n, BITS)
    N = 1 << log_n
    for n in (N // 2, 16):
        rng = np.random.default_rng(1000 * log_n + 10 * L + (n == 16))
        diags = _complex(rng, 3, n)
        pairs = [(2, 0), (0, 1), (1, n // 2), (2, n - 1), (0, 7)]
        values = S.values_of(diags, pairs, n, N, False)
        got = enc.encode_diagonals(L, _dev(_ri(diags), dev), _pairs_t(pairs, dev), SCALE, n).cpu().numpy()
        assert got.shape == (5, L, N)
        assert np.array_equal(got, _want(enc, L, values, dev)), n


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("L", [3, 4])
def test_matrix_mode_gives_the_words_of_encode_simd(O, pkg, dev, log_n, L):
    """n = 64 and n = 16 at every N (a small dense source): the diagonal index and the shift both wrap"""
    plan, enc, *_ = _setup(O, pkg, dev, log_n, BITS)
    N = 1 << log_n
    for n in (64, 16):
        rng = np.random.default_rng(2000 * log_n + 10 * L + n)
        M = _complex(rng, n, n)
        pairs = [(0, 0), (n - 1, 1), (5, n // 2), (n // 2, n - 1), (1, 7)]
        values = S.values_of(M, pairs, n, N, True)
        got = enc.encode_diagonals(L, _dev(_ri(M), dev), _pairs_t(pairs, dev), SCALE, n, matrix=True).cpu().numpy()
        assert np.array_equal(got, _want(enc, L, values, dev)), n
        # ... and of diagonals mode on the matrix's diagonals
        d = S.diagonals_of(M)
        table = np.stack([d[k] for k in range(n)])
        again = enc.encode_diagonals(L, _dev(_ri(table), dev), _pairs_t(pairs, dev), SCALE, n).cpu().numpy()
        assert np.array_equal(again, got), n


def test_full_size_matrix_at_one_tile(O, pkg, dev):
    """N = 1024, n = N/2 = 512 in matrix mode: every lane reads a row of its own"""
    plan, enc, *_ = _setup(O, pkg, dev, 10, BITS)
    N, n = 1024, 512
    M = _complex(np.random.default_rng(5), n, n)
    pairs = [(0, 0), (511, 511), (17, 256), (256, 1)]
    got = enc.encode_diagonals(3, _dev(_ri(M), dev), _pairs_t(pairs, dev), SCALE, n, matrix=True).cpu().numpy()
    assert np.array_equal(got, _want(enc, 3, S.values_of(M, pairs, n, N, True), dev))


@pytest.mark.parametrize("log_n", [10, 14])
def test_too_large_flags_one_item(O, pkg, dev, log_n):
    """scale 2^70 on two 60-bit primes, one diagonal 2^68 times larger: the item that reads it is flagged and no other; the others keep their words"""
    plan, enc, *_ = _setup(O, pkg, dev, log_n, (60, 60))
    N, n = 1 << log_n, 16
    diags = _complex(np.random.default_rng(log_n), 2, n)
    pairs = [(0, 3), (1, 3), (0, 5)]
    src = _dev(_ri(diags), dev)
    good, flags = enc.encode_diagonals(2, src, _pairs_t(pairs, dev), 2.0 ** 70, n, flags=True)
    assert flags.cpu().tolist() == [0, 0, 0]
    diags[1] *= 2.0 ** 68
    got, flags = enc.encode_diagonals(2, _dev(_ri(diags), dev), _pairs_t(pairs, dev), 2.0 ** 70, n, flags=True)
    assert flags.cpu().tolist() == [0, 1, 0]
    good, got = good.cpu().numpy(), got.cpu().numpy()
    assert np.array_equal(got[0], good[0]) and np.array_equal(got[2], good[2])
    # without a flag array the call succeeds and the neighbours are unaffected
    got = enc.encode_diagonals(2, _dev(_ri(diags), dev), _pairs_t(pairs, dev), 2.0 ** 70, n).cpu().numpy()
    assert np.array_equal(got[0], good[0]) and np.array_equal(got[2], good[2])


def test_out_of_range_pairs_stay_inside_the_source(O, pkg, dev):
    """the header's rule: s_t is masked; a_t is clamped to nd - 1 in diagonals mode and masked in matrix mode"""
    plan, enc, *_ = _setup(O, pkg, dev, 10, BITS)
    n = 16
    rng = np.random.default_rng(9)
    diags, M = _complex(rng, 3, n), _complex(rng, n, n)
    bad = [(3, 16 + 5), (2 ** 32 - 1, 2 ** 32 - 1)]
    got = enc.encode_diagonals(3, _dev(_ri(diags), dev), _pairs_t(bad, dev), SCALE, n).cpu().numpy()
    assert np.array_equal(got, enc.encode_diagonals(3, _dev(_ri(diags), dev), _pairs_t([(2, 5), (2, 15)], dev), SCALE, n).cpu().numpy())
    got = enc.encode_diagonals(3, _dev(_ri(M), dev), _pairs_t(bad, dev), SCALE, n, matrix=True).cpu().numpy()
    assert np.array_equal(got, enc.encode_diagonals(3, _dev(_ri(M), dev), _pairs_t([(3, 5), (15, 15)], dev), SCALE, n, matrix=True).cpu().numpy())


def test_items_zero_errors_and_stream(O, pkg, dev):
    plan, enc, *_ = _setup(O, pkg, dev, 10, BITS)
    lib, h, N, n = plan.lib, enc.h, 1024, 16
    INVALID, WORKSPACE = -1, -3
    diags = _dev(_ri(_complex(np.random.default_rng(1), 3, n)), dev)
    pairs = _pairs_t([(0, 0), (2, 9)], dev)
    out = torch.full((2, 3, N), -1, dtype=torch.int64, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(L=3, src=vp(diags), matrix=0, nn=n, nd=3, pr=vp(pairs), scale=2.0 ** 30, o=vp(out), w=None, wb=0, items=2, hh=h):
        return lib.troyn_ckks_encode_diagonals(hh, L, src, matrix, nn, nd, pr, scale, o, None, w, wb, items, st)
    # items == 0 touches nothing (null buffers are fine)
    assert call(src=None, pr=None, o=None, items=0) == 0
    assert call(src=None, pr=None, o=None, items=0, scale=-1.0, nn=3, nd=0) == 0
    torch.cuda.synchronize()
    assert (out == -1).all()
    assert call(hh=None) == INVALID and call(L=0) == INVALID and call(L=5) == INVALID
    assert call(src=None) == INVALID and call(pr=None) == INVALID and call(o=None) == INVALID
    assert call(src=C.c_void_p(diags.data_ptr() + 8)) == INVALID and call(pr=C.c_void_p(pairs.data_ptr() + 2)) == INVALID
    assert call(o=C.c_void_p(out.data_ptr() + 8)) == INVALID
    assert call(nn=0) == INVALID and call(nn=12) == INVALID and call(nn=1024) == INVALID
    assert call(nd=0) == INVALID and call(nd=0, matrix=1, nn=1) == 0                       # nd is not read in matrix mode (n = 1: one entry)
    assert call(scale=0.0) == INVALID and call(scale=-1.0) == INVALID
    assert call(L=1, scale=2.0 ** 59) == INVALID and call(L=1, scale=2.0 ** 58) == 0        # log2(scale) + 1 < 60 bits
    assert call() == 0
    # the encoder's workspace: nothing at N = 1024, the exchange buffer at N = 16384
    assert lib.troyn_ckks_encode_diagonals_workspace_bytes(h, 2) == 0 and lib.troyn_ckks_encode_diagonals_workspace_bytes(None, 2) == 0
    plan14, enc14, *_ = _setup(O, pkg, dev, 14, BITS)
    need14 = lib.troyn_ckks_encode_diagonals_workspace_bytes(enc14.h, 2)
    assert need14 >= 2 * 16384 * 16
    out14 = torch.empty((2, 3, 16384), dtype=torch.int64, device=dev)
    ws14 = torch.empty(need14, dtype=torch.uint8, device=dev)
    for w, wb in ((vp(ws14), need14 - 1), (None, need14)):
        assert call(hh=enc14.h, o=vp(out14), w=w, wb=wb) == WORKSPACE
    assert call(hh=enc14.h, o=vp(out14), w=vp(ws14), wb=need14) == 0
    # a non-default stream gives the same words
    want = enc.encode_diagonals(3, diags, pairs, 2.0 ** 30, n).cpu().numpy()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = enc.encode_diagonals(3, diags, pairs, 2.0 ** 30, n)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
