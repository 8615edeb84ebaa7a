"""troyn_ckks_dft_factor_diagonals_sparse against tests/sparse_bootstrap_spec.py on the handle's own tables: the same words (the bits of every double)
at N = 1024 for n in {2, 4, 64, 256, 512}, both directions, every mask, the conjugate flag and a constant; one case at N = 16384, n = 32; n = N/2
against the existing entry; the refusals.  Then troyn_ckks_encode_diagonals reads the table with that n."""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_transform_spec as LS
import sparse_bootstrap_spec as S
from test_gpu_ckks_encode import _dev, _setup

pytestmark = pytest.mark.gpu

BITS = (60, 40, 40, 60)
SCALE = 2.0 ** 40
SLOT_COUNTS = [2, 4, 64, 256, 512]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same_words(got, want):
    """every double bit for bit (a -0 is not a +0)"""
    got = got.cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.array_equal(_bits(got), _bits(want))


def _groups(m):
    """(first, count): one layer at each end, the whole transform, the top and the bottom group of up to three layers, one in the middle"""
    out = {(0, 1), (m - 1, 1), (0, m), (m - min(3, m), min(3, m)), (0, min(3, m))}
    if m >= 5:
        out.add((1, 3))
    return sorted(out)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", SLOT_COUNTS)
def test_words_at_1024(O, pkg, dev, n, inverse):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    m = n.bit_length() - 1
    for first, count in _groups(m):
        assert enc.lib.troyn_ckks_dft_factor_diagonals_sparse_count(enc.h, n, first, count) == S.diagonal_count(n, first, count)
        got = enc.dft_factor_diagonals_sparse(n, first, count, inverse=inverse)
        assert _same_words(got, S.table(tables, n, first, count, inverse=inverse)), (n, first, count)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", [4, 64])
def test_options_at_1024(O, pkg, dev, n, inverse):
    """each mask on columns and rows, the conjugate flag, a constant != 1 (negative, not a power of two), and all of them at once"""
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    m = n.bit_length() - 1
    for first, count in ((0, min(3, m)), (m - min(3, m), min(3, m))):
        for kw in ({"col_mask": 1}, {"col_mask": 2}, {"row_mask": 1}, {"row_mask": 2}, {"conjugate": True}, {"constant": -0.7310585786300049},
                   {"col_mask": 2, "row_mask": 2, "conjugate": True, "constant": 1.0 / 3.0}, {"col_mask": 1, "row_mask": 2}):
            got = enc.dft_factor_diagonals_sparse(n, first, count, inverse=inverse, **kw)
            assert _same_words(got, S.table(tables, n, first, count, inverse=inverse, **kw)), (n, first, count, kw)


@pytest.mark.parametrize("inverse", [False, True])
def test_words_at_16384(O, pkg, dev, inverse):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 14, BITS)
    n = 32
    for first, count, nd in ((2, 3, 8), (0, 2, 7)):
        kw = dict(inverse=inverse, col_mask=1 if inverse else 0, row_mask=0 if inverse else 2, conjugate=not inverse, constant=0.9)
        want = S.table(tables, n, first, count, **kw)
        assert want.shape == (nd, n, 2)
        assert _same_words(enc.dft_factor_diagonals_sparse(n, first, count, **kw), want)


@pytest.mark.parametrize("inverse", [False, True])
def test_full_n_gives_the_words_of_the_existing_entry(O, pkg, dev, inverse):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    for first, count in ((0, 3), (3, 3), (6, 3), (8, 1), (0, 9)):
        for kw in ({}, {"col_mask": 1, "constant": 0.9}, {"row_mask": 2, "conjugate": True}):
            got = enc.dft_factor_diagonals_sparse(512, first, count, inverse=inverse, **kw)
            assert torch.equal(got.view(torch.int64), enc.dft_factor_diagonals(first, count, inverse=inverse, **kw).view(torch.int64)), (first, count, kw)


def test_refusals_count_zero_and_stream(O, pkg, dev):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    lib, h, n = plan.lib, enc.h, 64
    INVALID = -1
    out = torch.full((15, n, 2), -1.0, dtype=torch.float64, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nn=n, first=0, count=3, inverse=0, cm=0, rm=0, conj=0, const=1.0, o=vp(out), hh=h):
        return lib.troyn_ckks_dft_factor_diagonals_sparse(hh, nn, first, count, inverse, cm, rm, conj, const, o, st)
    # count == 0 touches nothing, whatever else is passed
    assert call(count=0) == 0 and call(count=0, o=None, nn=3, first=99, cm=7, const=float("nan")) == 0
    assert call(hh=None) == INVALID and call(hh=None, count=0) == INVALID
    assert call(o=None) == INVALID and call(o=C.c_void_p(out.data_ptr() + 8)) == INVALID
    # n: a power of two in [2, N/2]
    for bad in (0, 1, 3, 48, 1024, 2048, 2 ** 31, 2 ** 32 - 1):
        assert call(nn=bad, count=1) == INVALID, bad
    # layers outside [0, log2 n] = [0, 6]
    assert call(first=6, count=1) == INVALID and call(first=4, count=3) == INVALID and call(first=0, count=7) == INVALID and call(first=2 ** 32 - 1, count=2) == INVALID
    assert call(nn=2, first=0, count=2) == INVALID and call(nn=2, first=1, count=1) == INVALID
    assert call(cm=3) == INVALID and call(cm=-1) == INVALID and call(rm=3) == INVALID and call(rm=-1) == INVALID
    assert call(const=float("nan")) == INVALID and call(const=float("inf")) == INVALID and call(const=-float("inf")) == INVALID
    torch.cuda.synchronize()
    assert (out == -1.0).all()
    # the count query
    cnt = lib.troyn_ckks_dft_factor_diagonals_sparse_count
    assert cnt(h, 64, 0, 3) == 15 and cnt(h, 64, 3, 3) == 8 and cnt(h, 64, 0, 6) == 64 and cnt(h, 64, 5, 1) == 2 and cnt(h, 64, 0, 1) == 3
    assert cnt(h, 2, 0, 1) == 2 and cnt(h, 512, 3, 3) == 15 and cnt(h, 512, 6, 3) == 8
    assert cnt(h, 64, 3, 0) == 0 and cnt(None, 64, 3, 3) == 0 and cnt(h, 64, 4, 3) == 0 and cnt(h, 64, 7, 1) == 0
    assert cnt(h, 1, 0, 1) == 0 and cnt(h, 3, 0, 1) == 0 and cnt(h, 1024, 0, 1) == 0
    assert call() == 0
    want = S.table(tables, n, 0, 3)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    # a non-default stream gives the same words
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = enc.dft_factor_diagonals_sparse(n, 0, 3)
    side.synchronize()
    assert _same_words(got, want)


def test_encoded_table_is_encode_simd_on_the_specification(O, pkg, dev):
    """the device table through troyn_ckks_encode_diagonals with the same n = the specification's table, rotated back and repeated across the slots as
    linear_transform_spec states, through troyn_ckks_encode_simd: word for word"""
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    N, n, L = 1024, 64, 4
    first, count, kw = 3, 3, {"inverse": True, "col_mask": 1, "constant": 0.25}
    table = enc.dft_factor_diagonals_sparse(n, first, count, **kw)
    spec = S.table(tables, n, first, count, **kw)
    nd = spec.shape[0]
    pairs = [(a, (37 * a + 5) % n) for a in range(nd)]
    got = enc.encode_diagonals(L, table, torch.from_numpy(np.asarray(pairs, dtype=np.int32)).to(dev), SCALE, n).cpu().numpy()
    values = LS.values_of(spec[..., 0] + 1j * spec[..., 1], pairs, n, N, False)
    want = enc.encode_simd(L, _dev(np.stack([values.real, values.imag], axis=-1), dev), SCALE).cpu().numpy()
    assert got.shape == (nd, L, N)
    assert np.array_equal(got, want)
