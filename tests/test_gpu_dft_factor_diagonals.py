"""troyn_ckks_dft_factor_diagonals against tests/dft_factors_spec.py on the handle's own tables: the same words (the bits of every double), both
directions, every mask, the conjugate flag and a constant; N = 1024 and two groups at N = 16384, (12, 1) being the last layer, where +lh and -lh
coincide mod n.  Then troyn_ckks_encode_diagonals on the device table gives the words of troyn_ckks_encode_simd on the specification's values."""
import ctypes as C

import numpy as np
import pytest
import torch

import dft_factors_spec as S
import linear_transform_spec as LS
from test_gpu_ckks_encode import _dev, _setup

pytestmark = pytest.mark.gpu

BITS = (60, 40, 40, 60)
SCALE = 2.0 ** 40
GROUPS_1024 = [(0, 1), (0, 3), (3, 3), (6, 3), (8, 1), (0, 9)]
GROUPS_16384 = [(5, 3), (12, 1)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same_words(got, want):
    """every double bit for bit (a -0 is not a +0)"""
    got = got.cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("first,count", GROUPS_1024)
def test_words_at_1024(O, pkg, dev, first, count, inverse):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    assert enc.lib.troyn_ckks_dft_factor_diagonals_count(enc.h, first, count) == S.diagonal_count(512, first, count)
    assert _same_words(enc.dft_factor_diagonals(first, count, inverse=inverse), S.table(tables, first, count, inverse=inverse))


@pytest.mark.parametrize("inverse", [False, True])
def test_options_at_1024(O, pkg, dev, inverse):
    """each mask on columns and rows, the conjugate flag, a constant != 1 (negative, not a power of two), and all of them at once"""
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    for first, count in ((0, 3), (6, 3)):
        for kw in ({"col_mask": 1}, {"col_mask": 2}, {"row_mask": 1}, {"row_mask": 2}, {"conjugate": True}, {"constant": -0.7310585786300049},
                   {"col_mask": 2, "row_mask": 2, "conjugate": True, "constant": 1.0 / 3.0}, {"col_mask": 1, "row_mask": 2}):
            assert _same_words(enc.dft_factor_diagonals(first, count, inverse=inverse, **kw), S.table(tables, first, count, inverse=inverse, **kw)), (first, count, kw)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("first,count", GROUPS_16384)
def test_words_at_16384(O, pkg, dev, first, count, inverse):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 14, BITS)
    want = S.table(tables, first, count, inverse=inverse, col_mask=1 if inverse else 0, row_mask=0 if inverse else 2, conjugate=not inverse, constant=0.9)
    assert want.shape[0] == (2 if (first, count) == (12, 1) else 15)
    got = enc.dft_factor_diagonals(first, count, inverse=inverse, col_mask=1 if inverse else 0, row_mask=0 if inverse else 2, conjugate=not inverse, constant=0.9)
    assert _same_words(got, want)


def test_refusals_count_zero_and_stream(O, pkg, dev):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    lib, h, n = plan.lib, enc.h, 512
    INVALID = -1
    out = torch.full((15, n, 2), -1.0, dtype=torch.float64, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(first=3, count=3, inverse=0, cm=0, rm=0, conj=0, const=1.0, o=vp(out), hh=h):
        return lib.troyn_ckks_dft_factor_diagonals(hh, first, count, inverse, cm, rm, conj, const, o, st)
    # count == 0 touches nothing, whatever else is passed
    assert call(count=0) == 0 and call(count=0, o=None, first=99, cm=7, const=float("nan")) == 0
    torch.cuda.synchronize()
    assert (out == -1.0).all()
    assert call(hh=None) == INVALID and call(hh=None, count=0) == INVALID
    assert call(o=None) == INVALID and call(o=C.c_void_p(out.data_ptr() + 8)) == INVALID
    # layers outside [0, log2 n] = [0, 9]
    assert call(first=9, count=1) == INVALID and call(first=7, count=3) == INVALID and call(first=0, count=10) == INVALID and call(first=2 ** 32 - 1, count=2) == INVALID
    assert call(cm=3) == INVALID and call(cm=-1) == INVALID and call(rm=3) == INVALID and call(rm=-1) == INVALID
    assert call(const=float("nan")) == INVALID and call(const=float("inf")) == INVALID and call(const=-float("inf")) == INVALID
    torch.cuda.synchronize()
    assert (out == -1.0).all()
    # the count query
    cnt = lib.troyn_ckks_dft_factor_diagonals_count
    assert cnt(h, 3, 3) == 15 and cnt(h, 6, 3) == 8 and cnt(h, 0, 9) == 512 and cnt(h, 8, 1) == 2 and cnt(h, 0, 1) == 3
    assert cnt(h, 3, 0) == 0 and cnt(None, 3, 3) == 0 and cnt(h, 7, 3) == 0 and cnt(h, 10, 1) == 0
    assert call() == 0
    want = S.table(tables, 3, 3)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    # a non-default stream gives the same words
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = enc.dft_factor_diagonals(3, 3)
    side.synchronize()
    assert _same_words(got, want)


@pytest.mark.parametrize("first,count,inverse", [(6, 3, True), (0, 3, False), (3, 3, True)])
def test_encoded_table_is_encode_simd_on_the_specification(O, pkg, dev, first, count, inverse):
    """the device table through troyn_ckks_encode_diagonals = the specification's table, rotated back as linear_transform_spec states, through
    troyn_ckks_encode_simd: word for word, at the key level; every diagonal with a shift of its own"""
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    N, n, L = 1024, 512, 4
    kw = {"col_mask": 1, "constant": 0.25} if inverse else {"row_mask": 2, "conjugate": True}
    table = enc.dft_factor_diagonals(first, count, inverse=inverse, **kw)
    spec = S.table(tables, first, count, inverse=inverse, **kw)
    nd = spec.shape[0]
    pairs = [(a, (37 * a + 5) % n) for a in range(nd)]
    got = enc.encode_diagonals(L, table, torch.from_numpy(np.asarray(pairs, dtype=np.int32)).to(dev), SCALE, n).cpu().numpy()
    values = LS.values_of(spec[..., 0] + 1j * spec[..., 1], pairs, n, N, False)
    want = enc.encode_simd(L, _dev(np.stack([values.real, values.imag], axis=-1), dev), SCALE).cpu().numpy()
    assert got.shape == (nd, L, N)
    assert np.array_equal(got, want)
