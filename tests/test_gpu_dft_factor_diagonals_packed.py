"""troyn_ckks_dft_factor_diagonals_packed against tests/packed_bootstrap_spec.py on the handle's own tables: the same words (the bits of every double, the
-0.0 of a turned zero component and the +0 of absent entries included) at N = 1024 for n in {4, 64, 256}, (first, count) in {(0, 1), (0, log2 n), (1, 2)},
both directions, with and without a constant; one case at N = 16384, n = 4096 (s = 2); rows < n against the sparse entry at 2n; the refusals and
count == 0.  Then troyn_ckks_encode_diagonals reads the table with n = 2n."""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_transform_spec as LS
import packed_bootstrap_spec as P
from test_gpu_ckks_encode import _dev, _setup

pytestmark = pytest.mark.gpu

BITS = (60, 40, 40, 60)
SCALE = 2.0 ** 40
CONSTANT = -0.7310585786300049          # negative, not a power of two


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same_words(got, want):
    """every double bit for bit (a -0 is not a +0)"""
    got = got.cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.array_equal(_bits(got), _bits(want))


def _groups(n):
    m = n.bit_length() - 1
    return [(first, count) for first, count in ((0, 1), (0, m), (1, 2)) if first + count <= m]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", [4, 64, 256])
def test_words_at_1024(O, pkg, dev, n, inverse):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    groups = _groups(n)
    assert len(groups) == (2 if n == 4 else 3)          # (1, 2) does not fit into log2 4 = 2 layers
    for first, count in groups:
        assert enc.lib.troyn_ckks_dft_factor_diagonals_packed_count(enc.h, n, first, count) == P.diagonal_count(n, first, count) == (2 << count) - 1
        for constant in (1.0, CONSTANT):
            got = enc.dft_factor_diagonals_packed(n, first, count, inverse=inverse, constant=constant)
            want = P.table(tables, n, first, count, inverse=inverse, constant=constant)
            assert _same_words(got, want), (n, first, count, constant)
            # rows < n are the sparse entry's at 2n
            sparse = enc.dft_factor_diagonals_sparse(2 * n, first, count, inverse=inverse, constant=constant)
            assert torch.equal(got[:, :n].contiguous().view(torch.int64), sparse[:, :n].contiguous().view(torch.int64)), (n, first, count, constant)


def test_minus_zero_and_absent_entries(O, pkg, dev):
    """forward, layer 0, constant 1: (1, +0) turned by +i is (-0.0, 1); absent entries are +0 in both words"""
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    n = 64
    got = enc.dft_factor_diagonals_packed(n, 0, 1).cpu().numpy()
    want = P.table(tables, n, 0, 1)
    minus_zero = _bits(want) == np.uint64(1 << 63)
    assert minus_zero[:, n:].any() and not minus_zero[:, :n].any()
    assert np.array_equal(_bits(got) == np.uint64(1 << 63), minus_zero)
    absent = (want[..., 0] == 0) & (want[..., 1] == 0) & ~np.signbit(want[..., 0]) & ~np.signbit(want[..., 1])
    assert absent[:, n:].any() and not _bits(got)[absent].any()


@pytest.mark.parametrize("inverse", [False, True])
def test_words_at_16384(O, pkg, dev, inverse):
    """n = N/4 = 4096, s = 2: the table fills the slots; 16 workgroups along the rows"""
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 14, BITS)
    n = 4096
    for first, count in ((0, 2), (9, 3)):
        want = P.table(tables, n, first, count, inverse=inverse, constant=0.9)
        assert want.shape == ((2 << count) - 1, 2 * n, 2)
        assert _same_words(enc.dft_factor_diagonals_packed(n, first, count, inverse=inverse, constant=0.9), want)


def test_refusals_count_zero_and_stream(O, pkg, dev):
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    lib, h, n = plan.lib, enc.h, 64
    INVALID = -1
    out = torch.full((15, 2 * n, 2), -1.0, dtype=torch.float64, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nn=n, first=0, count=3, inverse=0, const=1.0, o=vp(out), hh=h):
        return lib.troyn_ckks_dft_factor_diagonals_packed(hh, nn, first, count, inverse, const, o, st)
    # count == 0 touches nothing, whatever else is passed
    assert call(count=0) == 0 and call(count=0, o=None, nn=3, first=99, const=float("nan")) == 0
    assert call(hh=None) == INVALID and call(hh=None, count=0) == INVALID
    assert call(o=None) == INVALID and call(o=C.c_void_p(out.data_ptr() + 8)) == INVALID
    # n: a power of two in [2, N/4]
    for bad in (0, 1, 3, 48, 512, 1024, 2048, 2 ** 31, 2 ** 32 - 1):
        assert call(nn=bad, count=1) == INVALID, bad
    # layers outside [0, log2 n] = [0, 6]
    assert call(first=6, count=1) == INVALID and call(first=4, count=3) == INVALID and call(first=0, count=7) == INVALID and call(first=2 ** 32 - 1, count=2) == INVALID
    assert call(nn=2, first=0, count=2) == INVALID and call(nn=2, first=1, count=1) == INVALID
    assert call(const=float("nan")) == INVALID and call(const=float("inf")) == INVALID and call(const=-float("inf")) == INVALID
    torch.cuda.synchronize()
    assert (out == -1.0).all()
    # the count query
    cnt = lib.troyn_ckks_dft_factor_diagonals_packed_count
    assert cnt(h, 64, 0, 3) == 15 and cnt(h, 64, 3, 3) == 15 and cnt(h, 64, 0, 6) == 127 and cnt(h, 64, 5, 1) == 3 and cnt(h, 256, 0, 8) == 511
    assert cnt(h, 2, 0, 1) == 3 and cnt(h, 256, 1, 2) == 7
    assert cnt(h, 64, 3, 0) == 0 and cnt(None, 64, 3, 3) == 0 and cnt(h, 64, 4, 3) == 0 and cnt(h, 64, 7, 1) == 0
    assert cnt(h, 1, 0, 1) == 0 and cnt(h, 3, 0, 1) == 0 and cnt(h, 512, 0, 1) == 0 and cnt(h, 1024, 0, 1) == 0
    assert call() == 0
    want = P.table(tables, n, 0, 3)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    # n = 2 is the entry's smallest n (the plans start at 4)
    assert _same_words(enc.dft_factor_diagonals_packed(2, 0, 1, inverse=True), P.table(tables, 2, 0, 1, inverse=True))
    # a non-default stream gives the same words
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = enc.dft_factor_diagonals_packed(n, 0, 3)
    side.synchronize()
    assert _same_words(got, want)


def test_encoded_table_is_encode_simd_on_the_specification(O, pkg, dev):
    """the device table through troyn_ckks_encode_diagonals with n = 2n = the specification's table, rotated back and repeated across the slots as
    linear_transform_spec states, through troyn_ckks_encode_simd: word for word"""
    plan, enc, _, tables, _ = _setup(O, pkg, dev, 10, BITS)
    N, n, L = 1024, 64, 4
    first, count, kw = 0, 3, {"inverse": True, "constant": 0.25}
    table = enc.dft_factor_diagonals_packed(n, first, count, **kw)
    spec = P.table(tables, n, first, count, **kw)
    nd = spec.shape[0]
    pairs = [(a, (37 * a + 5) % (2 * n)) for a in range(nd)]
    got = enc.encode_diagonals(L, table, torch.from_numpy(np.asarray(pairs, dtype=np.int32)).to(dev), SCALE, 2 * n).cpu().numpy()
    values = LS.values_of(spec[..., 0] + 1j * spec[..., 1], pairs, 2 * n, N, False)
    want = enc.encode_simd(L, _dev(np.stack([values.real, values.imag], axis=-1), dev), SCALE).cpu().numpy()
    assert got.shape == (nd, L, N)
    assert np.array_equal(got, want)
