"""troyn_sample_ternary_sparse (csrc/crypto_kernels.hpp sample_ternary_sparse_kernel) against tests/sparse_secret_spec.py, word for word: N = 1024 (512
AES blocks: half of the workgroup's 1024 threads own one, the other half none) and N = 16384 (eight blocks, sixteen coefficients, per thread), h in {1, 32, 192, N}, one and three limbs,
from a nonzero block counter; the counter the call reports; its refusals."""
import numpy as np
import pytest
import torch

import sparse_secret_spec as S

pytestmark = pytest.mark.gpu

SEED = (0xC0FFEE, 0x51)
START = 11          # blocks consumed before the call


@pytest.fixture(scope="module", params=[1024, 16384])
def ring(request, O, pkg, dev):
    n = request.param
    q = [int(v) for v in O.coeff_modulus_create(n, [50, 40, 60])]
    w, after = S.words(O, SEED[0], SEED[1], START, n)
    w.setflags(write=False)
    return n, q, pkg.Plan(dev, n.bit_length() - 1, q), w, after.sample_uint64()


def _prng(pkg, plan):
    gpu = pkg.Prng(plan, *SEED)
    gpu.counter = START
    return gpu


@pytest.mark.parametrize("nmod", [1, 3])
@pytest.mark.parametrize("h", [1, 32, 192, "N"])
def test_kernel_equals_the_specification(pkg, ring, h, nmod):
    n, q, plan, w, _ = ring
    h = n if h == "N" else h
    got = pkg.to_host(_prng(pkg, plan).ternary_sparse(nmod, h))
    want = S.ternary_sparse(w, h, q[:nmod])
    assert got.shape == want.shape and int(np.count_nonzero(got[0])) == h
    assert np.array_equal(got, want)


def test_counter_advances_by_half_n_blocks(pkg, ring):
    n, q, plan, w, next_word = ring
    gpu = _prng(pkg, plan)
    gpu.ternary_sparse(2, 32)
    assert gpu.counter == START + n // 2
    assert gpu.sample_uint64() == next_word          # the oracle generator after the same n / 2 blocks


def test_refusals(pkg, ring):
    n, q, plan, w, _ = ring
    for h in (0, n + 1):
        gpu = _prng(pkg, plan)
        with pytest.raises(pkg.capi.TroynInvalidArgument, match=r"\[RandomGenerator::sample_poly_ternary_sparse\].*\(troyn code -1\)"):     # TROYN_E_INVALID
            gpu.ternary_sparse(1, h)
        assert gpu.counter == START
    with pytest.raises(pkg.capi.TroynInvalidArgument, match=r"\[RandomGenerator::sample_poly_ternary_sparse\].*modulus count"):
        _prng(pkg, plan).ternary_sparse(len(q) + 1, 32)
    torch.cuda.synchronize()
