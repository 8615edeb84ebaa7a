"""The dispatch seam of the NTT launch layer (csrc/ntt_sizes.hpp, csrc/ntt_launch.inl): every ring size of the table under both arithmetic classes,
and at N = 8192 / 16384 both sides of the small-launch threshold (csrc/launch.hpp is_small_launch: limb_polys * 2 <= CUs takes the two-pass form,
one more limb-polynomial the whole-limb tile).  troyn_ntt forward, then inverse, word for word against the oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THRESHOLD_SIZES = (13, 14)      # the sizes with a small form of their own


@functools.lru_cache(maxsize=None)
def _reference(O, log_n, bits, polys):
    """(modulus, input, oracle forward, oracle inverse of the forward) for `polys` polynomials; computed once per size and class, sliced per launch"""
    n = 1 << log_n
    q = O.coeff_modulus_create(n, [bits])[0]
    tables = [O.NTTTables(log_n, q)]
    x = np.stack([O.fill_uniform(log_n * 1009 + bits * 31 + i, q, n) for i in range(polys)])
    fwd = x.copy().reshape(-1)
    O.ntt_forward(fwd, polys, 1, log_n, tables)
    inv = fwd.copy()
    O.ntt_inverse(inv, polys, 1, log_n, tables)
    for a in (x, fwd, inv):
        a.setflags(write=False)
    return q, x, fwd.reshape(polys, n), inv.reshape(polys, n)


@pytest.mark.parametrize("bits", [40, 60], ids=["fp64-class", "integer-class"])
@pytest.mark.parametrize("log_n", [10, 11, 12, 13, 14, 15, 16, 17])
def test_forward_inverse_at_every_size_and_across_the_threshold(O, pkg, dev, log_n, bits):
    import torch
    n = 1 << log_n
    if log_n in THRESHOLD_SIZES:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        launches = (1, cus // 2, cus // 2 + 1)
    else:
        launches = (1, 3)
    q, x, fwd, inv = _reference(O, log_n, bits, max(launches))
    assert np.array_equal(inv, x), "oracle round trip"
    plan = pkg.Plan(dev, log_n, [q])
    for lp in launches:      # limb-polynomials of the launch: lp items of one polynomial and one limb
        d = pkg.to_device(x[:lp].reshape(lp, 1, 1, n), dev)
        plan.ntt(d, 1, 1)
        got = pkg.to_host(d).reshape(lp, n)
        assert np.array_equal(got, fwd[:lp]), "forward NTT differs from the oracle at %d limb-polynomials" % lp
        plan.ntt(d, 1, 1, inverse=True)
        got = pkg.to_host(d).reshape(lp, n)
        assert np.array_equal(got, inv[:lp]), "inverse NTT differs from the oracle at %d limb-polynomials" % lp
