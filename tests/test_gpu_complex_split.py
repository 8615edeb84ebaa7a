"""GPU parity of troyn_ckks_complex_split / troyn_ckks_complex_join (Plan.ckks_complex_split / ckks_complex_join): word for word against Python-integer
arithmetic on the same buffers with the mu vector of tests/bootstrap_spec.py built from the plan's own root table, against the composition the header
names (add, sub, dyadic product with the transformed monomial) on the device, the round trip join(split) = 2a, every refusal and batch == 0.
The launch has no item capacity (one row per (item, polynomial, limb), grid.x only), so the batches are 1 and 3."""
import ctypes as C

import numpy as np
import pytest
import torch

import bootstrap_spec as B

pytestmark = pytest.mark.gpu

BITS = [60, 50, 40, 60]      # 60-, 50- and 40-bit moduli in one chain (the last one is never used: L <= 3)
_SETUP = {}


def _setup(O, pkg, dev, n):
    if n not in _SETUP:
        q = O.coeff_modulus_create(n, BITS)
        plan = pkg.Plan(dev, n.bit_length() - 1, q)
        iota = []
        for l in range(len(q)):
            powers = np.zeros(2 * n, dtype=np.uint64)
            pkg.capi.check(plan.lib.troyn_plan_get_root_powers(plan.h, l, 0, powers.ctypes.data_as(pkg.capi.p64)))
            iota.append(int(powers[2]))          # entry 1 = bit_reverse(N/2): (operand, quotient)
        _SETUP[n] = (plan, [int(v) for v in q], iota)
    return _SETUP[n]


def _operands(rng, q, n, L, batch):
    """[batch][2][L][N] canonical residues; 0 and q - 1 in both halves of every row"""
    x = np.zeros((batch, 2, L, n), dtype=np.uint64)
    for l in range(L):
        x[:, :, l] = rng.integers(0, q[l], size=(batch, 2, n), dtype=np.uint64)
        x[:, :, l, 0] = 0
        x[:, :, l, 1] = q[l] - 1
        x[:, :, l, n // 2] = q[l] - 1
        x[:, :, l, n - 1] = 0
    return x


def _dev(pkg, dev, x):
    return pkg.to_device(x, dev)


@pytest.mark.parametrize("n,L,batch", [(1024, 1, 1), (1024, 3, 3), (16384, 1, 3), (16384, 3, 1)])
def test_split_and_join_equal_integer_arithmetic(O, pkg, dev, n, L, batch):
    plan, q, iota = _setup(O, pkg, dev, n)
    rng = np.random.default_rng(1000 * L + batch + n)
    a, b = _operands(rng, q, n, L, batch), _operands(rng, q, n, L, batch)
    b[:, :, :, 1] = 0                                    # (q - 1) - 0 and 0 - (q - 1) both occur
    da, db = _dev(pkg, dev, a), _dev(pkg, dev, b)
    s, d = plan.ckks_complex_split(L, da, db)
    out = plan.ckks_complex_join(L, da, db)
    back = plan.ckks_complex_join(L, s, d)
    torch.cuda.synchronize()
    s, d, out, back = (pkg.to_host(t) for t in (s, d, out, back))
    for l in range(L):
        mu = B.mu_vector(n, q[l], iota[l])
        for i in range(batch):
            for p in range(2):
                al, bl = [int(v) for v in a[i, p, l]], [int(v) for v in b[i, p, l]]
                ws, wd = B.split_rows(al, bl, mu, q[l])
                assert [int(v) for v in s[i, p, l]] == ws, (l, i, p)
                assert [int(v) for v in d[i, p, l]] == wd, (l, i, p)
                assert [int(v) for v in out[i, p, l]] == B.join_rows(al, bl, mu, q[l]), (l, i, p)
                assert [int(v) for v in back[i, p, l]] == [2 * v % q[l] for v in al], (l, i, p)      # a + b - (b - a) = 2a: mu squared is -1


@pytest.mark.parametrize("n", [1024, 16384])
def test_the_composition_the_header_names(O, pkg, dev, n):
    """add, sub and the dyadic product with the forward transform of X^(N/2), on the device"""
    plan, q, iota = _setup(O, pkg, dev, n)
    L, batch = 3, 2
    rng = np.random.default_rng(n)
    da, db = _dev(pkg, dev, _operands(rng, q, n, L, batch)), _dev(pkg, dev, _operands(rng, q, n, L, batch))
    mono = np.zeros((1, 1, L, n), dtype=np.uint64)
    mono[:, :, :, n // 2] = 1
    mu = plan.ntt(_dev(pkg, dev, mono), 1, L)
    torch.cuda.synchronize()
    mu_host = pkg.to_host(mu)
    for l in range(L):
        assert [int(v) for v in mu_host[0, 0, l]] == B.mu_vector(n, q[l], iota[l])       # the halves, from the library's own transform
    mus = mu.expand(batch, 2, L, n).contiguous()
    s, d = plan.ckks_complex_split(L, da, db)
    assert torch.equal(s, plan.add(da, db, L))
    assert torch.equal(d, plan.dyadic_product(plan.sub(db, da, L), mus, L))
    assert torch.equal(plan.ckks_complex_join(L, da, db), plan.add(da, plan.dyadic_product(db, mus, L), L))
    # an output may be one of the inputs
    a2 = da.clone()
    plan.ckks_complex_join(L, a2, db, out=a2)
    assert torch.equal(a2, plan.add(da, plan.dyadic_product(db, mus, L), L))


def test_refusals_and_the_empty_batch(O, pkg, dev):
    n = 1024
    plan, q, _ = _setup(O, pkg, dev, n)
    lib, h = plan.lib, plan.h
    x = _dev(pkg, dev, _operands(np.random.default_rng(5), q, n, 2, 1))
    y, z = torch.empty_like(x), torch.empty_like(x)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.troyn_ckks_complex_split(h, 2, None, None, None, None, 0, None) == 0         # batch 0: a no-op, no pointer looked at
    assert lib.troyn_ckks_complex_join(h, 2, None, None, None, 0, None) == 0
    bad = pkg.capi.TroynInvalidArgument
    for L in (0, len(q) + 1):
        with pytest.raises(bad, match=r"\[troyn_ckks_complex_split\].*L outside"):
            pkg.capi.check(lib.troyn_ckks_complex_split(h, L, p(x), p(x), p(y), p(z), 1, None))
        with pytest.raises(bad, match=r"\[troyn_ckks_complex_join\].*L outside"):
            pkg.capi.check(lib.troyn_ckks_complex_join(h, L, p(x), p(x), p(y), 1, None))
    for args in ((None, p(x), p(y), p(z)), (p(x), None, p(y), p(z)), (p(x), p(x), None, p(z)), (p(x), p(x), p(y), None)):
        with pytest.raises(bad, match=r"\[troyn_ckks_complex_split\].*null"):
            pkg.capi.check(lib.troyn_ckks_complex_split(h, 2, *args, 1, None))
    for args in ((None, p(x), p(y)), (p(x), None, p(y)), (p(x), p(x), None)):
        with pytest.raises(bad, match=r"\[troyn_ckks_complex_join\].*null"):
            pkg.capi.check(lib.troyn_ckks_complex_join(h, 2, *args, 1, None))
    with pytest.raises(bad, match=r"\[troyn_ckks_complex_split\].*null"):
        pkg.capi.check(lib.troyn_ckks_complex_split(None, 2, p(x), p(x), p(y), p(z), 1, None))
    with pytest.raises(bad, match=r"misaligned"):
        pkg.capi.check(lib.troyn_ckks_complex_join(h, 2, C.c_void_p(x.data_ptr() + 8), p(x), p(y), 1, None))
    with pytest.raises(bad, match=r"same buffer"):
        pkg.capi.check(lib.troyn_ckks_complex_split(h, 2, p(x), p(x), p(y), p(y), 1, None))
    torch.cuda.synchronize()
