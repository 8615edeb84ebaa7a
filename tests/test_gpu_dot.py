"""GPU parity of the ciphertext dot product: troyn_dyadic_convolute_accumulate (sum of tensor products in one pass) and
troyn_ckks_multiply_accumulate_relinearize_rescale (that sum, one relinearize, one rescale) vs the oracle and vs the composition of the
entries the oracle already pins.  The sum modulo each q_l in canonical form is defined exactly: every comparison is word for word."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_TERMS, MAX_BATCH = 5, 3
_CACHE = {}


def _setup(O, pkg, dev, scheme, n, bits, t=0):
    q = O.coeff_modulus_create(n, bits)
    ctx = O.Context(scheme, n, q, t)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    return ctx, plan, q


def _osum(O, ctx, L, n, terms):
    """sum of equally shaped residue arrays under the first L moduli (orc_add_ps, as tests/test_gpu_cpp_api.py)"""
    acc = np.ascontiguousarray(terms[0], dtype=np.uint64).reshape(-1).copy()
    pcount = acc.size // (L * n)
    for x in terms[1:]:
        out = np.empty_like(acc)
        O.lib().orc_add_ps(O.ptr(acc), O.ptr(np.ascontiguousarray(x).reshape(-1)), pcount, n, ctx.moduli(), L, O.ptr(out))
        acc = out
    return acc.reshape(np.shape(terms[0]))


def _operands(O, n, bits, L):
    """a[t][i], b[t][i] (t < MAX_TERMS, i < MAX_BATCH) and the oracle's product of every pair: computed once per shape, read-only"""
    key = (n, tuple(bits), L)
    if key not in _CACHE:
        q = O.coeff_modulus_create(n, bits)
        ctx = O.Context("ckks", n, q)
        a = np.stack([np.stack([ctx.random_ct(100 + 10 * t + i, 2, L) for i in range(MAX_BATCH)]) for t in range(MAX_TERMS)])
        b = np.stack([np.stack([ctx.random_ct(500 + 10 * t + i, 2, L) for i in range(MAX_BATCH)]) for t in range(MAX_TERMS)])
        prod = np.stack([np.stack([ctx.ckks_multiply(L, a[t, i], b[t, i]) for i in range(MAX_BATCH)]) for t in range(MAX_TERMS)])
        for x in (a, b, prod):
            x.setflags(write=False)
        _CACHE[key] = (ctx, a, b, prod)
    return _CACHE[key]


def _dev(pkg, x, dev):
    """a device copy of a slice of the shared (write-protected) operands"""
    return pkg.to_device(np.array(x), dev)


def _fold(plan, das, dbs, nmod, mod_start=0):
    """terms x dyadic_convolute + add: the composition of the entries this library had before the accumulate"""
    acc = plan.dyadic_convolute(das[0], 2, dbs[0], 2, nmod, mod_start=mod_start)
    for x, y in zip(das[1:], dbs[1:]):
        acc = plan.add(acc, plan.dyadic_convolute(x, 2, y, 2, nmod, mod_start=mod_start), nmod, mod_start=mod_start)
    return acc


# -- 1. accumulate against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", [1, 2, 3, 5])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n,bits,L", [(32, [30, 30, 30, 30], 3), (4096, [36] * 4, 3), (8192, [60, 40, 40, 60], 3)])
def test_accumulate_vs_oracle(O, pkg, dev, n, bits, L, batch, terms):
    ctx, a, b, prod = _operands(O, n, bits, L)
    plan = pkg.Plan(dev, n.bit_length() - 1, ctx.q)
    das = [_dev(pkg, a[t, :batch], dev) for t in range(terms)]
    dbs = [_dev(pkg, b[t, :batch], dev) for t in range(terms)]
    got_t = plan.dyadic_convolute_accumulate(das, dbs, L)
    assert tuple(got_t.shape) == (batch, 3, L, n)
    got = pkg.to_host(got_t)
    for i in range(batch):
        assert np.array_equal(got[i], _osum(O, ctx, L, n, [prod[t, i] for t in range(terms)])), i
    assert torch.equal(got_t, _fold(plan, das, dbs, L))
    for t in range(terms):      # the operands are left untouched
        assert np.array_equal(pkg.to_host(das[t]), a[t, :batch]) and np.array_equal(pkg.to_host(dbs[t]), b[t, :batch])


# -- 2. launch boundaries (32 terms per launch) and the overflow bound ----------------------------------------------------------------
@pytest.mark.parametrize("terms", [31, 32, 33, 64, 65])
def test_launch_boundaries_and_overflow_bound(O, pkg, dev, terms):
    """every operand word q_l - 1 under 60-bit moduli: the input that wraps a 128-bit accumulator if a launch took more than 32 terms
    ((q-1)^2 = 1 mod q, so out[0] = out[2] = terms, out[1] = 2 terms); then uniformly random operands against the oracle composition"""
    n, nmod = 64, 2
    ctx, plan, q = _setup(O, pkg, dev, "ckks", n, [60, 60])
    assert all(int(v).bit_length() == 60 for v in q)
    top = np.empty((1, 2, nmod, n), dtype=np.uint64)
    for l in range(nmod):
        top[:, :, l, :] = np.uint64(int(q[l]) - 1)
    # distinct buffers per term (equal words): the kernel reads `terms` different pointers
    das = [pkg.to_device(top, dev) for _ in range(terms)]
    dbs = [pkg.to_device(top, dev) for _ in range(terms)]
    got = pkg.to_host(plan.dyadic_convolute_accumulate(das, dbs, nmod))
    for l in range(nmod):
        ql = int(q[l])
        assert (got[0, 0, l] == np.uint64(terms % ql)).all() and (got[0, 2, l] == np.uint64(terms % ql)).all(), l
        assert (got[0, 1, l] == np.uint64((2 * terms) % ql)).all(), l
    ra = [ctx.random_ct(1000 + t, 2, nmod) for t in range(terms)]
    rb = [ctx.random_ct(3000 + t, 2, nmod) for t in range(terms)]
    exp = _osum(O, ctx, nmod, n, [ctx.ckks_multiply(nmod, x, y) for x, y in zip(ra, rb)])
    got = pkg.to_host(plan.dyadic_convolute_accumulate([pkg.to_device(x[None], dev) for x in ra], [pkg.to_device(y[None], dev) for y in rb], nmod))
    assert np.array_equal(got[0], exp)


# -- 3. accumulate=True -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits,L", [(32, [30, 30, 30, 30], 3), (4096, [36] * 4, 3)])
def test_accumulate_flag(O, pkg, dev, n, bits, L):
    ctx, a, b, prod = _operands(O, n, bits, L)
    plan = pkg.Plan(dev, n.bit_length() - 1, ctx.q)
    batch = 2
    das = [_dev(pkg, a[t, :batch], dev) for t in range(5)]
    dbs = [_dev(pkg, b[t, :batch], dev) for t in range(5)]
    whole = plan.dyadic_convolute_accumulate(das, dbs, L)
    # 5 terms as 2 + 3 across two calls
    out = plan.dyadic_convolute_accumulate(das[:2], dbs[:2], L)
    ret = plan.dyadic_convolute_accumulate(das[2:], dbs[2:], L, out=out, accumulate=True)
    assert ret is out and torch.equal(out, whole)
    # from a random canonical `out`: that value plus the sum
    start = np.stack([ctx.random_ct(900 + i, 3, L) for i in range(batch)])
    out = pkg.to_device(start, dev)
    plan.dyadic_convolute_accumulate(das, dbs, L, out=out, accumulate=True)
    got = pkg.to_host(out)
    for i in range(batch):
        assert np.array_equal(got[i], _osum(O, ctx, L, n, [start[i]] + [prod[t, i] for t in range(5)])), i
    # accumulate=False overwrites whatever `out` held
    out = pkg.to_device(start, dev)
    plan.dyadic_convolute_accumulate(das, dbs, L, out=out)
    assert torch.equal(out, whole)


# -- 4. mid-chain slice -------------------------------------------------------------------------------------------------------------------
def test_mid_chain_slice(O, pkg, dev):
    n, bits, L = 4096, [36] * 4, 3
    ctx, a, b, prod = _operands(O, n, bits, L)
    plan = pkg.Plan(dev, n.bit_length() - 1, ctx.q)
    batch, terms = 2, 3
    das = [_dev(pkg, a[t, :batch, :, 1:3], dev) for t in range(terms)]     # limbs 1, 2: moduli 1, 2 of the four-modulus plan
    dbs = [_dev(pkg, b[t, :batch, :, 1:3], dev) for t in range(terms)]
    got_t = plan.dyadic_convolute_accumulate(das, dbs, 2, mod_start=1)
    got = pkg.to_host(got_t)
    for i in range(batch):
        assert np.array_equal(got[i], _osum(O, ctx, L, n, [prod[t, i] for t in range(terms)])[:, 1:3]), i
    assert torch.equal(got_t, _fold(plan, das, dbs, 2, mod_start=1))


# -- 5. the chain entry against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", [1, 4])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n,bits,L", [(8192, [40] * 4, 3), (16384, [50] * 6, 5), (8192, [60, 40, 40, 60], 3), (4096, [36] * 4, 3)])
def test_chain_vs_oracle(O, pkg, dev, n, bits, L, batch, terms):
    ctx, a, b, prod = _operands(O, n, bits, L)
    plan = pkg.Plan(dev, n.bit_length() - 1, ctx.q)
    keys = ctx.random_keys(7, L)
    dkeys = [pkg.to_device(k, dev) for k in keys]
    das = [_dev(pkg, a[t, :batch], dev) for t in range(terms)]
    dbs = [_dev(pkg, b[t, :batch], dev) for t in range(terms)]
    got_t = plan.ckks_multiply_accumulate_relinearize_rescale(L, das, dbs, dkeys)
    assert tuple(got_t.shape) == (batch, 2, L - 1, n)
    got = pkg.to_host(got_t)
    for i in range(batch):
        s = _osum(O, ctx, L, n, [prod[t, i] for t in range(terms)])
        assert np.array_equal(got[i], ctx.mod_switch_scale_to_next(L, ctx.relinearize(L, True, s, keys))), i
    if terms == 1:
        assert torch.equal(got_t, plan.ckks_multiply_relinearize_rescale(L, das[0], dbs[0], dkeys))
    else:
        s3 = plan.dyadic_convolute_accumulate(das, dbs, L)
        assert torch.equal(got_t, plan.divide_and_round_q_last_ntt(L, plan.relinearize(L, s3, dkeys, is_ckks=True, is_ntt_form=True), 2))


# -- 6. argument checks ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks(O, pkg, dev):
    n, bits, L = 32, [30, 30, 30, 30], 3
    ctx, a, b, prod = _operands(O, n, bits, L)
    plan = pkg.Plan(dev, n.bit_length() - 1, ctx.q)
    bad = pkg.capi.TroynInvalidArgument
    da, db = _dev(pkg, a[0, :1], dev), _dev(pkg, b[0, :1], dev)
    dkeys = [pkg.to_device(k, dev) for k in ctx.random_keys(7, L)]
    words = 2 * L * n
    with pytest.raises(bad):                                   # terms = 0
        plan.dyadic_convolute_accumulate([], [], L)
    with pytest.raises(bad):
        plan.ckks_multiply_accumulate_relinearize_rescale(L, [], [], dkeys)
    with pytest.raises(bad):                                   # a null entry
        plan.dyadic_convolute_accumulate([da, None], [db, db], L)
    with pytest.raises(bad):
        plan.ckks_multiply_accumulate_relinearize_rescale(L, [da, da], [db, None], dkeys)
    # a misaligned pointer: a view offset by one word
    pad = torch.zeros(words + 2, dtype=torch.int64, device=dev)
    off = pad[1:1 + words]
    assert off.data_ptr() % 16 == 8
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([da, off], [db, db], L)
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([da], [db], L, out=torch.zeros(3 * L * n + 2, dtype=torch.int64, device=dev)[1:1 + 3 * L * n])
    with pytest.raises(bad):
        plan.ckks_multiply_accumulate_relinearize_rescale(L, [off], [db], dkeys)
    # out aliasing an input
    big = torch.zeros(3 * L * n, dtype=torch.int64, device=dev)
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([big[:words]], [db], L, out=big)
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([da], [big[L * n:L * n + words]], L, out=big)
    # a slice out of range
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([da], [db], L, mod_start=2)
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([da], [db], 0)
    z4 = pkg.to_device(np.zeros((1, 2, 4, n), dtype=np.uint64), dev)
    with pytest.raises(bad):                                   # L = K: no special prime left for the key switch
        plan.ckks_multiply_accumulate_relinearize_rescale(4, [z4], [z4.clone()], dkeys + dkeys[:1])
    # lists of different lengths never reach the library
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([da, da], [db], L)
    # ... nor do operands of different sizes (the kernel reads `batch` items behind every pointer)
    two = torch.zeros((2, 2, L, n), dtype=torch.int64, device=dev)
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([two], [db], L)
    with pytest.raises(bad):
        plan.ckks_multiply_accumulate_relinearize_rescale(L, [da, da], [db, two], dkeys)
    with pytest.raises(bad):
        plan.dyadic_convolute_accumulate([da], [db], L, out=torch.zeros((2, 3, L, n), dtype=torch.int64, device=dev))
    # the size query refuses the levels the entry refuses
    assert plan.lib.troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(plan.h, 4, 1, 1) == 0
    assert plan.lib.troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(plan.h, 1, 1, 1) == 0
    # the chain entry with a workspace one byte short
    lib = plan.lib
    nbytes = lib.troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(plan.h, L, 1, 1)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((1, 2, L - 1, n), dtype=torch.int64, device=dev)
    pa, pb = (C.c_void_p * 1)(da.data_ptr()), (C.c_void_p * 1)(db.data_ptr())
    kp = (C.c_void_p * L)(*[k.data_ptr() for k in dkeys])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.troyn_ckks_multiply_accumulate_relinearize_rescale(plan.h, L, pa, pb, 1, kp, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes - 1, 1, stream)
    assert rc == -3 and b"workspace too small" in lib.troyn_last_error()      # TROYN_E_WORKSPACE, which capi.check raises as an argument error
    with pytest.raises(bad, match="workspace too small"):
        pkg.capi.check(rc)
    # ... and with exactly the queried size it runs and equals the fused single-pair entry
    pkg.capi.check(lib.troyn_ckks_multiply_accumulate_relinearize_rescale(plan.h, L, pa, pb, 1, kp, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, 1, stream))
    assert torch.equal(out, plan.ckks_multiply_relinearize_rescale(L, da, db, dkeys))
    # batch = 0 returns without error
    e2 = torch.empty((0, 2, L, n), dtype=torch.int64, device=dev)
    assert tuple(plan.dyadic_convolute_accumulate([e2], [e2], L).shape) == (0, 3, L, n)
    assert tuple(plan.ckks_multiply_accumulate_relinearize_rescale(L, [e2], [e2], dkeys).shape) == (0, 2, L - 1, n)
    # ... at the C-ABI too, where a caller with nothing to do may pass no destination and no workspace (as the accumulate entry allows)
    assert lib.troyn_dyadic_convolute_accumulate(plan.h, 0, L, pa, pb, 1, None, 0, 0, stream) == 0
    assert lib.troyn_ckks_multiply_accumulate_relinearize_rescale(plan.h, L, pa, pb, 1, kp, None, None, 0, 0, stream) == 0
