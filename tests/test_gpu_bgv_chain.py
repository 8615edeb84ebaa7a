"""troyn_bgv_multiply_relinearize_mod_switch on the GPU: word for word the three device calls it fuses (troyn_dyadic_convolute,
troyn_bgv_relinearize, troyn_bgv_mod_t_and_divide_q_last_ntt) and the oracle's relinearize + mod_t_and_divide_q_last_ntt on the oracle's
dyadic product -- uniform residues and uniform key material, every level of every chain; then the refusals and the empty batch."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# n, prime bit sizes, t, batches: the shapes of the launch paths (tiny generic ring; inv == 1 for both divisions; smallest optimised ring with a
# power-of-two t; integer-class and FP64-class limbs in one chain; whole-limb one-launch inner product; two-pass transforms)
SHAPES = [(64, [30, 30, 30], 257, (1, 3)),
          (64, [30, 30, 30], 2, (1, 3)),
          (1024, [50, 50, 50, 50], 1 << 20, (1, 3)),
          (8192, [60, 40, 40, 60], 65537, (1, 3)),
          (16384, [50, 50, 50, 50], 65537, (1, 3)),
          (32768, [50, 50, 50], 65537, (1,))]


def _setup(O, pkg, dev, n, bits, t):
    q = [int(v) for v in O.coeff_modulus_create(n, bits)]
    return O.Context("bgv", n, q, t), pkg.Plan(dev, n.bit_length() - 1, q), q


def _levels(q, t):
    """every L from K-1 down to 2 whose dropped prime is invertible mod t (the reference refuses the others, as does the library)"""
    return [L for L in range(len(q) - 1, 1, -1) if np.gcd(q[L - 1] % t, t) == 1]


def _composed(pkg, plan, key_level, level, L, a, b, keys_d):
    prod = plan.dyadic_convolute(a, 2, b, 2, L)
    return level.mod_t_and_divide_q_last_ntt(key_level.relinearize(L, prod, keys_d), 2)


def test_no_shape_loses_every_level(O):
    """the skip of a non-invertible dropped prime must leave every row of the table with a level to test (CPU arithmetic only)"""
    for n, bits, t, _ in SHAPES:
        q = [int(v) for v in O.coeff_modulus_create(n, bits)]
        assert np.gcd(q[-1] % t, t) == 1, (n, bits, t)
        assert _levels(q, t), (n, bits, t)
        if n < 32768:
            assert _levels(q, t) == list(range(len(q) - 1, 1, -1)), (n, bits, t)      # in fact none is skipped


@pytest.mark.parametrize("n,bits,t,batches", SHAPES)
def test_fused_equals_three_calls_and_oracle(O, pkg, dev, n, bits, t, batches):
    ctx, plan, q = _setup(O, pkg, dev, n, bits, t)
    K = len(q)
    key_level = pkg.Bgv(plan, K, t)
    assert _levels(q, t)
    for L in _levels(q, t):
        level = pkg.Bgv(plan, L, t)
        keys_h = ctx.random_keys(40 + L, L)
        keys_d = [pkg.to_device(k, dev) for k in keys_h]
        items = max(batches)
        a = np.stack([ctx.random_ct(5 * L + i, 2, L) for i in range(items)])
        b = np.stack([ctx.random_ct(70 + 5 * L + i, 2, L) for i in range(items)])
        da, db = pkg.to_device(a, dev), pkg.to_device(b, dev)
        want_dev = pkg.to_host(_composed(pkg, plan, key_level, level, L, da, db, keys_d))
        want = np.stack([ctx.mod_t_and_divide_q_last_ntt(L, ctx.relinearize(L, True, ctx.ckks_multiply(L, a[i], b[i]), keys_h)) for i in range(items)])
        assert np.array_equal(want_dev, want), L                      # the yardstick itself
        for batch in batches:
            got = pkg.to_host(key_level.multiply_relinearize_mod_switch(level, da[:batch].contiguous(), db[:batch].contiguous(), keys_d))
            assert got.shape == (batch, 2, L - 1, n)
            mism = int(np.count_nonzero(got != want[:batch]))
            assert mism == 0, "L=%d batch=%d: %d of %d words differ from the oracle" % (L, batch, mism, got.size)
            assert np.array_equal(got, want_dev[:batch]), (L, batch)


@pytest.mark.parametrize("n,bits,t", [(64, [30, 30, 30], 257), (8192, [60, 40, 40, 60], 65537)])
def test_input_edges(O, pkg, dev, n, bits, t):
    """rows that are all q - 1, and a zero b (the composition then divides zero)"""
    ctx, plan, q = _setup(O, pkg, dev, n, bits, t)
    K, L = len(q), len(q) - 1
    key_level, level = pkg.Bgv(plan, K, t), pkg.Bgv(plan, L, t)
    keys_d = [pkg.to_device(k, dev) for k in ctx.random_keys(3, L)]
    top = np.empty((1, 2, L, n), dtype=np.uint64)
    for j in range(L):
        top[:, :, j, :] = q[j] - 1
    rnd = ctx.random_ct(17, 2, L)[None]
    zero = np.zeros_like(top)
    for x, y in ((top, top), (rnd, zero)):
        dx, dy = pkg.to_device(x, dev), pkg.to_device(y, dev)
        got = pkg.to_host(key_level.multiply_relinearize_mod_switch(level, dx, dy, keys_d))
        assert np.array_equal(got, pkg.to_host(_composed(pkg, plan, key_level, level, L, dx, dy, keys_d)))
        if y is zero:
            assert not got.any()


def test_refusals_and_empty_batch(O, pkg, dev):
    n, t = 1024, 65537
    ctx, plan, q = _setup(O, pkg, dev, n, [40, 40, 40, 40], t)
    K, L = len(q), len(q) - 1
    lib = plan.lib
    key_level, level = pkg.Bgv(plan, K, t), pkg.Bgv(plan, L, t)
    keys_d = [pkg.to_device(k, dev) for k in ctx.random_keys(3, L)]
    a = pkg.to_device(ctx.random_ct(1, 2, L)[None], dev)
    b = pkg.to_device(ctx.random_ct(2, 2, L)[None], dev)
    # one buffer for the aliasing cases: [a-sized | out-sized] words
    out = torch.empty((2 * (L - 1) * n + 2,), dtype=torch.int64, device=dev)
    nbytes = lib.troyn_bgv_multiply_relinearize_mod_switch_workspace_bytes(key_level.h, L, 1)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kp = (C.c_void_p * L)(*[k.data_ptr() for k in keys_d])
    p = lambda x: C.c_void_p(x.data_ptr())

    def raw(kl=key_level.h, lv=level.h, a_=p(a), b_=p(b), kp_=kp, out_=p(out), ws_=p(ws), bytes_=nbytes, batch=1):
        return lib.troyn_bgv_multiply_relinearize_mod_switch(kl, lv, a_, b_, kp_, out_, ws_, bytes_, batch, stream)

    want = pkg.to_host(_composed(pkg, plan, key_level, level, L, a, b, keys_d))
    assert raw() == 0
    assert np.array_equal(pkg.to_host(out[:2 * (L - 1) * n]).reshape(1, 2, L - 1, n), want)
    # TROYN_E_INVALID
    assert raw(kl=None) == -1 and raw(lv=None) == -1
    assert raw(a_=None) == -1 and raw(b_=None) == -1 and raw(kp_=None) == -1 and raw(out_=None) == -1 and raw(ws_=None) == -1
    assert raw(a_=C.c_void_p(a.data_ptr() + 8)) == -1 and b"misaligned" in lib.troyn_last_error()
    assert raw(out_=C.c_void_p(out.data_ptr() + 8)) == -1 and b"misaligned" in lib.troyn_last_error()
    other_plan = pkg.Plan(dev, 10, q)
    assert raw(lv=pkg.Bgv(other_plan, L, t).h) == -1                      # another plan
    assert raw(lv=pkg.Bgv(plan, L, 257).h) == -1                          # another t
    assert raw(kl=level.h) == -1 and b"key level" in lib.troyn_last_error()      # key_level not at the key level
    assert raw(lv=key_level.h) == -1                                      # L = K
    assert raw(lv=pkg.Bgv(plan, 1, t).h) == -1                            # L = 1
    assert raw(kp_=(C.c_void_p * L)(keys_d[0].data_ptr(), None, keys_d[2].data_ptr())) == -1
    assert raw(out_=C.c_void_p(a.data_ptr() + 16)) == -1 and b"overlaps" in lib.troyn_last_error()
    assert raw(out_=p(b)) == -1 and b"overlaps" in lib.troyn_last_error()
    # TROYN_E_MODULUS: t = q_last of the level / of the key level
    for bad_t, which in ((q[L - 1], "lv"), (q[K - 1], "kl")):
        kl2, lv2 = pkg.Bgv(plan, K, bad_t), pkg.Bgv(plan, L, bad_t)
        assert raw(kl=kl2.h, lv=lv2.h) == -2, which
        assert b"[RNSTool::RNSTool] Unable to invert q[last] mod t." in lib.troyn_last_error()
    # TROYN_E_WORKSPACE
    assert raw(bytes_=nbytes - 8) == -3 and b"workspace too small" in lib.troyn_last_error()
    # batch == 0: nothing is looked at
    assert raw(a_=None, b_=None, out_=None, ws_=None, bytes_=0, batch=0) == 0
    # the refused calls wrote nothing
    torch.cuda.synchronize()
    assert np.array_equal(pkg.to_host(out[:2 * (L - 1) * n]).reshape(1, 2, L - 1, n), want)
