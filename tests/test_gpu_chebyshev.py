"""GPU parity of troyn_ckks_multiply_affine_relinearize_rescale through Plan.multiply_affine_relinearize_rescale: word for word against the
composition the header names (dyadic_convolute, multiply_scalar by alpha, multiply_scalar and add of the addend, the constant, relinearize,
divide_and_round_q_last_ntt) on the device, the tensor stage also against tests/chebyshev_spec.py; every refusal; batch == 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import chebyshev_spec as S

pytestmark = pytest.mark.gpu

CHAINS = {"mixed": [60, 40, 40, 60], "50": [50, 50, 50, 50]}      # the integer and the FP64 arithmetic class
_SETUP = {}


def _setup(O, pkg, dev, n, chain, L):
    """plan, moduli and relinearization keys: once per shape, read-only"""
    key = (n, chain, L)
    if key not in _SETUP:
        q = O.coeff_modulus_create(n, CHAINS[chain])
        ctx = O.Context("ckks", n, q)
        _SETUP[key] = (pkg.Plan(dev, n.bit_length() - 1, q), [int(v) for v in q], [pkg.to_device(k, dev) for k in ctx.random_keys(7, L)])
    return _SETUP[key]


def _ct(rng, q, n, limbs, L, top=False):
    """[2][limbs][N]: canonical residues in the first L limbs (q - 1 everywhere for `top`), words no modulus admits beyond"""
    x = np.full((2, limbs, n), np.uint64((1 << 64) - 1), dtype=np.uint64)
    for l in range(L):
        x[:, l] = np.uint64(q[l] - 1) if top else rng.integers(0, q[l], size=(2, n), dtype=np.uint64)
    return x


def _items(rng, q, n, L, batch, with_constant):
    """the mix of one call: item i takes pattern j = 5 i + 13: addend NULL / L limbs / L + 1 limbs by j % 3, alpha in {1, 2, q - 1} by j // 3 % 3,
    w in {0, 1, q - 1} by j // 9 % 3 (33 items run through all 27); the last item of a batch >= 3 has EVERY word and scalar at q - 1"""
    a, b, c, c_nmod, alpha, w, k = [], [], [], [], [], [], []
    for i in range(batch):
        j = 5 * i + 13
        top = batch >= 3 and i == batch - 1
        a.append(_ct(rng, q, n, L, L, top))
        b.append(_ct(rng, q, n, L, L, top))
        kind = 1 if top else j % 3
        c_nmod.append(L + (kind == 2))
        c.append(None if kind == 0 else _ct(rng, q, n, c_nmod[-1], L, top))
        alpha.append([q[l] - 1 if top else (1, 2, q[l] - 1)[j // 3 % 3] for l in range(L)])
        w.append([q[l] - 1 if top else (0, 1, q[l] - 1)[j // 9 % 3] for l in range(L)])
        k.append([q[l] - 1 if top or i % 3 == 0 else (int(rng.integers(0, q[l])), 0)[i % 3 - 1] for l in range(L)])
    return a, b, c, c_nmod, alpha, w, (k if with_constant else None)


def _rows(plan, x, scal, L):
    """troyn_multiply_scalar takes one scalar for its slice: x [p][L][N] limb by limb"""
    out = torch.empty_like(x)
    for l in range(L):
        out[:, l, :] = plan.multiply_scalar(x[:, l, :].contiguous(), scal[l], 1, mod_start=l)
    return out


def _composed_tensor(plan, dev, n, L, da, db, dc, alpha, w, k):
    """P [3][L][N] of one item from the older entries"""
    p = _rows(plan, plan.dyadic_convolute(da, 2, db, 2, L)[0], alpha, L)
    if dc is not None:
        p[:2] = plan.add(p[:2].contiguous(), _rows(plan, dc[:, :L, :].contiguous(), w, L), L)
    if k is not None:
        const = torch.tensor(np.array(k, dtype=np.uint64).view(np.int64), device=dev).reshape(1, L, 1).expand(1, L, n).contiguous()
        p[:1] = plan.add(p[:1].contiguous(), const, L)
    return p


@pytest.mark.parametrize("with_constant", [False, True])      # `constant` is one table per call: NULL and non-NULL for every shape
@pytest.mark.parametrize("batch", [1, 3, 33])
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("chain", ["mixed", "50"])
@pytest.mark.parametrize("n", [64, 1024, 8192])
def test_word_for_word_with_the_composition(O, pkg, dev, n, chain, L, batch, with_constant):
    plan, q, dkeys = _setup(O, pkg, dev, n, chain, L)
    rng = np.random.default_rng(n + 100 * L + batch)
    a, b, c, c_nmod, alpha, w, k = _items(rng, q, n, L, batch, with_constant)
    da, db = [pkg.to_device(x, dev) for x in a], [pkg.to_device(x, dev) for x in b]
    dc = [None if x is None else pkg.to_device(x, dev) for x in c]
    out = plan.multiply_affine_relinearize_rescale(L, da, db, dc, c_nmod, alpha, w, dkeys, constant=k)
    assert tuple(out.shape) == (batch, 2, L - 1, n)
    p = torch.stack([_composed_tensor(plan, dev, n, L, da[i], db[i], dc[i], alpha[i], w[i], None if k is None else k[i]) for i in range(batch)])
    for i in {0, batch - 1}:      # the tensor stage of the composition is the specification's
        assert np.array_equal(pkg.to_host(p[i]), S.step_direct(q[:L], a[i], b[i], c[i], alpha[i], w[i], None if k is None else k[i])), i
    want = plan.divide_and_round_q_last_ntt(L, plan.relinearize(L, p, dkeys, is_ckks=True, is_ntt_form=True), 2)
    torch.cuda.synchronize()
    bad = [i for i in range(batch) if not torch.equal(out[i], want[i])]
    assert not bad, ("items that differ", bad, "addend", [c[i] is not None for i in bad])
    for x, d in zip(a + b + [x for x in c if x is not None], da + db + [d for d in dc if d is not None]):      # the operands are left untouched
        assert np.array_equal(pkg.to_host(d), x)


def test_double_angle_equals_the_fused_product(O, pkg, dev):
    """alpha = 1, no addend, no constant: the plain multiply -> relinearize -> rescale"""
    n, L = 8192, 3
    plan, q, dkeys = _setup(O, pkg, dev, n, "50", L)
    rng = np.random.default_rng(3)
    x = pkg.to_device(_ct(rng, q, n, L, L), dev)
    out = plan.multiply_affine_relinearize_rescale(L, [x], [x], None, None, [[1] * L], None, dkeys)      # no addend anywhere: the lists may be None
    assert torch.equal(out, plan.ckks_multiply_relinearize_rescale(L, x[None], x[None], dkeys))


# -- refusals ---------------------------------------------------------------------------------------------------------------------
def _raw(pkg, plan, L, a, b, c, c_nmod, alpha, w, k, keys, out, ws, ws_bytes, batch):
    lib = pkg.capi.lib()
    ptrs = lambda v: None if v is None else (C.c_void_p * max(len(v), 1))(*v)
    keep = [None if v is None else np.ascontiguousarray(np.array(v, dtype=np.uint64)).reshape(-1) for v in (alpha, w, k)]      # (alive across the call)
    sc = [None if v is None else v.ctypes.data_as(pkg.capi.p64) for v in keep]
    rc = lib.troyn_ckks_multiply_affine_relinearize_rescale(plan.h, L, ptrs(a), ptrs(b), ptrs(c), None if c_nmod is None else (C.c_uint32 * max(len(c_nmod), 1))(*c_nmod),
                                                            sc[0], sc[1], sc[2], ptrs(keys), out, ws, ws_bytes, batch, None)
    return rc, lib.troyn_last_error().decode()


def test_refusals(O, pkg, dev):
    n, L, batch = 64, 3, 2
    plan, q, dkeys = _setup(O, pkg, dev, n, "mixed", L)
    rng = np.random.default_rng(9)
    a, b, c, c_nmod, alpha, w, k = _items(rng, q, n, L, batch, True)
    c[0], c_nmod[0] = _ct(rng, q, n, L + 1, L), L + 1
    c[1], c_nmod[1] = _ct(rng, q, n, L, L), L
    words = 2 * L * n
    buf = torch.zeros(6 * 2 * (L + 1) * n + 2, dtype=torch.int64, device=dev)      # every operand at a 16-byte aligned base, words to spare for the odd address
    base, at, ptr = buf.data_ptr(), 0, []
    assert base % 16 == 0
    for x in a + b + c:
        buf[at:at + x.size] = pkg.to_device(x, dev).reshape(-1)
        ptr.append(base + at * 8)
        at += 2 * (L + 1) * n
    pa, pb, pc = ptr[0:2], ptr[2:4], ptr[4:6]
    out = torch.zeros(batch * 2 * (L - 1) * n + 2, dtype=torch.int64, device=dev)
    lib = pkg.capi.lib()
    nbytes = lib.troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(plan.h, L, batch)
    assert nbytes > lib.troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(plan.h, L, 1, batch)      # ... plus the scalar table
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    good = dict(L=L, a=pa, b=pb, c=pc, c_nmod=c_nmod, alpha=alpha, w=w, k=k, keys=[x.data_ptr() for x in dkeys], out=out.data_ptr(), ws=ws.data_ptr(),
                ws_bytes=nbytes, batch=batch)
    rc, msg = _raw(pkg, plan, **good)
    torch.cuda.synchronize()
    assert rc == 0, msg
    ref = plan.multiply_affine_relinearize_rescale(L, [pkg.to_device(x, dev) for x in a], [pkg.to_device(x, dev) for x in b], [pkg.to_device(x, dev) for x in c],
                                                   c_nmod, alpha, w, dkeys, constant=k)
    assert torch.equal(out[:batch * 2 * (L - 1) * n].reshape(ref.shape), ref)

    def refused(code=-1, named=True, **change):
        rc, msg = _raw(pkg, plan, **dict(good, **change))
        assert rc == code and (not named or "[troyn_ckks_multiply_affine_relinearize_rescale]" in msg), (sorted(change), rc, msg)

    refused(L=1, named=False)                                   # L < 2
    refused(L=4, named=False)                                   # no special prime left for the key switch
    for table in ("a", "b", "c", "c_nmod", "alpha", "w", "keys"):
        refused(**{table: None})                                # a null table
    refused(out=None)
    refused(ws=None)
    refused(a=[pa[0], None])                                    # a null a[i]
    refused(b=[None, pb[1]])                                    # a null b[i]
    refused(a=[pa[0], pa[1] + 8])                               # a misaligned pointer: operand, addend, destination, workspace
    refused(c=[pc[0] + 8, pc[1]])
    refused(out=out.data_ptr() + 8)
    refused(ws=ws.data_ptr() + 8)
    refused(c_nmod=[L + 1, L - 1])                              # c_nmod[i] < L
    for name, tab in (("alpha", alpha), ("w", w), ("k", k)):   # a scalar word >= its modulus
        badt = [list(r) for r in tab]
        badt[1][2] = q[2]
        refused(**{name: badt})
    refused(out=pa[1])                                          # out overlapping an input
    refused(out=pc[0] + (2 * (L + 1) * n - 2) * 8)              # ... an addend, by its last words only
    refused(out=ws.data_ptr() + 64)                             # out overlapping the workspace
    refused(code=-3, ws_bytes=nbytes - 1)                       # TROYN_E_WORKSPACE
    # a weight is not looked at where there is no addend
    badw = [list(r) for r in w]
    badw[1][0] = q[0] + 3
    rc, msg = _raw(pkg, plan, **dict(good, c=[pc[0], None], w=badw))
    torch.cuda.synchronize()
    assert rc == 0, msg
    # the size query refuses the levels the entry refuses
    assert lib.troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(plan.h, 1, 1) == 0
    assert lib.troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(plan.h, 4, 1) == 0
    # through Plan: a TroynInvalidArgument
    with pytest.raises(pkg.capi.TroynInvalidArgument):
        plan.multiply_affine_relinearize_rescale(L, [pkg.to_device(a[0], dev)], [pkg.to_device(b[0], dev)], [None], [0], [[q[0], 1, 1]], [[0] * L], dkeys)


def test_batch_zero_with_null_buffers(O, pkg, dev):
    plan, q, dkeys = _setup(O, pkg, dev, 64, "mixed", 3)
    rc, msg = _raw(pkg, plan, 3, None, None, None, None, None, None, None, None, None, None, 0, 0)
    assert rc == 0, msg
    assert plan.multiply_affine_relinearize_rescale(3, [], [], [], [], [], [], dkeys) is None
    rc, _ = _raw(pkg, plan, 1, None, None, None, None, None, None, None, None, None, None, 0, 0)
    assert rc == -1      # the level is still checked
