"""The baby-step/giant-step linear transform on the GPU (troyn_linear_transform_bsgs) against the exact big-integer specification of
tests/bsgs_spec.py -- never against another GPU path.  Conversions between NTT and coefficient form as in tests/test_gpu_sum_each.py."""
import ctypes as C

import numpy as np
import pytest

from bsgs_spec import bsgs_spec
from test_gpu_hoist import _ints, _small_case
from test_gpu_sum_each import _random_ct, _small_forms, _small_keys
from test_gpu_weighted_hoist import _keys_as_lists, _random_weight
from test_keyswitch_spec import _ntt_polys

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,bits,L", [(32, (50, 50, 50, 50), 3), (64, (60, 40, 40, 60), 3)])
@pytest.mark.parametrize("scheme,is_ntt", [("ckks", True), ("bfv", False)])
def test_small_rings_by_definition(O, pkg, dev, n, bits, L, scheme, is_ntt):
    """babies {1, 5, 25}, giants {1, 125, 2N - 1} (125 = 5^3 reduced modulo 2N: an element is below 2N, so 61 at N = 32), one weight absent, one
    giant step with a single weight, two different items"""
    q, all_elements, _, all_keys, _ = _small_case(O, n, bits, L, None)      # keys of {5, 25, 2N - 1, 3}
    babies, baby_keys = [1, 5, 25], [None, all_keys[0], all_keys[1]]
    giants, giant_keys = [1, 125 % (2 * n), 2 * n - 1], [None, all_keys[3], all_keys[2]]      # (any key buffer serves the words of 5^3)
    rng = np.random.default_rng(5 * n + L)
    w = lambda: _random_weight(q, n, rng)
    weights = [[w(), w(), w()], [w(), None, w()], [None, w(), None]]
    items = [_random_ct(q, L, n, rng) for _ in range(2)]
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    form = _small_forms(q, L, is_ntt)
    dweights = [[None if x is None else pkg.to_device(_ntt_polys(np.array(x, dtype=np.uint64), q), dev) for x in row] for row in weights]
    ct = pkg.to_device(np.stack([form(np.stack(it)) for it in items]), dev)
    got = pkg.to_host(plan.linear_transform_bsgs(L, ct, babies, _small_keys(pkg, dev, q, baby_keys), giants, _small_keys(pkg, dev, q, giant_keys),
                                                 dweights, is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    assert got.shape == (2, 2, L, n)
    for b, (c0, c1) in enumerate(items):
        want = bsgs_spec(q, L, _ints(c0), _ints(c1), babies, _keys_as_lists(baby_keys), giants, _keys_as_lists(giant_keys), weights)
        assert np.array_equal(got[b], form(want)), b


def test_kernel_size_against_spec(O, pkg, dev):
    """N = 8192 {60,40,40,60}, L = 3, CKKS: babies {identity, 5}, giants {identity, 2N - 1}, batch 3 (a group of two items and a padded one)"""
    n, L, is_ntt = 8192, 3, True
    q = [int(v) for v in O.coeff_modulus_create(n, [60, 40, 40, 60])]
    K = len(q)
    plan = pkg.Plan(dev, 13, q)
    rng = np.random.default_rng(87)
    babies, giants = [1, 5], [1, 2 * n - 1]
    c0, c1 = _random_ct(q, L, n, rng)
    key = lambda: [np.stack([np.stack([rng.integers(0, q[k], size=n, dtype=np.uint64) for k in range(K)]) for c in range(2)]) for j in range(L)]
    baby_keys, giant_keys = [None, key()], [None, key()]
    weights = [[_random_weight(q, n, rng), _random_weight(q, n, rng)], [_random_weight(q, n, rng), None]]

    def to_ntt_rows(x, rows):        # x [len(rows)][N] under moduli q[rows]; the oracle's transform, conversions only
        out = np.empty_like(x)
        for i, r in enumerate(rows):
            c1x = O.Context("ckks", n, [q[r], q[(r + 1) % K]])
            out[i] = c1x.to_ntt(x[i][None, None], 1, 1)[0, 0]
        return out

    every = list(range(K))
    form = lambda x: np.stack([to_ntt_rows(np.array(x[c], dtype=np.uint64), list(range(L))) for c in range(2)])
    dkeys = lambda ks: [None if kt is None else [pkg.to_device(np.stack([to_ntt_rows(kj[c], every) for c in range(2)]), dev) for kj in kt] for kt in ks]
    dweights = [[None if x is None else pkg.to_device(to_ntt_rows(np.array(x, dtype=np.uint64), every), dev) for x in row] for row in weights]
    batch = 3
    ct = pkg.to_device(np.repeat(form(np.stack([c0, c1]))[None], batch, axis=0), dev)
    got = pkg.to_host(plan.linear_transform_bsgs(L, ct, babies, dkeys(baby_keys), giants, dkeys(giant_keys), dweights, is_ckks=True, is_ntt_form=is_ntt))
    assert got.shape == (batch, 2, L, n)
    want = form(bsgs_spec(q, L, _ints(c0), _ints(c1), babies, _keys_as_lists(baby_keys), giants, _keys_as_lists(giant_keys), weights))
    for i in range(batch):
        assert np.array_equal(got[i], want), i


def test_errors(O, pkg, dev):
    import torch
    n, L = 32, 2
    q = O.coeff_modulus_create(n, [40, 40, 40])
    K = len(q)
    plan = pkg.Plan(dev, 5, q)
    lib = pkg.capi.lib()
    ctx = O.Context("ckks", n, q)
    ct = pkg.to_device(ctx.random_ct(1, 2, L)[None], dev)
    key = [pkg.to_device(k, dev) for k in ctx.random_keys(2, L)]
    w = pkg.to_device(np.ones((K, n), dtype=np.uint64), dev)
    INVALID = pkg.capi.TroynInvalidArgument
    fn = plan.linear_transform_bsgs
    with pytest.raises(INVALID):
        fn(L, ct, [1, 3], [None, key], [1, 5], [None, key], [[w, w], [None, None]])      # a giant step with no weight
    with pytest.raises(INVALID):
        fn(L, ct, [1, 3], [None, key], [], [], [])                                         # giants == 0
    with pytest.raises(INVALID):
        fn(L, ct, [], [], [1, 5], [None, key], [[], []])                                   # babies == 0
    with pytest.raises(INVALID):
        fn(L, ct, [1, 4], [None, key], [1, 5], [None, key], [[w, w], [w, w]])            # an even baby element
    with pytest.raises(INVALID):
        fn(L, ct, [1, 3], [None, key], [1, 2 * n + 1], [None, key], [[w, w], [w, w]])    # a giant element >= 2N
    with pytest.raises(INVALID):
        fn(L, ct, [1, 3], [None, key], [1, 5], [None, key], [[w, w], [w, w]], out=ct)    # out overlapping ct
    assert fn(L, ct[:0], [1, 3], [None, key], [1, 5], [None, key], [[w, w], [w, w]]).numel() == 0      # batch == 0
    # the raw entry: a short workspace, and the same refusals without the binding's own checks
    wb = lib.troyn_linear_transform_bsgs_workspace_bytes
    ws = torch.empty(wb(plan.h, L, 2, 2, 1, 1), dtype=torch.uint8, device=dev)
    out = torch.empty_like(ct)
    bel, gel = (C.c_uint64 * 2)(1, 3), (C.c_uint64 * 2)(1, 5)
    kp = (C.c_void_p * (2 * L))(*([None] * L + [k.data_ptr() for k in key]))
    full = (C.c_void_p * 4)(w.data_ptr(), w.data_ptr(), w.data_ptr(), None)
    raw = lib.troyn_linear_transform_bsgs
    args = lambda wp_=full, babies=2, giants=2, wsb=None, out_=out.data_ptr(): (
        plan.h, L, 1, 1, C.c_void_p(ct.data_ptr()), bel, kp, babies, gel, kp, giants, wp_, C.c_void_p(out_), C.c_void_p(ws.data_ptr()),
        ws.numel() if wsb is None else wsb, 1, None)
    assert raw(*args()) == 0
    assert raw(*args(wp_=(C.c_void_p * 4)(w.data_ptr(), None, None, None))) == -1
    assert raw(*args(wp_=(C.c_void_p * 4)(w.data_ptr() + 8, None, w.data_ptr(), None))) == -1
    assert raw(*args(wp_=None)) == -1
    assert raw(*args(babies=0)) == -1
    assert raw(*args(giants=0)) == -1
    assert raw(*args(out_=ct.data_ptr())) == -1
    assert raw(*args(wsb=ws.numel() - 8)) == -3
    torch.cuda.synchronize()
    # the inner results live in the workspace: room for one ciphertext per giant step on top of the larger stage
    each = lib.troyn_apply_galois_sum_each_workspace_bytes(plan.h, L, 2, 1, 1)
    weighted = lib.troyn_apply_galois_weighted_workspace_bytes(plan.h, L, 2, 2, 1, 1)
    assert wb(plan.h, L, 2, 2, 1, 1) == 2 * 2 * L * n * 8 + max(each, weighted)
