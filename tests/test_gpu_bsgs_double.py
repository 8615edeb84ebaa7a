"""The double-hoisted baby-step/giant-step linear transform on the GPU (troyn_linear_transform_bsgs_double_hoisted) against the exact
big-integer specification of tests/bsgs_double_spec.py -- word for word, never against another GPU path.

Small rings (N = 32 / 64): everything by definition.  N = 1024 / 8192: the specification's negacyclic products and exact rounded divisions on
Python integers; only the NTT <-> coefficient form conversions of operands use the oracle's transform, which tests/test_keyswitch_spec.py pins
to the by-definition transform (as tests/test_gpu_hoist.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bsgs_double_spec import bsgs_double_spec, divide, inner_values, outer_sum
from test_gpu_hoist import EDGE, _ints, _small_case
from test_gpu_sum_each import _random_ct, _small_forms, _small_keys
from test_gpu_weighted_hoist import _keys_as_lists, _random_weight
from test_keyswitch_spec import _ntt_polys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = int(re.search(r"^#define TROYN_HOIST_EACH_GROUP (\d+)$", open(os.path.join(ROOT, "include", "troyn.h")).read(), flags=re.M).group(1))


def _device_weights(pkg, dev, q, weights):
    return [[None if x is None else pkg.to_device(_ntt_polys(np.array(x, dtype=np.uint64), q), dev) for x in row] for row in weights]


@pytest.mark.parametrize("n,bits,L,order", [(32, (50, 50, 50, 50), 3, None), (64, (60, 40, 40, 60), 3, None), (32, (50, 50, 50), 2, "reversed")])
@pytest.mark.parametrize("scheme,is_ntt", [("ckks", True), ("bfv", False)])
def test_small_rings_by_definition(O, pkg, dev, n, bits, L, order, scheme, is_ntt):
    """babies {1, 5, 25}, giants {1, 125 mod 2N, 2N - 1}, absent weights, two different items whose digit 0 is the constant 1 (fixed by every
    automorphism), the construction of test_gpu_hoist._solve_boundary twice:
      item 0: the special row of baby key (5, digit 0, component 1) is solved so that the INNER X_1[q_special] of the giant step 125 sits on the
              rounding boundaries h - 1, h, h + 1, 0, 1, q_special - 1, ... at the first coefficients (baby 5 has the constant 1 as its
              special-row weight there);
      item 1: baby 25 is present in the identity giant step alone, with the constant 1 on the special row, so the special rows of its key
              (digit 0, both components) move the FINAL Y_c[q_special] and nothing else: solved so that Y_c[q_special] sits on the boundaries."""
    q, _, _, all_keys, _ = _small_case(O, n, bits, L, order)      # keys of {5, 25, 2N - 1, 3}
    K = len(q)
    qs, h = q[-1], q[-1] // 2
    rng = np.random.default_rng(7 * n + L)
    keys_c = [[kj.copy() for kj in kt] for kt in all_keys]
    babies, baby_keys = [1, 5, 25], [None, keys_c[0], keys_c[1]]
    giants, giant_keys = [1, 125 % (2 * n), 2 * n - 1], [None, keys_c[3], keys_c[2]]      # (any key buffer serves the words of 5^3)
    w = lambda unit=False: _random_weight(q, n, rng, unit_special=unit)
    weights = [[w(), None, w(True)], [w(), w(True), None], [None, w(), None]]
    items = [_random_ct(q, L, n, rng, unit_digit=True) for _ in range(2)]
    edge = EDGE(qs, h)
    spec_args = lambda: (babies, _keys_as_lists(baby_keys))
    baby_keys[1][0][1][K - 1][:] = 0
    for c in range(2):
        baby_keys[2][0][c][K - 1][:] = 0
    # item 0: the inner special row of component 1 of giant step 1
    X = inner_values(q, L, _ints(items[0][0]), _ints(items[0][1]), *spec_args(), weights)
    target = [int(v) for v in rng.integers(0, qs, size=n, dtype=np.uint64)]
    target[:len(edge)] = edge
    baby_keys[1][0][1][K - 1][:] = np.array([(a - b) % qs for a, b in zip(target, X[1][1][K - 1])], dtype=np.uint64)
    # item 1: the final special rows
    X = inner_values(q, L, _ints(items[1][0]), _ints(items[1][1]), *spec_args(), weights)
    Y, _ = outer_sum(q, L, X, giants, _keys_as_lists(giant_keys))
    for c in range(2):
        target = [int(v) for v in rng.integers(0, qs, size=n, dtype=np.uint64)]
        target[:len(edge)] = edge if c == 0 else edge[::-1]
        baby_keys[2][0][c][K - 1][:] = np.array([(a - b) % qs for a, b in zip(target, Y[c][K - 1])], dtype=np.uint64)
    # the solved keys put the rows where they were aimed
    bl, gl = _keys_as_lists(baby_keys), _keys_as_lists(giant_keys)
    X0 = inner_values(q, L, _ints(items[0][0]), _ints(items[0][1]), babies, bl, weights)
    assert X0[1][1][K - 1][:len(edge)] == edge
    X1 = inner_values(q, L, _ints(items[1][0]), _ints(items[1][1]), babies, bl, weights)
    Y1, _ = outer_sum(q, L, X1, giants, gl)
    assert Y1[0][K - 1][:len(edge)] == edge and Y1[1][K - 1][:len(edge)] == edge[::-1]
    want = []
    for Xi in (X0, X1):
        Yi, _ = outer_sum(q, L, Xi, giants, gl)
        want.append([divide(q, L, Yi[c]) for c in range(2)])
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    form = _small_forms(q, L, is_ntt)
    ct = pkg.to_device(np.stack([form(np.stack(it)) for it in items]), dev)
    got = pkg.to_host(plan.linear_transform_bsgs_double_hoisted(L, ct, babies, _small_keys(pkg, dev, q, baby_keys), giants,
                                                                _small_keys(pkg, dev, q, giant_keys), _device_weights(pkg, dev, q, weights),
                                                                is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    assert got.shape == (2, 2, L, n)
    for b in range(2):
        assert np.array_equal(got[b], form(want[b])), b


@pytest.mark.parametrize("scheme,is_ntt", [("ckks", True), ("bfv", False)])
@pytest.mark.parametrize("giants", [[1], [3, 1] + list(range(5, 5 + 2 * (GROUP - 1), 2))])
def test_one_identity_giant_and_a_second_group(O, pkg, dev, scheme, is_ntt, giants):
    """N = 32: giants = 1 with G = 1 (no inner division at all), and TROYN_HOIST_EACH_GROUP + 1 giant steps with an identity step in the first
    group (two runs of keyed steps, the last step alone in a second group that adds into the sum)"""
    n, L = 32, 3
    q, _, _, all_keys, _ = _small_case(O, n, (50, 50, 50, 50), L, None)
    assert len(giants) in (1, GROUP + 1)
    rng = np.random.default_rng(len(giants))
    babies, baby_keys = [1, 5, 25], [None, all_keys[0], all_keys[1]]
    giant_keys = [None if G == 1 else all_keys[2 + i % 2] for i, G in enumerate(giants)]
    weights = [[_random_weight(q, n, rng), None if g % 2 else _random_weight(q, n, rng), _random_weight(q, n, rng)] for g in range(len(giants))]
    items = [_random_ct(q, L, n, rng) for _ in range(2)]
    plan = pkg.Plan(dev, 5, q)
    form = _small_forms(q, L, is_ntt)
    ct = pkg.to_device(np.stack([form(np.stack(it)) for it in items]), dev)
    got = pkg.to_host(plan.linear_transform_bsgs_double_hoisted(L, ct, babies, _small_keys(pkg, dev, q, baby_keys), giants,
                                                                _small_keys(pkg, dev, q, giant_keys), _device_weights(pkg, dev, q, weights),
                                                                is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    for b, (c0, c1) in enumerate(items):
        want = bsgs_double_spec(q, L, _ints(c0), _ints(c1), babies, _keys_as_lists(baby_keys), giants, _keys_as_lists(giant_keys), weights)
        assert np.array_equal(got[b], form(want)), b


@pytest.mark.parametrize("n,bits,L,is_ntt", [(1024, [50, 50, 50], 2, True),
                                             (8192, [60, 40, 40, 60], 3, True),
                                             (8192, [40, 40, 40], 2, False)])
def test_kernel_sizes_against_spec(O, pkg, dev, n, bits, L, is_ntt):
    """babies {identity, 5}, giants {identity, 2N - 1}, batch = 8 identical items (groups of four items per workgroup, two groups)"""
    q = [int(v) for v in O.coeff_modulus_create(n, bits)]
    K = len(q)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    rng = np.random.default_rng(91 + L)
    babies, giants = [1, 5], [1, 2 * n - 1]
    c0, c1 = _random_ct(q, L, n, rng)
    key = lambda: [np.stack([np.stack([rng.integers(0, q[k], size=n, dtype=np.uint64) for k in range(K)]) for c in range(2)]) for j in range(L)]
    baby_keys, giant_keys = [None, key()], [None, key()]
    weights = [[_random_weight(q, n, rng), _random_weight(q, n, rng)], [None, _random_weight(q, n, rng)]]

    def to_ntt_rows(x, rows):        # x [len(rows)][N] under moduli q[rows]; the oracle's transform, conversions only
        out = np.empty_like(x)
        for i, r in enumerate(rows):
            c1x = O.Context("ckks", n, [q[r], q[(r + 1) % K]])
            out[i] = c1x.to_ntt(x[i][None, None], 1, 1)[0, 0]
        return out

    every = list(range(K))
    form = (lambda x: np.stack([to_ntt_rows(np.array(x[c], dtype=np.uint64), list(range(L))) for c in range(2)])) if is_ntt else (lambda x: np.array(x, dtype=np.uint64))
    dkeys = lambda ks: [None if kt is None else [pkg.to_device(np.stack([to_ntt_rows(kj[c], every) for c in range(2)]), dev) for kj in kt] for kt in ks]
    dweights = [[None if x is None else pkg.to_device(to_ntt_rows(np.array(x, dtype=np.uint64), every), dev) for x in row] for row in weights]
    batch = 8
    ct = pkg.to_device(np.repeat(form(np.stack([c0, c1]))[None], batch, axis=0), dev)
    got = pkg.to_host(plan.linear_transform_bsgs_double_hoisted(L, ct, babies, dkeys(baby_keys), giants, dkeys(giant_keys), dweights,
                                                                is_ckks=is_ntt, is_ntt_form=is_ntt))
    assert got.shape == (batch, 2, L, n)
    want = form(bsgs_double_spec(q, L, _ints(c0), _ints(c1), babies, _keys_as_lists(baby_keys), giants, _keys_as_lists(giant_keys), weights))
    for i in (0, 3, 7):
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
    fn = plan.linear_transform_bsgs_double_hoisted
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
    with pytest.raises(INVALID, match="troyn_linear_transform_bsgs_double_hoisted"):
        fn(L, ct, [1, 3], [None, key], [1, 5], [None, [key[0], None]], [[w, w], [w, w]])   # a null entry of a keyed giant step
    assert fn(L, ct[:0], [1, 3], [None, key], [1, 5], [None, key], [[w, w], [w, w]]).numel() == 0      # batch == 0
    # the raw entry: a short workspace, and the same refusals without the binding's own checks
    wb = lib.troyn_linear_transform_bsgs_double_hoisted_workspace_bytes
    ws = torch.empty(wb(plan.h, L, 2, 2, 1, 1), dtype=torch.uint8, device=dev)
    out = torch.empty_like(ct)
    bel, gel = (C.c_uint64 * 2)(1, 3), (C.c_uint64 * 2)(1, 5)
    kp = (C.c_void_p * (2 * L))(*([None] * L + [k.data_ptr() for k in key]))
    full = (C.c_void_p * 4)(w.data_ptr(), w.data_ptr(), w.data_ptr(), None)
    raw = lib.troyn_linear_transform_bsgs_double_hoisted
    args = lambda wp_=full, babies=2, giants=2, wsb=None, out_=out.data_ptr(), L_=L, ct_=ct.data_ptr(), batch=1: (
        plan.h, L_, 1, 1, C.c_void_p(ct_), bel, kp, babies, gel, kp, giants, wp_, C.c_void_p(out_), C.c_void_p(ws.data_ptr()),
        ws.numel() if wsb is None else wsb, batch, None)
    assert raw(*args()) == 0
    assert raw(*args(wp_=(C.c_void_p * 4)(w.data_ptr(), None, None, None))) == -1
    assert raw(*args(wp_=(C.c_void_p * 4)(w.data_ptr() + 8, None, w.data_ptr(), None))) == -1
    assert raw(*args(wp_=None)) == -1
    assert raw(*args(babies=0)) == -1
    assert raw(*args(giants=0)) == -1
    assert raw(*args(L_=0)) == -1
    assert raw(*args(L_=K)) == -1
    assert raw(*args(ct_=None)) == -1
    assert raw(*args(out_=None)) == -1
    assert raw(*args(out_=ct.data_ptr())) == -1
    assert raw(*args(out_=ct.data_ptr() + 16)) == -1
    assert raw(*args(wsb=ws.numel() - 1)) == -3                                          # one byte short
    assert raw(*args(wsb=0, batch=0, ct_=None, out_=None)) == 0                          # batch == 0 looks at nothing
    torch.cuda.synchronize()
    # past one group only the inner results grow with `giants`, [batch][2][L+1][N] words per giant step, and the inner stage's table by at most
    # one weight pointer per baby and giant step (the table region also holds one group's hoisted tables, so it may not grow at all)
    batch, babies = 3, 2
    grow = wb(plan.h, L, babies, GROUP + 3, batch, 1) - wb(plan.h, L, babies, GROUP + 1, batch, 1)
    inner = 8 * 2 * batch * 2 * (L + 1) * n
    assert inner <= grow <= inner + 8 * 2 * babies
