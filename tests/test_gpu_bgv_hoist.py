"""The hoisted BGV entries on the GPU (troyn_bgv_apply_galois_many / _sum / _weighted_sums / _sum_each, troyn_bgv_linear_transform_bsgs,
through engine.Bgv) against the exact big-integer specification of tests/bgv_hoist_spec.py, word for word -- never against another GPU
path, except where the contract itself is an equality between entries.

Small rings (N = 32 / 64): everything by definition.  N = 1024 / 8192: the specification's negacyclic products and exact division on Python
integers; only the NTT <-> coefficient form conversions of operands use the oracle's transform (as tests/test_gpu_hoist.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bgv_hoist_spec as S
from hoist_spec import inner_products
from test_keyswitch_spec import _ntt_polys

pytestmark = pytest.mark.gpu

# (N, bit sizes, t): t = 2 is the plain modulus whose inverse of the special prime is 1 (no multiply in the kernel)
SHAPES = [(32, (30, 30, 30), 257), (64, (30, 30, 30), 2), (64, (60, 40, 40, 60), 65537)]
POOL = lambda n: [5, 25, 2 * n - 1, 3]
ITEMS = 5


def _ints(a):
    return [[int(v) for v in row] for row in a]


@functools.lru_cache(maxsize=None)
def _case(O, n, bits, L):
    """five different items, one key set per pool element, six weights; shared by every test of this chain and level"""
    q = [int(v) for v in O.coeff_modulus_create(n, list(bits))]
    K = len(q)
    rng = np.random.default_rng(n + 7 * L + K)
    poly = lambda m: rng.integers(0, m, size=n, dtype=np.uint64)
    items = [(np.stack([poly(q[l]) for l in range(L)]), np.stack([poly(q[l]) for l in range(L)])) for _ in range(ITEMS)]
    keys_c = [[np.stack([np.stack([poly(q[k]) for k in range(K)]) for c in range(2)]) for j in range(L)] for _ in range(4)]
    keys_l = [[[_ints(kj[c]) for c in range(2)] for kj in kt] for kt in keys_c]
    weights = [np.stack([poly(q[k]) for k in range(K)]) for _ in range(6)]
    return q, items, keys_c, keys_l, weights


@functools.lru_cache(maxsize=None)
def _inner(O, n, bits, L, b):
    """hoist_spec.inner_products of item b with the four pool keys"""
    q, items, _, keys_l, _ = _case(O, n, bits, L)
    return inner_products(q, L, _ints(items[b][1]), POOL(n), keys_l)


class _Dev:
    """the device side of one case: plan, key-level handle, keys and weights in NTT form"""

    def __init__(self, O, pkg, dev, n, bits, t, L):
        self.q, self.items, keys_c, self.keys_l, weights = _case(O, n, bits, L)
        self.n, self.L, self.t, self.pkg, self.dev = n, L, t, pkg, dev
        q = self.q
        self.plan = pkg.Plan(dev, n.bit_length() - 1, q)
        self.bgv = pkg.Bgv(self.plan, len(q), t)
        self.keys = [[pkg.to_device(np.stack([_ntt_polys(kj[c], q) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
        self.weights_l = [_ints(w) for w in weights]
        self.weights = [pkg.to_device(_ntt_polys(w, q), dev) for w in weights]

    def form(self, x):
        """[2][L][N] coefficient form -> NTT form"""
        return np.stack([_ntt_polys(np.array(x[c], dtype=np.uint64), self.q[:self.L]) for c in range(2)])

    def ct(self, batch):
        return self.pkg.to_device(np.stack([self.form(np.stack(it)) for it in self.items[:batch]]), self.dev)


def _levels(bits):
    return sorted({len(bits) - 1, 1})


CASES = [(n, bits, t, L, batch) for n, bits, t in SHAPES for L in _levels(bits) for batch in (1, 3, 5)]


@pytest.mark.parametrize("n,bits,t,L,batch", CASES)
def test_many_and_sum_by_definition(O, pkg, dev, n, bits, t, L, batch):
    """terms = 1 and terms = 3 with a duplicate element; batches 1, 3 and 5 reach the bodies of one, two and four items with a remainder"""
    d = _Dev(O, pkg, dev, n, bits, t, L)
    ct = d.ct(batch)
    for sel in ([3], [0, 2, 0]):
        elements = [POOL(n)[i] for i in sel]
        keys = [d.keys[i] for i in sel]
        many = pkg.to_host(d.bgv.apply_galois_many(L, ct, elements, keys))
        summed = pkg.to_host(d.bgv.apply_galois_sum(L, ct, elements, keys))
        assert many.shape == (len(sel), batch, 2, L, n) and summed.shape == (batch, 2, L, n)
        for b in range(batch):
            P = _inner(O, n, bits, L, b)
            c0 = _ints(d.items[b][0])
            for u, i in enumerate(sel):
                assert np.array_equal(many[u, b], d.form(S.finish(d.q, L, t, c0, POOL(n), P, [i]))), ("many", sel, b, u)
            assert np.array_equal(summed[b], d.form(S.finish(d.q, L, t, c0, POOL(n), P, sel))), ("sum", sel, b)


def _keyed(O, n, bits, L, b, sel):
    """keyed_inner_products' shape for the terms drawn from the pool by `sel` (None = the identity)"""
    P = _inner(O, n, bits, L, b)
    return [None if i is None else P[i] for i in sel]


@pytest.mark.parametrize("n,bits,t,L,batch", CASES)
def test_weighted_sums_by_definition(O, pkg, dev, n, bits, t, L, batch):
    """three slots over {5, identity, 2N-1, 5}: a NULL weight in every slot, an identity term, a slot with the identity alone"""
    d = _Dev(O, pkg, dev, n, bits, t, L)
    sel = [0, None, 2, 0]
    elements = [1 if i is None else POOL(n)[i] for i in sel]
    keys = [None if i is None else d.keys[i] for i in sel]
    w = [[0, 1, 2, None], [None, 3, None, 4], [None, 5, None, None]]
    got = pkg.to_host(d.bgv.apply_galois_weighted_sums(L, d.ct(batch), elements, keys, [[None if i is None else d.weights[i] for i in row] for row in w]))
    assert got.shape == (3, batch, 2, L, n)
    for b in range(batch):
        P = _keyed(O, n, bits, L, b, sel)
        c0, c1 = _ints(d.items[b][0]), _ints(d.items[b][1])
        for s, row in enumerate(w):
            want = S.finish_weighted(d.q, L, t, c0, c1, elements, P, [None if i is None else d.weights_l[i] for i in row], "post")
            assert np.array_equal(got[s, b], d.form(want)), (s, b)


@pytest.mark.parametrize("n,bits,t,L,batch", CASES)
def test_sum_each_by_definition(O, pkg, dev, n, bits, t, L, batch):
    """9 terms, one more than TROYN_HOIST_EACH_GROUP, with an identity term inside the first group; term u of item b is item (u + b) mod 5"""
    d = _Dev(O, pkg, dev, n, bits, t, L)
    sel = [0, 1, None, 2, 3, 0, 1, 2, 3]
    elements = [1 if i is None else POOL(n)[i] for i in sel]
    keys = [None if i is None else d.keys[i] for i in sel]
    src = lambda u, b: (u + b) % ITEMS
    cts = pkg.to_device(np.stack([np.stack([d.form(np.stack(d.items[src(u, b)])) for b in range(batch)]) for u in range(len(sel))]), dev)
    got = pkg.to_host(d.bgv.apply_galois_sum_each(L, cts, elements, keys))
    assert got.shape == (batch, 2, L, n)
    for b in range(batch):
        P = [None if i is None else _inner(O, n, bits, L, src(u, b))[i] for u, i in enumerate(sel)]
        each = [(_ints(d.items[src(u, b)][0]), _ints(d.items[src(u, b)][1])) for u in range(len(sel))]
        assert np.array_equal(got[b], d.form(S.sum_each_spec(d.q, L, t, each, elements, None, "post", P=P))), b


@pytest.mark.parametrize("n,bits,t,L,batch", CASES)
def test_bsgs_by_definition(O, pkg, dev, n, bits, t, L, batch):
    """2 giants x 2 babies with an identity baby, an identity giant and one absent weight; and the contract's equality on the device"""
    d = _Dev(O, pkg, dev, n, bits, t, L)
    babies, bsel = [1, POOL(n)[0]], [None, 0]
    giants, gsel = [POOL(n)[2], 1], [2, None]
    bkeys = [None if i is None else d.keys[i] for i in bsel]
    gkeys = [None if i is None else d.keys[i] for i in gsel]
    w = [[0, 1], [None, 2]]
    dw = [[None if i is None else d.weights[i] for i in row] for row in w]
    lw = [[None if i is None else d.weights_l[i] for i in row] for row in w]
    ct = d.ct(batch)
    got = pkg.to_host(d.bgv.linear_transform_bsgs(L, ct, babies, bkeys, giants, gkeys, dw))
    inner = d.bgv.apply_galois_weighted_sums(L, ct, babies, bkeys, dw)
    assert np.array_equal(got, pkg.to_host(d.bgv.apply_galois_sum_each(L, inner, giants, gkeys)))
    for b in range(batch):
        c0, c1 = _ints(d.items[b][0]), _ints(d.items[b][1])
        want = S.bsgs_spec(d.q, L, t, c0, c1, babies, [None if i is None else d.keys_l[i] for i in bsel],
                           giants, [None if i is None else d.keys_l[i] for i in gsel], lw, "post")
        assert np.array_equal(got[b], d.form(want)), b


def test_special_row_edges(O, pkg, dev):
    """the special row in coefficient form holds the edges of the mod-t correction: 0, 1, t-1, t, t+1, qk-1, qk-t, multiples of t around qk/2.
    Digit 0 of the item is the constant 1 (fixed by every automorphism), so the special row of the key (term 0, digit 0) sets it."""
    n, bits, t, L = 64, (60, 40, 40, 60), 65537, 3
    q = [int(v) for v in O.coeff_modulus_create(n, list(bits))]
    K, qk = len(q), q[-1]
    rng = np.random.default_rng(5)
    poly = lambda m: rng.integers(0, m, size=n, dtype=np.uint64)
    c0, c1 = np.stack([poly(q[l]) for l in range(L)]), np.stack([poly(q[l]) for l in range(L)])
    c1[0] = 0
    c1[0, 0] = 1
    elements = [5, 2 * n - 1]
    keys_c = [[np.stack([np.stack([poly(q[k]) for k in range(K)]) for c in range(2)]) for j in range(L)] for _ in elements]
    for c in range(2):
        keys_c[0][0][c][K - 1][:] = 0
    keys_l = lambda: [[[_ints(kj[c]) for c in range(2)] for kj in kt] for kt in keys_c]
    P = inner_products(q, L, _ints(c1), elements, keys_l())
    half = (qk // 2) // t * t
    edge = [0, 1, t - 1, t, t + 1, qk - 1, qk - t, qk - t - 1, half, half - 1, half + 1, half + t, 2 * t - 1, qk - 2]
    for c in range(2):
        want = [int(v) for v in poly(qk)]
        want[:len(edge)] = edge if c == 0 else edge[::-1]
        rest = [(x + y) % qk for x, y in zip(P[0][c][K - 1], P[1][c][K - 1])]
        keys_c[0][0][c][K - 1][:] = np.array([(x - y) % qk for x, y in zip(want, rest)], dtype=np.uint64)
    P = inner_products(q, L, _ints(c1), elements, keys_l())
    assert [(x + y) % qk for x, y in zip(P[0][0][K - 1], P[1][0][K - 1])][:len(edge)] == edge
    plan = pkg.Plan(dev, 6, q)
    bgv = pkg.Bgv(plan, K, t)
    form = lambda x: np.stack([_ntt_polys(np.array(x[c], dtype=np.uint64), q[:L]) for c in range(2)])
    dkeys = [[pkg.to_device(np.stack([_ntt_polys(kj[c], q) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    ct = pkg.to_device(form(np.stack([c0, c1]))[None], dev)
    summed = pkg.to_host(bgv.apply_galois_sum(L, ct, elements, dkeys))
    assert np.array_equal(summed[0], form(S.finish(q, L, t, _ints(c0), elements, P, range(2))))


@pytest.mark.parametrize("n,bits,t,L", [(1024, [50, 50, 50, 50], 1 << 20, 3), (8192, [60, 40, 40, 60], 65537, 3)])
@pytest.mark.parametrize("batch", [1, 3])
def test_kernel_sizes_against_spec(O, pkg, dev, n, bits, t, L, batch):
    """the optimised transforms' sizes: many and sum against the specification, the weighted entry with unit weights against sum, and
    bsgs against weighted_sums followed by sum_each, word for word"""
    q = [int(v) for v in O.coeff_modulus_create(n, bits)]
    K = len(q)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    bgv = pkg.Bgv(plan, K, t)
    rng = np.random.default_rng(78 + batch)
    elements = [5, 2 * n - 1]
    poly = lambda m: rng.integers(0, m, size=n, dtype=np.uint64)
    items = [(np.stack([poly(q[l]) for l in range(L)]), np.stack([poly(q[l]) for l in range(L)])) for _ in range(batch)]
    keys_c = [[np.stack([np.stack([poly(q[k]) for k in range(K)]) for c in range(2)]) for j in range(L)] for _ in elements]
    keys_l = [[[_ints(kj[c]) for c in range(2)] for kj in kt] for kt in keys_c]

    def to_ntt_rows(x, rows):        # x [len(rows)][N] under moduli q[rows]; the oracle's transform, conversions only
        out = np.empty_like(x)
        for i, r in enumerate(rows):
            c1x = O.Context("ckks", n, [q[r], q[(r + 1) % K]])
            out[i] = c1x.to_ntt(x[i][None, None], 1, 1)[0, 0]
        return out

    form = lambda x: np.stack([to_ntt_rows(np.array(x[c], dtype=np.uint64), list(range(L))) for c in range(2)])
    dkeys = [[pkg.to_device(np.stack([to_ntt_rows(kj[c], list(range(K))) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    ct = pkg.to_device(np.stack([form(np.stack(it)) for it in items]), dev)
    many = pkg.to_host(bgv.apply_galois_many(L, ct, elements, dkeys))
    summed = pkg.to_host(bgv.apply_galois_sum(L, ct, elements, dkeys))
    for b in sorted({0, batch - 1}):
        P = inner_products(q, L, _ints(items[b][1]), elements, keys_l)
        c0 = _ints(items[b][0])
        for u in range(2):
            assert np.array_equal(many[u, b], form(S.finish(q, L, t, c0, elements, P, [u]))), ("many", u, b)
        assert np.array_equal(summed[b], form(S.finish(q, L, t, c0, elements, P, range(2)))), ("sum", b)
    # unit weights (the transform of the constant 1 is 1 at every point): the weighted entry's words are the summed form's
    one = pkg.to_device(np.ones((K, n), dtype=np.uint64), dev)
    assert np.array_equal(pkg.to_host(bgv.apply_galois_weighted_sums(L, ct, elements, dkeys, [[one, one]]))[0], summed)
    # bsgs = weighted_sums then sum_each, on random weights with an identity baby and an absent weight
    w = [pkg.to_device(np.stack([poly(q[k]) for k in range(K)]), dev) for _ in range(3)]
    babies, bkeys, giants, gkeys = [1, 5], [None, dkeys[0]], [2 * n - 1, 5], [dkeys[1], dkeys[0]]
    weights = [[w[0], w[1]], [None, w[2]]]
    inner = bgv.apply_galois_weighted_sums(L, ct, babies, bkeys, weights)
    assert np.array_equal(pkg.to_host(bgv.linear_transform_bsgs(L, ct, babies, bkeys, giants, gkeys, weights)),
                          pkg.to_host(bgv.apply_galois_sum_each(L, inner, giants, gkeys)))


def test_refusals_and_the_empty_batch(O, pkg, dev):
    import torch
    n, L, t = 32, 2, 257
    q = [int(v) for v in O.coeff_modulus_create(n, [30, 30, 30])]
    K = len(q)
    plan = pkg.Plan(dev, 5, q)
    lib = pkg.capi.lib()
    ctx = O.Context("ckks", n, q)
    bgv = pkg.Bgv(plan, K, t)
    ct = pkg.to_device(ctx.random_ct(1, 2, L)[None], dev)
    key = [pkg.to_device(k, dev) for k in ctx.random_keys(2, L)]
    one = pkg.to_device(np.ones((K, n), dtype=np.uint64), dev)
    INVALID = pkg.capi.TroynInvalidArgument
    calls = {
        "many": lambda h, L_, ct_, el, ks, **kw: h.apply_galois_many(L_, ct_, el, ks, **kw),
        "sum": lambda h, L_, ct_, el, ks, **kw: h.apply_galois_sum(L_, ct_, el, ks, **kw),
        "weighted": lambda h, L_, ct_, el, ks, **kw: h.apply_galois_weighted_sums(L_, ct_, el, ks, [[one] * len(el)], **kw),
        "each": lambda h, L_, ct_, el, ks, **kw: h.apply_galois_sum_each(L_, ct_.repeat(*([len(el) or 1] + [1] * (ct_.dim() - 1))), el, ks, **kw),
        "bsgs": lambda h, L_, ct_, el, ks, **kw: h.linear_transform_bsgs(L_, ct_, el, ks, el, ks, [[one] * len(el)] * len(el), **kw),
    }
    for name, fn in calls.items():
        # the handle first: not the key level; no inverse of the special prime mod t (t = the special prime itself)
        with pytest.raises(INVALID, match="BGV key switching needs the key level's constants"):
            fn(pkg.Bgv(plan, L, t), L, ct, [3], [key])
        with pytest.raises(INVALID, match="Unable to invert"):
            fn(pkg.Bgv(plan, K, q[-1]), L, ct, [3], [key])
        with pytest.raises(INVALID):
            fn(bgv, L, ct, [], [])                                  # terms == 0
        identity_ok = name not in ("many", "sum")
        for bad in (4, 2 * n, 2 * n + 1) + (() if identity_ok else (1,)):      # even, >= 2N, the identity where the namesake refuses it
            with pytest.raises(INVALID):
                fn(bgv, L, ct, [3, bad], [key, key])
        with pytest.raises(INVALID):
            fn(bgv, L, ct, [3], [[key[0], None]])                   # a null key entry
        with pytest.raises(INVALID):
            fn(bgv, 3, pkg.to_device(np.zeros((1, 2, 3, n), dtype=np.uint64), dev), [3], [key + key])      # L = K
        if name != "each":
            with pytest.raises(INVALID):
                fn(bgv, L, ct, [3], [key], out=ct)                  # out overlapping ct
        assert fn(bgv, L, ct[:0], [3], [key]).numel() == 0          # batch == 0: TROYN_OK, nothing launched
    with pytest.raises(INVALID):
        bgv.apply_galois_weighted_sums(L, ct, [3], [key], [[None]])     # a slot with no weight
    # the raw entries: a null handle, null tables, L = 0, a short workspace; the workspace is the plan's query with is_ntt_form = 1
    ws = torch.empty(max(lib.troyn_apply_galois_hoisted_workspace_bytes(plan.h, L, 1, 1, 0), lib.troyn_apply_galois_sum_each_workspace_bytes(plan.h, L, 1, 1, 1)),
                     dtype=torch.uint8, device=dev)
    out = torch.empty_like(ct)
    el = (C.c_uint64 * 1)(3)
    kp = (C.c_void_p * L)(*[k.data_ptr() for k in key])
    args = lambda h=bgv.h, L_=L, ct_=ct.data_ptr(), el_=el, kp_=kp, out_=out.data_ptr(), wsb=None: (
        h, L_, C.c_void_p(ct_), el_, kp_, 1, C.c_void_p(out_), C.c_void_p(ws.data_ptr()), ws.numel() if wsb is None else wsb, 1, None)
    for fn in (lib.troyn_bgv_apply_galois_many, lib.troyn_bgv_apply_galois_sum, lib.troyn_bgv_apply_galois_sum_each):
        assert fn(*args()) == 0
        assert fn(*args(h=None)) == -1
        assert fn(*args(L_=0)) == -1
        assert fn(*args(el_=None)) == -1
        assert fn(*args(kp_=None)) == -1
        assert fn(*args(ct_=None)) == -1
        assert fn(*args(out_=None)) == -1
        assert fn(*args(out_=ct.data_ptr() + 16)) == -1
        assert fn(*args(wsb=8)) == -3
    torch.cuda.synchronize()
    no_inverse = pkg.Bgv(plan, K, q[-1])
    assert lib.troyn_bgv_apply_galois_sum(*args(h=no_inverse.h)) == -2
    assert b"[RNSTool::RNSTool] Unable to invert q[last] mod t." in lib.troyn_last_error()
