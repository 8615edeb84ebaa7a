"""BFV inner product through the C-ABI (engine.Behz.bfv_multiply_accumulate[_relinearize]) against the specification composed from the oracle's
bare tools (tests/bfv_dot_spec.py, the reference's 61-bit auxiliary base): every word equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from bfv_dot_spec import BfvDotSpec

pytestmark = pytest.mark.gpu

OPTION_NAMES = ("TROYN_BEHZ", "TROYN_BEHZ_BASE", "TROYN_BFV_TENSOR", "TROYN_BEHZ_LIFT")
CAP, CHUNK = 1024, 32
T_OF = {1024: 65537, 2048: 65537, 4096: 65537, 32768: 786433}

_CACHE = {}


def _shape(O, n, bits):
    """(q, L, t, oracle context, specification) of a chain, built once"""
    key = ("shape", n, tuple(bits))
    if key not in _CACHE:
        q = O.coeff_modulus_create(n, bits)
        L, t = len(q) - 1, T_OF[n]
        _CACHE[key] = (q, L, t, O.Context("bfv", n, q, t), BfvDotSpec(O, n, q, L, t))
    return _CACHE[key]


def _case(O, n, bits, terms, batch):
    """operands a[t][item], b[t][item] ([2][L][N]) and the expected sums [batch][3][L][N], computed once per case and left unchanged"""
    key = ("case", n, tuple(bits), terms, batch)
    if key not in _CACHE:
        q, L, t, ctx, spec = _shape(O, n, bits)
        a = [[ctx.random_ct(1000 * k + 10 * i + 1, 2, L) for i in range(batch)] for k in range(terms)]
        b = [[ctx.random_ct(1000 * k + 10 * i + 2, 2, L) for i in range(batch)] for k in range(terms)]
        want = np.stack([spec.dot([a[k][i] for k in range(terms)], [b[k][i] for k in range(terms)]) for i in range(batch)])
        _CACHE[key] = (a, b, want)
    return _CACHE[key]


def _handles(pkg, dev, n, q, L, t):
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    return plan, pkg.Behz(plan, L, t)


def _clean_env(monkeypatch, env=()):
    for k in OPTION_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def _run(O, pkg, dev, n, bits, terms, batch):
    q, L, t, ctx, spec = _shape(O, n, bits)
    a, b, want = _case(O, n, bits, terms, batch)
    plan, behz = _handles(pkg, dev, n, q, L, t)
    da = [pkg.to_device(np.stack(x), dev) for x in a]
    db = [pkg.to_device(np.stack(x), dev) for x in b]
    got = behz.bfv_multiply_accumulate(da, db)
    torch.cuda.synchronize()
    assert np.array_equal(pkg.to_host(got), want)
    return behz, da, db, got


@pytest.mark.parametrize("n,bits,terms,batch", [
    (1024, [40, 40, 40], 1, 1), (1024, [40, 40, 40], 1, 3), (1024, [40, 40, 40], 2, 1), (1024, [40, 40, 40], 2, 3),
    (1024, [40, 40, 40], 5, 1), (1024, [40, 40, 40], 5, 3),
    (4096, [60, 40, 40, 60], 3, 2),          # both arithmetic classes in one chain
    (32768, [50, 50, 50], 3, 1),             # the accumulating kernel between the fused lift / floor launches
    (32768, [60, 50, 50, 60], 2, 1),         # limbs of the integer class at a two-pass size
])
def test_sum_equals_the_specification(O, pkg, dev, monkeypatch, n, bits, terms, batch):
    _clean_env(monkeypatch)
    behz, da, db, got = _run(O, pkg, dev, n, bits, terms, batch)
    if terms == 1:
        q, L, t, ctx, spec = _shape(O, n, bits)
        assert torch.equal(got, behz.multiply(da[0], 2, db[0], 2))


@pytest.mark.parametrize("n,terms", [(1024, 2), (32768, 3)])
@pytest.mark.parametrize("env", [(("TROYN_BEHZ", "v1"),), (("TROYN_BFV_TENSOR", "split"),), (("TROYN_BFV_TENSOR", "fused"),),
                                 (("TROYN_BEHZ_BASE", "ref"),), (("TROYN_BEHZ_LIFT", "split"),)], ids=lambda e: "%s=%s" % e[0])
def test_same_words_under_every_plan_option(O, pkg, dev, monkeypatch, env, n, terms):
    _clean_env(monkeypatch, env)
    _run(O, pkg, dev, n, [40, 40, 40] if n == 1024 else [50, 50, 50], terms, 1)


def test_chunk_boundary_and_workspace_plateau(O, pkg, dev, monkeypatch):
    """33 terms cross the chunk of 32: the second chunk adds into the accumulator; the workspace stops growing at one chunk"""
    _clean_env(monkeypatch)
    n, bits = 1024, [40, 40, 40]
    behz, da, db, got = _run(O, pkg, dev, n, bits, CHUNK + 1, 1)
    lib = pkg.capi.lib()
    for fn in (lib.troyn_bfv_multiply_accumulate_workspace_bytes, lib.troyn_bfv_multiply_accumulate_relinearize_workspace_bytes):
        sizes = [int(fn(behz.h, k, 2)) for k in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, CAP)]
        assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] == sizes[4] == sizes[5]
        assert int(fn(behz.h, 0, 2)) == 0 and int(fn(behz.h, CAP + 1, 2)) == 0


def test_chunk_boundary_on_the_accumulating_kernel(O, pkg, dev, monkeypatch):
    """the same at N = 32768: the kernel's add-to-what-is-there form.  Two ciphertexts in rotating roles keep the specification cheap."""
    _clean_env(monkeypatch)
    n, bits = 32768, [50, 50, 50]
    q, L, t, ctx, spec = _shape(O, n, bits)
    x, y = ctx.random_ct(71, 2, L), ctx.random_ct(73, 2, L)
    # 33 terms: 20 x (x, y), 12 x (x, x), 1 x (y, y) -- the last one alone in the second chunk
    want = spec.finish(spec.add(spec.add(spec.scale(spec.tensor(spec.lift(x), spec.lift(y)), 20), spec.scale(spec.tensor(spec.lift(x), spec.lift(x)), 12)),
                                spec.tensor(spec.lift(y), spec.lift(y))))
    plan, behz = _handles(pkg, dev, n, q, L, t)
    dx, dy = pkg.to_device(x[None], dev), pkg.to_device(y[None], dev)
    got = behz.bfv_multiply_accumulate([dx] * 32 + [dy], [dy] * 20 + [dx] * 12 + [dy])
    torch.cuda.synchronize()
    assert np.array_equal(pkg.to_host(got)[0], want)


def test_aliasing(O, pkg, dev, monkeypatch):
    """a[t] == b[t] (squares) and one pointer repeated in several terms"""
    _clean_env(monkeypatch)
    n, bits = 2048, [40, 40, 40]
    q, L, t, ctx, spec = _shape(O, n, bits)
    x, y, z = (ctx.random_ct(s, 2, L) for s in (81, 83, 85))
    plan, behz = _handles(pkg, dev, n, q, L, t)
    dx, dy, dz = (pkg.to_device(v[None], dev) for v in (x, y, z))
    got = behz.bfv_multiply_accumulate([dx, dy, dx, dz], [dx, dy, dy, dx])
    torch.cuda.synchronize()
    assert np.array_equal(pkg.to_host(got)[0], spec.dot([x, y, x, z], [x, y, y, x]))


@pytest.mark.parametrize("n,bits", [(1024, [40, 40, 40]), (32768, [50, 50, 50])])
def test_worst_case_at_the_cap(O, pkg, dev, monkeypatch, n, bits):
    """every coefficient floor(q / 2), 1024 terms of that one pair: the largest sum the entries accept.  The specification works in the reference's
    61-bit base and the library (here) in primes below 2^50, so an overflow of either base shows as unequal words."""
    _clean_env(monkeypatch)
    q, L, t, ctx, spec = _shape(O, n, bits)
    half = 1
    for p in q[:L]:
        half *= int(p)
    half //= 2
    x = np.empty((2, L, n), dtype=np.uint64)
    for l in range(L):
        x[:, l, :] = half % int(q[l])
    want = spec.repeated(x, x, CAP)
    plan, behz = _handles(pkg, dev, n, q, L, t)
    dx = pkg.to_device(x[None], dev)
    got = behz.bfv_multiply_accumulate([dx] * CAP, [dx] * CAP)
    torch.cuda.synchronize()
    assert np.array_equal(pkg.to_host(got)[0], want)


@pytest.mark.parametrize("n,bits,terms", [(1024, [40, 40, 40], 2), (32768, [50, 50, 50], 3)])
def test_relinearizing_entry(O, pkg, dev, monkeypatch, n, bits, terms):
    _clean_env(monkeypatch)
    q, L, t, ctx, spec = _shape(O, n, bits)
    a, b, want3 = _case(O, n, bits, terms, 1)
    keys = ctx.random_keys(7, L)
    want = ctx.relinearize(L, False, want3[0], keys)
    plan, behz = _handles(pkg, dev, n, q, L, t)
    dkeys = [pkg.to_device(k, dev) for k in keys]
    da = [pkg.to_device(np.stack(v), dev) for v in a]
    db = [pkg.to_device(np.stack(v), dev) for v in b]
    got = behz.bfv_multiply_accumulate_relinearize(da, db, dkeys)
    torch.cuda.synchronize()
    assert np.array_equal(pkg.to_host(got)[0], want)


def test_refusals(O, pkg, dev, monkeypatch):
    _clean_env(monkeypatch)
    n, bits = 1024, [40, 40, 40]
    q, L, t, ctx, spec = _shape(O, n, bits)
    plan, behz = _handles(pkg, dev, n, q, L, t)
    lib = pkg.capi.lib()
    bad = pkg.capi.TroynInvalidArgument
    x = pkg.to_device(ctx.random_ct(91, 2, L)[None], dev)
    keys = [pkg.to_device(k, dev) for k in ctx.random_keys(7, L)]
    vp = C.c_void_p
    tab = lambda ptrs: (vp * max(len(ptrs), 1))(*ptrs)
    out3 = torch.zeros((1, 3, L, n), dtype=torch.int64, device=dev)
    need = int(lib.troyn_bfv_multiply_accumulate_workspace_bytes(behz.h, 2, 1))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    px, po, pw = x.data_ptr(), out3.data_ptr(), ws.data_ptr()

    def call(a, b, terms, out=po, wsp=pw, wbytes=need, batch=1):
        return lib.troyn_bfv_multiply_accumulate(behz.h, a, b, terms, vp(out), vp(wsp), wbytes, batch, None)
    INVALID, WORKSPACE = -1, -3
    assert call(tab([px, px]), tab([px, px]), 2) == 0                                  # the well-formed call
    assert call(tab([px]), tab([px]), 0) == INVALID                                    # no terms
    assert call(tab([px] * (CAP + 1)), tab([px] * (CAP + 1)), CAP + 1) == INVALID      # above the cap
    assert call(None, tab([px]), 1) == INVALID and call(tab([px]), None, 1) == INVALID # a null table
    assert call(tab([px, None]), tab([px, px]), 2) == INVALID                          # a null entry
    assert call(tab([px, px + 8]), tab([px, px]), 2) == INVALID                        # a misaligned pointer
    assert call(tab([px, px]), tab([px, px]), 2, out=px) == INVALID                    # out overlaps an input
    assert call(tab([px, px]), tab([px, px]), 2, out=px + 2 * L * n * 8 - 16) == INVALID
    assert call(tab([px, px]), tab([px, px]), 2, wbytes=need - 1) == WORKSPACE
    assert b"workspace too small" in lib.troyn_last_error()
    assert call(tab([px, px]), tab([px, px]), 2, out=None, wsp=None, wbytes=0, batch=0) == 0      # nothing to do: neither is looked at
    # the relinearizing entry: the same checks, and its keys
    need2 = int(lib.troyn_bfv_multiply_accumulate_relinearize_workspace_bytes(behz.h, 2, 1))
    ws2 = torch.zeros(need2, dtype=torch.uint8, device=dev)
    out2 = torch.zeros((1, 2, L, n), dtype=torch.int64, device=dev)
    kp = plan._key_ptrs(keys, L)

    def call2(a, b, terms, k=kp, out=out2.data_ptr(), wsp=ws2.data_ptr(), wbytes=need2, batch=1):
        return lib.troyn_bfv_multiply_accumulate_relinearize(behz.h, a, b, terms, k, vp(out), vp(wsp), wbytes, batch, None)
    assert call2(tab([px, px]), tab([px, px]), 2) == 0
    assert call2(tab([px]), tab([px]), 0) == INVALID
    assert call2(tab([px] * (CAP + 1)), tab([px] * (CAP + 1)), CAP + 1) == INVALID
    assert call2(tab([px]), tab([px]), 1, k=None) == INVALID
    assert call2(tab([px, None]), tab([px, px]), 2) == INVALID
    assert call2(tab([px, px + 8]), tab([px, px]), 2) == INVALID
    assert call2(tab([px, px]), tab([px, px]), 2, out=px) == INVALID
    assert call2(tab([px, px]), tab([px, px]), 2, wbytes=need2 - 1) == WORKSPACE
    assert call2(tab([px, px]), tab([px, px]), 2, out=None, wsp=None, wbytes=0, batch=0) == 0
    torch.cuda.synchronize()
    # through the engine: lists of different lengths and the cap raise the argument error
    with pytest.raises(bad):
        behz.bfv_multiply_accumulate([x, x], [x])
    with pytest.raises(bad):
        behz.bfv_multiply_accumulate([x] * (CAP + 1), [x] * (CAP + 1))
