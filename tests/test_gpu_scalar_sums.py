"""GPU parity of troyn_scalar_weighted_sums through Plan.scalar_weighted_sums: word for word against tests/scalar_sums_spec.py (the contract
of include/troyn.h in Python big integers) and against multiply_scalar + add composed on the device; every refusal; batch == 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import scalar_sums_spec as S

pytestmark = pytest.mark.gpu

NMOD = 3
CHAINS = {"40": [40] * 5 + [60], "60": [60] * 6}      # the FP64-capable class and the integer class; 5 data limbs so inputs can be taller
_PLANS = {}


def _plan(O, pkg, dev, n, bits):
    key = (n, tuple(bits))
    if key not in _PLANS:
        q = O.coeff_modulus_create(n, bits)
        _PLANS[key] = (pkg.Plan(dev, n.bit_length() - 1, q), [int(x) for x in q])
    return _PLANS[key]


def _inputs(rng, q, n, batch, pcount, terms, nmod, extra=(0, 1, 2)):
    """random canonical residues in the first nmod limbs; the limbs beyond hold all-ones words, which no modulus admits"""
    xs, rows = [], []
    for t in range(terms):
        r = nmod + extra[t % len(extra)]
        x = np.full((batch, pcount, r, n), np.uint64((1 << 64) - 1), dtype=np.uint64)
        for l in range(nmod):
            x[:, :, l, :] = rng.integers(0, q[l], size=(batch, pcount, n), dtype=np.uint64)
        xs.append(x)
        rows.append(r)
    return xs, rows


def _scalars(rng, q, terms, slots, nmod):
    """random residues with the words q - 1, 1 and 0 planted on a diagonal pattern"""
    def word(s, t, l):
        k = (s + t + l) % 4
        return int(rng.integers(0, q[l], dtype=np.uint64)) if k == 0 else (q[l] - 1, 1, 0)[k - 1]
    sc = [[[word(s, t, l) for l in range(nmod)] for t in range(terms)] for s in range(slots)]
    cs = [[(q[l] - 1) if (s + l) % 3 == 0 else int(rng.integers(0, q[l], dtype=np.uint64)) for l in range(nmod)] for s in range(slots)]
    return sc, cs


def _run(pkg, plan, dev, xs, rows, sc, cs, at0, pcount, nmod=NMOD, **kw):
    dx = [pkg.to_device(x, dev) for x in xs]
    out = plan.scalar_weighted_sums(dx, rows, sc, nmod, pcount, constants=cs, constant_at_index0=at0, **kw)
    torch.cuda.synchronize()
    for x, d in zip(xs, dx):      # the inputs are left untouched
        assert np.array_equal(pkg.to_host(d), x)
    return out


@pytest.mark.parametrize("mode", ["none", "every", "index0"])
@pytest.mark.parametrize("terms,slots", [(1, 1), (3, 3), (9, 5), (2, 9)])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("pcount", [2, 3])
@pytest.mark.parametrize("chain", ["40", "60"])
def test_small_cases_vs_spec(O, pkg, dev, chain, pcount, batch, terms, slots, mode):
    n = 32
    plan, q = _plan(O, pkg, dev, n, CHAINS[chain])
    rng = np.random.default_rng(1000 * terms + 10 * slots + batch + pcount)
    xs, rows = _inputs(rng, q, n, batch, pcount, terms, NMOD)
    sc, cs = _scalars(rng, q, terms, slots, NMOD)
    cs = None if mode == "none" else cs
    out = _run(pkg, plan, dev, xs, rows, sc, cs, mode == "index0", pcount)
    assert tuple(out.shape) == (slots, batch, pcount, NMOD, n)
    want = S.scalar_weighted_sums(q[:NMOD], xs, sc, cs, mode == "index0")
    assert np.array_equal(pkg.to_host(out), want)


def test_modulus_slice_with_offset(O, pkg, dev):
    """mod_start > 0: limb l of every input is under modulus mod_start + l"""
    n = 32
    plan, q = _plan(O, pkg, dev, n, CHAINS["40"])
    rng = np.random.default_rng(5)
    xs, rows = _inputs(rng, q[2:], n, 2, 2, 3, NMOD, extra=(0, 1))
    sc, cs = _scalars(rng, q[2:], 3, 2, NMOD)
    out = _run(pkg, plan, dev, xs, rows, sc, cs, False, 2, mod_start=2)
    assert np.array_equal(pkg.to_host(out), S.scalar_weighted_sums(q[2:2 + NMOD], xs, sc, cs, False))


def test_seventy_terms_cross_the_accumulation_cut(O, pkg, dev):
    """60-bit moduli, every input word and every scalar q - 1: 64 such products fill the 128-bit accumulator's bound, 70 need the carry"""
    n, terms, slots = 32, 70, 3
    plan, q = _plan(O, pkg, dev, n, CHAINS["60"])
    rng = np.random.default_rng(70)
    xs, rows = _inputs(rng, q, n, 2, 2, terms, NMOD)
    for x in xs[::2]:
        for l in range(NMOD):
            x[:, :, l, :] = q[l] - 1
    sc, cs = _scalars(rng, q, terms, slots, NMOD)
    sc[0] = [[q[l] - 1 for l in range(NMOD)] for _ in range(terms)]
    out = _run(pkg, plan, dev, xs, rows, sc, cs, False, 2)
    assert np.array_equal(pkg.to_host(out), S.scalar_weighted_sums(q[:NMOD], xs, sc, cs, False))


def test_real_grid(O, pkg, dev):
    """N = 16384, L = 5, 7 terms, 8 slots, batch 2: full tiles of 8 on the grid the polynomial evaluation launches"""
    n, L, terms, slots, batch = 16384, 5, 7, 8, 2
    plan, q = _plan(O, pkg, dev, n, [50] * 6)
    rng = np.random.default_rng(16384)
    xs, rows = _inputs(rng, q, n, batch, 2, terms, L, extra=(0, 1))
    sc, cs = _scalars(rng, q, terms, slots, L)
    out = _run(pkg, plan, dev, xs, rows, sc, cs, False, 2, nmod=L)
    assert np.array_equal(pkg.to_host(out), S.scalar_weighted_sums(q[:L], xs, sc, cs, False))


def test_equals_multiply_scalar_and_add_on_the_device(O, pkg, dev):
    n, terms, slots, batch, pcount = 4096, 5, 3, 2, 2
    plan, q = _plan(O, pkg, dev, n, [60, 40, 40, 60])
    rng = np.random.default_rng(4096)
    xs, rows = _inputs(rng, q, n, batch, pcount, terms, NMOD, extra=(0,))
    sc, _ = _scalars(rng, q, terms, slots, NMOD)
    dx = [pkg.to_device(x, dev) for x in xs]
    out = plan.scalar_weighted_sums(dx, rows, sc, NMOD, pcount)
    for s in range(slots):
        acc = None
        for t in range(terms):
            prod = torch.empty_like(dx[t])
            for l in range(NMOD):      # troyn_multiply_scalar takes one scalar for its slice: limb by limb
                prod[:, :, l, :] = plan.multiply_scalar(dx[t][:, :, l, :].contiguous(), sc[s][t][l], 1, mod_start=l)
            acc = prod if acc is None else plan.add(acc, prod, NMOD)
        assert torch.equal(out[s], acc), s


# -- refusals ---------------------------------------------------------------------------------------------------------------------
def _raw(pkg, plan, ins, rows, terms, sc, cs, pcount, out, slots, batch, ws, ws_bytes, nmod=NMOD, mod_start=0):
    lib = pkg.capi.lib()
    parr = None if ins is None else (C.c_void_p * max(len(ins), 1))(*ins)
    narr = (C.c_uint32 * max(len(rows), 1))(*rows)
    sca = np.ascontiguousarray(np.array(sc, dtype=np.uint64)).reshape(-1)
    if sca.size == 0:
        sca = np.zeros(1, dtype=np.uint64)
    csa = None if cs is None else np.ascontiguousarray(np.array(cs, dtype=np.uint64)).reshape(-1)
    rc = lib.troyn_scalar_weighted_sums(plan.h, mod_start, nmod, parr, narr, terms, sca.ctypes.data_as(pkg.capi.p64),
                                        None if csa is None else csa.ctypes.data_as(pkg.capi.p64), 0, pcount, out, slots, batch, ws, ws_bytes, None)
    return rc, lib.troyn_last_error().decode()


def test_refusals(O, pkg, dev):
    n, terms, slots, batch, pcount = 32, 2, 2, 1, 2
    plan, q = _plan(O, pkg, dev, n, CHAINS["40"])
    rng = np.random.default_rng(9)
    xs, rows = _inputs(rng, q, n, batch, pcount, terms, NMOD, extra=(0,))
    sc, cs = _scalars(rng, q, terms, slots, NMOD)
    words = batch * pcount * NMOD * n
    buf = torch.zeros(terms * words + 2, dtype=torch.int64, device=dev)      # inputs at a 16-byte aligned base, one word to spare for the odd address
    for t, x in enumerate(xs):
        buf[t * words:(t + 1) * words] = pkg.to_device(x, dev).reshape(-1)
    base = buf.data_ptr()
    assert base % 16 == 0
    ins = [base + t * words * 8 for t in range(terms)]
    out = torch.zeros(slots * words, dtype=torch.int64, device=dev)
    nbytes = pkg.capi.lib().troyn_scalar_weighted_sums_workspace_bytes(plan.h, NMOD, terms, slots)
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    good = dict(ins=ins, rows=rows, terms=terms, sc=sc, cs=cs, pcount=pcount, out=out.data_ptr(), slots=slots, batch=batch, ws=ws.data_ptr(), ws_bytes=nbytes)
    rc, _ = _raw(pkg, plan, **good)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(pkg.to_host(out).reshape(slots, batch, pcount, NMOD, n), S.scalar_weighted_sums(q[:NMOD], xs, sc, cs, False))

    def refused(code=-1, **change):
        rc, msg = _raw(pkg, plan, **dict(good, **change))
        assert rc == code and "[troyn_scalar_weighted_sums]" in msg, (change.keys(), rc, msg)

    refused(terms=0)
    refused(slots=0)
    refused(pcount=0)
    refused(ins=None)                                           # a null table
    refused(ins=[ins[0], None])                                 # a null entry
    refused(ins=[ins[0], ins[1] + 8])                           # a misaligned input
    refused(out=out.data_ptr() + 8)                             # a misaligned destination
    refused(out=None)
    refused(ws=None)
    refused(rows=[NMOD, NMOD - 1])                              # in_nmod[t] < nmod
    refused(mod_start=len(q) - NMOD + 1)                        # a modulus slice outside the plan
    refused(nmod=0)
    bad = [[list(r) for r in row] for row in sc]
    bad[1][1][2] = q[2]
    refused(sc=bad)                                             # a scalar word >= its modulus
    badc = [list(r) for r in cs]
    badc[0][1] = q[1] + 5
    refused(cs=badc)                                            # a constant word >= its modulus
    refused(out=ins[1])                                         # out overlapping an input
    refused(out=ins[1] + (words - 2) * 8)                       # ... by its last words only
    refused(code=-3, ws_bytes=nbytes - 1)                       # TROYN_E_WORKSPACE
    torch.cuda.synchronize()

    # through Plan: a TroynInvalidArgument that names the entry
    dx = [pkg.to_device(x, dev) for x in xs]
    with pytest.raises(pkg.capi.TroynInvalidArgument, match="troyn_scalar_weighted_sums"):
        plan.scalar_weighted_sums(dx, [NMOD, NMOD - 1], sc, NMOD, pcount, batch=batch)
    with pytest.raises(pkg.capi.TroynInvalidArgument, match="troyn_scalar_weighted_sums"):
        plan.scalar_weighted_sums(dx, rows, bad, NMOD, pcount)


def test_batch_zero_with_null_buffers(O, pkg, dev):
    plan, q = _plan(O, pkg, dev, 32, CHAINS["40"])
    sc = [[[1] * NMOD, [2] * NMOD]]
    rc, _ = _raw(pkg, plan, ins=[None, None], rows=[NMOD, NMOD], terms=2, sc=sc, cs=None, pcount=2, out=None, slots=1, batch=0, ws=None, ws_bytes=0)
    assert rc == 0
    assert plan.scalar_weighted_sums([None, None], [NMOD, NMOD], sc, NMOD, 2, batch=0) is None
    rc, msg = _raw(pkg, plan, ins=[None, None], rows=[NMOD, NMOD], terms=0, sc=sc, cs=None, pcount=2, out=None, slots=1, batch=0, ws=None, ws_bytes=0)
    assert rc == -1 and "no terms" in msg      # the shape of the call is still checked
