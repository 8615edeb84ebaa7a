"""troyn_ckks_mod_raise (include/troyn.h) against the integer specification (tests/mod_raise_spec.py): exact equality of every word.

Coefficient form: the specification itself.  NTT form: NTT o extend o INTT with the oracle's transforms -- the input is the forward transform of the
coefficient-form words, so the planted values sit where they are meant to.  Shapes: log_n = 5 (partial workgroups; L_in = 1, the LM = 16
instantiation at its limit, and 17 limbs refused), log_n = 12 on {60,40,40,40,40,60} (LM = 1, 2, 4, 8; mixed prime sizes), log_n = 13 on six 50-bit primes
(where the NTT layer changes kernel family).  One reference per shape for 3 items x 3 polynomials; the cases read slices of it."""
import ctypes as C

import numpy as np
import pytest
import torch

import mod_raise_spec as S

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
CHAINS = {5: [30] * 18, 12: [60, 40, 40, 40, 40, 60], 13: [50] * 6}
SHAPES = [(5, 1, 4), (5, 16, 17), (12, 1, 6), (12, 2, 6), (12, 3, 6), (12, 5, 6), (13, 2, 6)]
GUARD = 64                                     # words after `out` and after the workspace
SENTINEL = 0x5A5A5A5A5A5A5A5A
_plans, _refs = {}, {}


def _setup(O, pkg, dev, log_n):
    if log_n not in _plans:
        n = 1 << log_n
        moduli = [int(q) for q in O.coeff_modulus_create(n, CHAINS[log_n])]
        plan = pkg.Plan(dev, log_n, moduli)
        _plans[log_n] = (plan, plan.ckks_handle(), moduli, [O.NTTTables(log_n, q) for q in moduli])
    return _plans[log_n]


def _ntt(O, rows, log_n, tabs):
    L = rows.shape[0]
    return O.ntt_forward(np.ascontiguousarray(rows, dtype=np.uint64).copy().reshape(-1), 1, L, log_n, tabs).reshape(L, 1 << log_n)


def _reference(O, log_n, L_in, L_out, moduli, tabs):
    """3 x 3 polynomials: coefficient-form input and result, and both in NTT form.  Random canonical words; the planted values at the first and the
    last coefficients of every polynomial, the ties after the first ones"""
    key = (log_n, L_in, L_out)
    if key not in _refs:
        n = 1 << log_n
        rng = np.random.default_rng(31 * log_n + 7 * L_in + L_out)
        inp = moduli[:L_in]
        planted = S.residues_of(S.planted_values(inp), inp)                  # eight values: four at each end of every polynomial
        ties = S.tie_values(inp, rng)
        room = n - 8 - n // 4                                                # a quarter of a polynomial stays random
        chunks = [ties[k:k + room] for k in range(0, len(ties), room)]       # one chunk but at n = 32, L_in = 16: three, one per polynomial index
        assert len(chunks) <= 3
        coef_in = np.zeros((3, 3, L_in, n), dtype=np.uint64)
        coef_out = np.zeros((3, 3, L_out, n), dtype=np.uint64)
        ntt_in, ntt_out = np.zeros_like(coef_in), np.zeros_like(coef_out)
        for b in range(3):
            for c in range(3):
                res = np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in inp])
                res[:, :4], res[:, n - 4:] = planted[:, :4], planted[:, 4:]
                chunk = chunks[c % len(chunks)]
                res[:, 4:4 + len(chunk)] = S.residues_of(chunk, inp)
                coef_in[b, c] = res
                coef_out[b, c] = S.mod_raise_rows(res, moduli, L_in, L_out)
                ntt_in[b, c] = _ntt(O, res, log_n, tabs[:L_in])
                ntt_out[b, c, :L_in] = ntt_in[b, c]
                ntt_out[b, c, L_in:] = _ntt(O, coef_out[b, c, L_in:], log_n, tabs[L_in:L_out])
        _refs[key] = (coef_in, coef_out, ntt_in, ntt_out)
    return _refs[key]


def _call(lib, h, L_in, L_out, ntt, src, pcount, batch, dev, stream=None):
    """the C-ABI entry on guarded buffers: (rc, out words, guards intact)"""
    n = src.shape[-1]
    words = batch * pcount * L_out * n
    out = torch.full((words + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    nbytes = lib.troyn_ckks_mod_raise_workspace_bytes(h, L_in, L_out, pcount, batch, ntt)
    assert nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()                       # the fills above ran on the current stream
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.troyn_ckks_mod_raise(h, L_in, L_out, ntt, C.c_void_p(src.data_ptr()), pcount, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, batch, st)
    (stream or torch.cuda.current_stream()).synchronize()
    intact = bool((out[words:] == SENTINEL).all()) and bool((ws[nbytes // 8:] == SENTINEL).all())
    return rc, out[:words].cpu().numpy().view(np.uint64).reshape(batch, pcount, L_out, n), intact, nbytes


@pytest.mark.parametrize("ntt", [0, 1])
@pytest.mark.parametrize("pcount", [2, 3])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log_n,L_in,L_out", SHAPES)
def test_mod_raise_matches_spec(O, pkg, dev, log_n, L_in, L_out, batch, pcount, ntt):
    plan, enc, moduli, tabs = _setup(O, pkg, dev, log_n)
    coef_in, coef_out, ntt_in, ntt_out = _reference(O, log_n, L_in, L_out, moduli, tabs)
    # the last item and the last polynomial of the reference are part of every slice
    pick_b, pick_c = [0, 1, 2][-batch:], [0, 1, 2][-pcount:]
    src_h = np.ascontiguousarray((ntt_in if ntt else coef_in)[pick_b][:, pick_c])
    want = (ntt_out if ntt else coef_out)[pick_b][:, pick_c]
    src = pkg.to_device(src_h, dev)
    rc, got, intact, nbytes = _call(plan.lib, enc.h, L_in, L_out, ntt, src, pcount, batch, dev)
    assert rc == 0
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, :, :L_in], src_h)                           # the low rows are the input, word for word
    assert np.array_equal(pkg.to_host(src), src_h)                           # the input is not written
    assert intact                                                            # nothing beyond `out` or the workspace's size
    assert (nbytes == 0) == (ntt == 0)
    # the engine wrapper takes the same path
    assert np.array_equal(pkg.to_host(enc.mod_raise(src, L_in, L_out, pcount, bool(ntt))), want)


def test_reference_holds_both_signs_and_the_planted_values(O, pkg, dev):
    plan, enc, moduli, tabs = _setup(O, pkg, dev, 12)
    coef_in, coef_out, _, _ = _reference(O, 12, 3, 6, moduli, tabs)
    Q = S.product(moduli[:3])
    xs = [S.centre(X, Q) for X in S.compose(coef_in[0, 0], moduli[:3])]
    assert min(xs) < 0 < max(xs)
    q0 = moduli[0]
    assert xs[:4] + xs[-4:] == [0, 1, -1, Q // 2, Q // 2 + 1 - Q, -1, Q // 2 + q0 - Q, Q // 2 - q0]
    assert [int(v) for v in coef_out[0, 0, 3, :3]] == [0, 1, moduli[3] - 1]


def test_seventeen_input_limbs_are_unsupported(O, pkg, dev):
    plan, enc, moduli, tabs = _setup(O, pkg, dev, 5)
    src = torch.zeros((1, 2, 17, 32), dtype=torch.int64, device=dev)
    rc, got, intact, _ = _call(plan.lib, enc.h, 17, 18, 1, src, 2, 1, dev)
    assert rc == UNSUPPORTED and intact
    assert (got == np.uint64(SENTINEL)).all()
    rc, got, intact, _ = _call(plan.lib, enc.h, 17, 18, 0, src, 2, 1, dev)
    assert rc == UNSUPPORTED and intact and (got == np.uint64(SENTINEL)).all()


def test_non_default_stream_gives_the_same_words(O, pkg, dev):
    for log_n, L_in, ntt in ((12, 2, 1), (12, 5, 0), (13, 2, 1)):
        plan, enc, moduli, tabs = _setup(O, pkg, dev, log_n)
        coef_in, coef_out, ntt_in, ntt_out = _reference(O, log_n, L_in, 6, moduli, tabs)
        src = pkg.to_device(np.ascontiguousarray(ntt_in if ntt else coef_in), dev)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        rc, got, intact, _ = _call(plan.lib, enc.h, L_in, 6, ntt, src, 3, 3, dev, stream=side)
        assert rc == 0 and intact
        assert np.array_equal(got, ntt_out if ntt else coef_out)


def test_refusals_and_batch_zero(O, pkg, dev):
    plan, enc, moduli, tabs = _setup(O, pkg, dev, 12)
    lib, h, n = plan.lib, enc.h, 4096
    coef_in, coef_out, ntt_in, ntt_out = _reference(O, 12, 2, 6, moduli, tabs)
    src = pkg.to_device(np.ascontiguousarray(ntt_in[:1, :2]), dev)
    out = torch.full((2 * 6 * n + 2,), SENTINEL, dtype=torch.int64, device=dev)
    nbytes = lib.troyn_ckks_mod_raise_workspace_bytes(h, 2, 6, 2, 1, 1)
    assert nbytes >= 2 * 6 * n * 8                                           # the coefficient forms of the input rows and of the new rows
    ws = torch.full((nbytes // 8 + 2,), SENTINEL, dtype=torch.int64, device=dev)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(L_in=2, L_out=6, ntt=1, i=vp(src), pcount=2, o=vp(out), w=vp(ws), wb=nbytes, batch=1, hh=h):
        return lib.troyn_ckks_mod_raise(hh, L_in, L_out, ntt, i, pcount, o, w, wb, batch, st)
    # batch == 0 touches nothing (null buffers are fine); only the handle and the limb counts are looked at before
    assert call(i=None, o=None, w=None, wb=0, batch=0) == 0
    assert call(batch=0) == 0
    assert call(batch=0, L_in=6) == INVALID and call(batch=0, hh=None) == INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    # limb counts
    assert call(L_in=0) == INVALID and call(L_in=2, L_out=2) == INVALID and call(L_in=3, L_out=2) == INVALID and call(L_out=7) == INVALID
    for bad in ((0, 6), (2, 2), (3, 2), (2, 7)):
        assert lib.troyn_ckks_mod_raise_workspace_bytes(h, bad[0], bad[1], 2, 1, 1) == 0
    # pointers
    assert call(hh=None) == INVALID and call(i=None) == INVALID and call(o=None) == INVALID
    assert call(i=vp(src, 8)) == INVALID and call(o=vp(out, 8)) == INVALID and call(w=vp(ws, 8)) == INVALID
    assert call(o=vp(src)) == INVALID and call(o=vp(src, 16 * n)) == INVALID  # `out` overlapping `in`
    # workspace
    assert call(wb=nbytes - 1) == WORKSPACE and call(w=None) == WORKSPACE and call(w=None, wb=0) == WORKSPACE
    assert lib.troyn_ckks_mod_raise_workspace_bytes(h, 2, 6, 2, 1, 0) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())    # a refused call has written nothing
    # coefficient form needs no workspace at all
    csrc = pkg.to_device(np.ascontiguousarray(coef_in[:1, :2]), dev)
    assert call(ntt=0, i=vp(csrc), w=None, wb=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:2 * 6 * n].cpu().numpy().view(np.uint64).reshape(1, 2, 6, n), coef_out[:1, :2])
    assert bool((out[2 * 6 * n:] == SENTINEL).all())
    # and the full call
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:2 * 6 * n].cpu().numpy().view(np.uint64).reshape(1, 2, 6, n), ntt_out[:1, :2])
    assert bool((out[2 * 6 * n:] == SENTINEL).all()) and bool((ws[nbytes // 8:] == SENTINEL).all())
