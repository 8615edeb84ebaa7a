"""Fused multiply -> relinearize -> rescale at N = 16384, all-FP64 chain, batches beyond the small-batch forms: step (1), digits = INTT(a1 (.) b1), runs on
half-limb tiles with two workgroups per CU (csrc/mulpair_half_kernels.hpp, mulpair_half_kernel; selected in csrc/troyn.hip mrr_digits under
mrr_whole_limb_class, the class mrr_tail_kernel serves).  Every digit is the same canonical integer the whole-limb kernel stores, so the fused entry must
equal the three library calls (dyadic_convolute -> relinearize -> divide_and_round_q_last_ntt) on every item, the CPU oracle on the items checked, and the
same call with TROYN_MULPAIR_HALF=0 (the whole-limb kernel) word for word.

Store formats: the kernel stores its digits as doubles (NTT_FLAG_STORE_F64) or as words.  It is selected for all-FP64 chains only, and those always hand
ksmac2 doubles; the chains that hand over words (a modulus of 2^50 or more, TROYN_NTT_ARITH=u64) are not all-FP64 and keep the whole-limb kernel.  The words
form is therefore not reachable through the library's switches for this class and is not forced here; tools/fp64_half_check.cpp
(tests/test_fp64_bounds_half.py) replays both forms of the last step on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, BITS, LTOP = 16384, [50] * 6, 5
SMALL_LP_FACTOR = 2      # csrc/launch.hpp TROYN_SMALL_LP_FACTOR: a launch of at most CUs / 2 limb-polynomials counts as small


def _smallest_selecting_batch(dev, L):
    """mrr_whole_limb_class (csrc/troyn.hip): not small_tail_wanted, i.e. batch * 2 * (L - 1) limb-polynomials * TROYN_SMALL_LP_FACTOR > CUs"""
    import torch
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return cus // (SMALL_LP_FACTOR * 2 * (L - 1)) + 1


@pytest.fixture(scope="module")
def env(O, pkg, dev):
    q = O.coeff_modulus_create(N, BITS)
    ctx, plan = O.Context("ckks", N, q), pkg.Plan(dev, N.bit_length() - 1, q)
    keys = {L: ctx.random_keys(31 + L, L) for L in (LTOP, 3)}
    dkeys = {L: [pkg.to_device(k, dev) for k in ks] for L, ks in keys.items()}
    return ctx, plan, q, keys, dkeys


def _uniform(torch, q, L, batch, dev, seed):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.empty((batch, 2, L, N), dtype=torch.int64, device=dev)
        for l in range(L):
            x[:, :, l, :] = torch.randint(0, int(q[l]), (batch, 2, N), dtype=torch.int64, device=dev, generator=gen)
        out.append(x)
    return out


def _three_calls(plan, L, a, b, dkeys):
    prod = plan.dyadic_convolute(a, 2, b, 2, L)
    relin = plan.relinearize(L, prod, dkeys, is_ckks=True, is_ntt_form=True)
    return plan.divide_and_round_q_last_ntt(L, relin, 2)


def _check(torch, pkg, env, L, a, b, oracle_items):
    ctx, plan, q, keys, dkeys = env
    a0, b0 = a.clone(), b.clone()
    fused = plan.ckks_multiply_relinearize_rescale(L, a, b, dkeys[L])
    three = _three_calls(plan, L, a, b, dkeys[L])
    assert torch.equal(a, a0) and torch.equal(b, b0), "operands were written"
    diff = (fused != three).flatten(1).any(1).nonzero().flatten().tolist()
    assert not diff, "fused entry differs from the three calls on items %s" % diff[:16]
    for i in oracle_items:
        e = ctx.relinearize(L, True, ctx.ckks_multiply(L, pkg.to_host(a[i]), pkg.to_host(b[i])), keys[L])
        assert np.array_equal(pkg.to_host(fused[i]), ctx.mod_switch_scale_to_next(L, e)), i
    return fused


@pytest.mark.parametrize("L", [LTOP, 3])
@pytest.mark.parametrize("extra", [0, 3])
def test_smallest_batches_that_select_the_kernel(O, pkg, dev, env, L, extra):
    """the smallest batch that selects the kernel and that batch + 3 (odd item count: neither a whole XCD group nor a whole wave of workgroups), at the
    top level L = 5 and at L = 3 on the same plan (other limb count and strides): every item against the three calls, items {0, 1, B - 1} against the oracle"""
    import torch
    batch = _smallest_selecting_batch(dev, L) + extra
    a, b = _uniform(torch, env[2], L, batch, dev, 100 * L + batch)
    _check(torch, pkg, env, L, a, b, [0, 1, batch - 1])


def _corner_batch(torch, q, L, batch, dev):
    """polynomial 1 of items 2 .. 7 of a AND b, and of items 8 .. 13 of a alone (against a uniform b1): all q - 1 | all zero | impulse at 0 | impulse at
    N - 1 | impulses at 8191 and 8192 (the two sides of the half boundary) | alternating 0, q - 1"""
    a, b = _uniform(torch, q, L, batch, dev, 4242)
    top = torch.tensor([int(v) - 1 for v in q[:L]], dtype=torch.int64, device=dev)[:, None]      # [L][1]
    pats = []
    z = torch.zeros((L, N), dtype=torch.int64, device=dev)
    pats.append(top.expand(L, N).clone())
    pats.append(z.clone())
    for idx in ([0], [N - 1], [8191, 8192]):
        x = z.clone()
        for i in idx:
            x[:, i] = top[:, 0]
        pats.append(x)
    alt = z.clone()
    alt[:, 1::2] = top
    pats.append(alt)
    for k, x in enumerate(pats):
        a[2 + k, 1] = x
        b[2 + k, 1] = x
        a[8 + k, 1] = x
    return a, b


def test_corner_operands(O, pkg, dev, env):
    """corner values of a1 and b1 against the three calls (every item) and the oracle (every corner item)"""
    import torch
    batch = max(_smallest_selecting_batch(dev, LTOP), 14)
    a, b = _corner_batch(torch, env[2], LTOP, batch, dev)
    _check(torch, pkg, env, LTOP, a, b, list(range(2, 14)))


def test_switch_restores_the_whole_limb_kernel(O, pkg, dev, env):
    """TROYN_MULPAIR_HALF=0 (Plan.set_option) runs the whole-limb kernel: the same inputs give word-identical output"""
    import torch
    ctx, plan, q, keys, dkeys = env
    batch = max(_smallest_selecting_batch(dev, LTOP), 14) + 3
    a, b = _corner_batch(torch, q, LTOP, batch, dev)
    half = plan.ckks_multiply_relinearize_rescale(LTOP, a, b, dkeys[LTOP])
    plan.set_option("TROYN_MULPAIR_HALF", "0")
    try:
        whole = plan.ckks_multiply_relinearize_rescale(LTOP, a, b, dkeys[LTOP])
    finally:
        plan.set_option("TROYN_MULPAIR_HALF", None)
    assert torch.equal(half, whole)
    with pytest.raises(Exception):
        plan.set_option("TROYN_MULPAIR_HALF", "2")      # not a value of this option
