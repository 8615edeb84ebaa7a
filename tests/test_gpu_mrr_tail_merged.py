"""Fused multiply -> relinearize -> rescale at N = 16384 with batches that fill the chip: the chain's tail (INTT of the special rows, LAST_LIMB,
TAIL_RESCALE) runs as ONE whole-limb launch with T_s and T_l in registers (csrc/troyn_mrr_tail.hip, mrr_tail_kernel).  Every value is the same exact
integer as in the three launches, so the result must equal the CPU oracle (ckks_multiply -> relinearize -> mod_switch_scale_to_next) AND the same call
with TROYN_MRR_SMALL=0 (the three launches), word for word, on both sides of the dispatch boundary (the largest batch that still takes the two-pass
form of a small launch, mrr_quartet_kernel, and the next one up) and at 64 and 1024; operands: uniform residues, all-zero, all q - 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, BITS, L = 16384, [50] * 6, 5
SMALL_LP_FACTOR = 2      # csrc/launch.hpp TROYN_SMALL_LP_FACTOR: a launch of at most CUs / 2 limb-polynomials counts as small


def _setup(O, pkg, dev, bits=BITS):
    q = O.coeff_modulus_create(N, bits)
    return O.Context("ckks", N, q), pkg.Plan(dev, N.bit_length() - 1, q), q


def _largest_small_batch(dev):
    """small_tail_wanted (csrc/troyn.hip): batch * 2 * (L - 1) limb-polynomials * TROYN_SMALL_LP_FACTOR <= CUs"""
    import torch
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return max(1, cus // (SMALL_LP_FACTOR * 2 * (L - 1)))


def _operands(torch, q, batch, dev, seed):
    """[batch][2][L][N] uniform residues below each limb's modulus; item 2 of a is all-zero, item 3 of a and of b all q - 1, item 4 of b all q - 1
    (against a uniform a), item 5 of b all-zero"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.empty((batch, 2, L, N), dtype=torch.int64, device=dev)
        for l in range(L):
            x[:, :, l, :] = torch.randint(0, int(q[l]), (batch, 2, N), dtype=torch.int64, device=dev, generator=gen)
        out.append(x)
    a, b = out
    top = torch.tensor([int(v) - 1 for v in q[:L]], dtype=torch.int64, device=dev)[None, :, None]
    a[2] = 0
    a[3] = top
    b[3] = top
    b[4] = top
    b[5] = 0
    return a, b


def _both_tails(plan, a, b, dkeys):
    merged = plan.ckks_multiply_relinearize_rescale(L, a, b, dkeys)
    plan.set_option("TROYN_MRR_SMALL", "0")
    try:
        three = plan.ckks_multiply_relinearize_rescale(L, a, b, dkeys)
    finally:
        plan.set_option("TROYN_MRR_SMALL", None)
    return merged, three


def _check_items(pkg, ctx, keys, a, b, got, items):
    for i in items:
        ai, bi = pkg.to_host(a[i]), pkg.to_host(b[i])
        e = ctx.relinearize(L, True, ctx.ckks_multiply(L, ai, bi), keys)
        assert np.array_equal(pkg.to_host(got[i]), ctx.mod_switch_scale_to_next(L, e)), i


@pytest.mark.parametrize("where", ["largest-small", "next-up", "64"])
def test_merged_tail_around_the_dispatch_boundary(O, pkg, dev, where):
    """every item against the oracle; the whole batch against the three launches"""
    import torch
    ctx, plan, q = _setup(O, pkg, dev)
    small = _largest_small_batch(dev)
    batch = {"largest-small": small, "next-up": small + 1, "64": 64}[where]
    batch = max(batch, 6)      # the corner operands sit in items 2 .. 5
    keys = ctx.random_keys(21, L)
    dkeys = [pkg.to_device(k, dev) for k in keys]
    a, b = _operands(torch, q, batch, dev, 1000 + batch)
    a0, b0 = a.clone(), b.clone()
    merged, three = _both_tails(plan, a, b, dkeys)
    assert torch.equal(merged, three), "merged tail differs from the three-launch tail"
    assert torch.equal(a, a0) and torch.equal(b, b0), "operands were written"
    _check_items(pkg, ctx, keys, a, b, merged, range(batch))


def test_merged_tail_batch_1024(O, pkg, dev):
    """the headline shape: items 0, 1, 7, 512, 1023, the corner operands (2 .. 5) and one item per residue modulo 8 (the inner product deals the items of a
    batch to the 8 XCDs by that residue) against the oracle; all 1024 against the three launches"""
    import torch
    ctx, plan, q = _setup(O, pkg, dev)
    batch = 1024
    keys = ctx.random_keys(23, L)
    dkeys = [pkg.to_device(k, dev) for k in keys]
    a, b = _operands(torch, q, batch, dev, 77)
    merged, three = _both_tails(plan, a, b, dkeys)
    assert torch.equal(merged, three), "merged tail differs from the three-launch tail"
    del three
    items = sorted({0, 1, 7, 512, 1023, 2, 3, 4, 5} | {129 * r for r in range(8)})      # 129 r = r (mod 8)
    _check_items(pkg, ctx, keys, a, b, merged, items)


def test_wide_prime_chain_keeps_the_three_launches(O, pkg, dev):
    """a chain with a 60-bit prime is not all-FP64: it keeps the separate launches (per modulus class) and still equals the oracle, with and without
    TROYN_MRR_SMALL=0"""
    import torch
    bits = [60, 50, 50, 50, 50, 60]
    ctx, plan, q = _setup(O, pkg, dev, bits)
    batch = 24
    keys = ctx.random_keys(25, L)
    dkeys = [pkg.to_device(k, dev) for k in keys]
    a, b = _operands(torch, q, batch, dev, 5)
    merged, three = _both_tails(plan, a, b, dkeys)
    assert torch.equal(merged, three)
    _check_items(pkg, ctx, keys, a, b, merged, [0, 1, 2, 3, 4, 5, 7, 12, 23])
