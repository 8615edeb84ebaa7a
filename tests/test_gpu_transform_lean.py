"""The lean FP64 transform body of the fused multiply -> relinearize -> rescale chain at N = 16384 (csrc/ntt_kernels.hpp: the rows handed over inside
mrr_tail_kernel as centred representatives, a1 (.) b1 entering its inverse transform without a re-centring, digits stored as doubles without the u64
round trip, TAIL_RESCALE's outputs re-centred once).  Every stored word must equal the CPU oracle's (ckks_multiply -> relinearize ->
mod_switch_scale_to_next), never the code under test's own other form -- the three-launch form (TROYN_MRR_SMALL=0) is checked against the oracle too.
Shapes: the smallest batch that takes MULPAIR + mrr_tail_kernel (one above the largest small launch, csrc/launch.hpp is_small_launch) and the next odd
one; chains: the flagship 6 x 50-bit chain, the largest primes below 2^50 and chains with the smallest primes above 2^49 in the output-limb, dropped and
special positions (the ends of the growth bound: |c| / p is largest when the row's prime is large and the limb's prime small)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, LOG_N, L = 16384, 14, 5
SMALL_LP_FACTOR = 2      # csrc/launch.hpp TROYN_SMALL_LP_FACTOR: a launch of at most CUs / 2 limb-polynomials counts as small


def _is_prime(n):
    """deterministic Miller-Rabin below 2^64"""
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _smallest_primes(count):
    """the smallest primes above 2^49 that are 1 modulo 2N"""
    out, c = [], (1 << 49) // (2 * N) * (2 * N) + 1
    while len(out) < count:
        if c > (1 << 49) and _is_prime(c):
            out.append(c)
        c += 2 * N
    return out


def _chain(O, name):
    if name == "flagship":
        return O.coeff_modulus_create(N, [50] * 6)
    big = O.get_primes(2 * N, 50, 6)          # the largest primes below 2^50, descending
    assert all((1 << 49) < p < (1 << 50) for p in big) and big[0] == max(big)
    assert not any(_is_prime(c) for c in range(big[0] + 2 * N, 1 << 50, 2 * N)), "get_primes starts at the largest prime below 2^50"
    small = _smallest_primes(2)
    if name == "largest":
        return big
    if name == "small-limb":              # output limb 0 smallest; dropped limb and special prime the largest
        return [small[0], big[2], big[3], big[4], big[1], big[0]]
    if name == "small-rows":              # dropped limb and special prime the smallest; output limbs the largest
        return [big[0], big[1], big[2], big[3], small[1], small[0]]
    raise KeyError(name)


def _smallest_merged_batch(dev):
    """small_tail_wanted (csrc/troyn.hip): batch * 2 * (L - 1) limb-polynomials * TROYN_SMALL_LP_FACTOR <= CUs is a small launch; one more is not"""
    import torch
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return max(1, cus // (SMALL_LP_FACTOR * 2 * (L - 1))) + 1


def _operands(torch, q, batch, dev, seed):
    """[batch][2][L][N] uniform residues; worst-case words in the first items (in the manner of test_gpu_corners): item 0 a and b all q - 1, item 1 a all 0,
    item 2 b all 0, item 3 a alternating 0 / q - 1 against b all q - 1, item 4 a and b the floor(q / 2), floor(q / 2) + 1 pattern, item 5 a that pattern
    against a uniform b, item 6 a all q - 1 against b all 1"""
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
    half = torch.tensor([int(v) // 2 for v in q[:L]], dtype=torch.int64, device=dev)[None, :, None]
    odd = (torch.arange(N, device=dev) & 1)[None, None, :]
    a[0], b[0] = top, top
    a[1] = 0
    b[2] = 0
    a[3], b[3] = top * odd, top
    a[4], b[4] = half + odd, half + (1 - odd)
    a[5] = half + odd
    a[6], b[6] = top, 1
    return a, b


_REFERENCE = {}      # (chain, batch) -> operands, keys and the oracle's words, computed once and shared by the forms


def _reference(O, pkg, dev, chain, batch):
    import torch
    key = (chain, batch)
    if key not in _REFERENCE:
        q = _chain(O, chain)
        ctx = O.Context("ckks", N, q)
        keys = ctx.random_keys(31 + batch, L)
        a, b = _operands(torch, q, batch, dev, 500 + batch)
        ah, bh = pkg.to_host(a), pkg.to_host(b)
        want = np.stack([ctx.mod_switch_scale_to_next(L, ctx.relinearize(L, True, ctx.ckks_multiply(L, ah[i], bh[i]), keys)) for i in range(batch)])
        want.setflags(write=False)
        _REFERENCE[key] = (q, keys, a, b, want)
    return _REFERENCE[key]


def _run(pkg, dev, q, keys, a, b, three_launches):
    plan = pkg.Plan(dev, LOG_N, q)
    dkeys = [pkg.to_device(k, dev) for k in keys]
    if three_launches:
        plan.set_option("TROYN_MRR_SMALL", "0")
    try:
        return pkg.to_host(plan.ckks_multiply_relinearize_rescale(L, a, b, dkeys))
    finally:
        if three_launches:
            plan.set_option("TROYN_MRR_SMALL", None)


def _assert_every_item(got, want):
    assert got.shape == want.shape
    for i in range(want.shape[0]):
        assert np.array_equal(got[i], want[i]), "item %d differs from the oracle" % i


@pytest.mark.parametrize("three_launches", [False, True], ids=["merged", "three-launches"])
@pytest.mark.parametrize("extra", [0, 2], ids=["smallest", "odd-above"])
def test_flagship_chain_smallest_merged_batches(O, pkg, dev, extra, three_launches):
    """MULPAIR + mrr_tail_kernel at its smallest batch and the next odd one, and the three launches that share the body: every item, worst-case words included"""
    batch = _smallest_merged_batch(dev) + extra
    assert batch != 1024 and batch >= 7
    q, keys, a, b, want = _reference(O, pkg, dev, "flagship", batch)
    a0 = a.clone()
    _assert_every_item(_run(pkg, dev, q, keys, a, b, three_launches), want)
    import torch
    assert torch.equal(a, a0), "operands were written"


@pytest.mark.parametrize("three_launches", [False, True], ids=["merged", "three-launches"])
@pytest.mark.parametrize("chain", ["largest", "small-limb", "small-rows"])
def test_extreme_primes(O, pkg, dev, chain, three_launches):
    """the ends of the growth bound: the largest primes below 2^50, and the smallest primes above 2^49 as an output limb under the largest special and
    dropped primes, and the other way round"""
    batch = _smallest_merged_batch(dev)
    q, keys, a, b, want = _reference(O, pkg, dev, chain, batch)
    _assert_every_item(_run(pkg, dev, q, keys, a, b, three_launches), want)


def test_separate_calls_keep_their_words(O, pkg, dev):
    """the instantiations outside the fused chain that share ntt_pass_body: dyadic product -> relinearize -> divide_and_round_q_last_ntt as three calls, and
    the plain forward and inverse transforms out of place, at N = 16384 on the flagship chain"""
    import torch
    batch = 7
    q, keys, a, b, want = _reference(O, pkg, dev, "flagship", _smallest_merged_batch(dev))
    a, b, want = a[:batch], b[:batch], want[:batch]
    plan = pkg.Plan(dev, LOG_N, q)
    dkeys = [pkg.to_device(k, dev) for k in keys]
    prod = plan.dyadic_convolute(a, 2, b, 2, L)
    relin = plan.relinearize(L, prod, dkeys, is_ckks=True, is_ntt_form=True)
    _assert_every_item(pkg.to_host(plan.divide_and_round_q_last_ntt(L, relin, 2)), want)
    # plain transforms, out of place: inverse then forward of the operands against the oracle's
    ctx = O.Context("ckks", N, q)
    x0 = a.clone()
    coeff = plan.ntt(a, 2, L, inverse=True, out=torch.empty_like(a))
    assert torch.equal(a, x0), "out-of-place inverse wrote its input"
    ch = pkg.to_host(coeff)
    for i in range(batch):
        assert np.array_equal(ch[i], ctx.from_ntt(pkg.to_host(a[i]), 2, L)), i
    back = plan.ntt(coeff, 2, L, inverse=False, out=torch.empty_like(a))
    bh = pkg.to_host(back)
    for i in range(batch):
        assert np.array_equal(bh[i], ctx.to_ntt(ch[i], 2, L)), i
