"""tests/scheme_boundary_spec.py is the contract, and its input builders build what they claim: the specification against the oracle wherever
the oracle has the function, against the reference's own known answers (tests/golden/ref_kats.json), bfv_scale_up against what BFV encryption adds
to c0 (the oracle has no scale_up of its own), exact rounding away from the boundary, and the conditions the GPU tests rely on (half-integer double
sums with both outcomes, a non-zero high word in the scale-up quotient, t above / a multiple of q_l, q_last = 1 mod t).  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import scheme_boundary_spec as S

N = 64
KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kats.json")))["rns_tool"]


def _chain(O, bits, n=N):
    return [int(v) for v in O.coeff_modulus_create(n, list(bits))]


def _uniform(O, seed, q, n=N):
    return np.stack([O.fill_uniform(seed * 131 + j, int(qj), n) for j, qj in enumerate(q)])


def _ints(a):
    return [int(v) for v in np.asarray(a).reshape(-1)]


def test_parameter_moduli_are_what_their_names_say():
    ts = S.scale_up_plain_moduli()
    assert S.is_prime((1 << 40) - 87) and S.prev_prime(1 << 40) == (1 << 40) - 87
    assert S.is_prime(ts[6]) and ts[6] < (1 << 59) and S.is_prime(ts[7]) and (1 << 60) < ts[7] < (1 << 61)
    assert S.is_prime(S.prev_prime(1 << 49)) and S.prev_prime(1 << 49) >> 48 == 1


@pytest.mark.parametrize("bits", S.SCALE_UP_CHAINS, ids=str)
def test_decrypt_scale_and_round_against_the_oracle(O, bits):
    """every plain modulus of the list at every level, on uniform phases and on round_boundaries (the oracle accepts all of them: gamma is an odd
    61-bit prime = 1 mod 2N and no t of the list shares a factor with it or with Q)"""
    q = _chain(O, bits)
    for t in S.scale_up_plain_moduli():
        ctx = O.Context("bfv", N, q, t)
        for L in range(len(q), 0, -1):
            gamma = int(O.lib().orc_rns_tool_gamma(ctx.rns_tool(L)))
            assert math.gcd(gamma, t) == 1
            edges = S.residue_rows(S.round_boundaries(q[:L], t, S.SEED), q[:L])
            for phase in (_uniform(O, 3 + L, q[:L]), S.tile_columns(edges, N, _uniform(O, 7, q[:L])), S.tile_columns(edges[:, N:], N, _uniform(O, 9, q[:L]))):
                assert S.bfv_decrypt_scale_and_round(phase, q[:L], t, gamma) == _ints(ctx.decrypt_scale_and_round(L, phase)), (t, L)


@pytest.mark.parametrize("bits", S.DECRYPT_MOD_T_CHAINS, ids=str)
def test_decrypt_mod_t_against_the_oracle(O, bits):
    q = _chain(O, bits)
    for t in S.decrypt_mod_t_plain_moduli():
        ctx = O.Context("bgv", N, q, t)
        for L in range(1, len(q) + 1):
            phases = [_uniform(O, 11 + L, q[:L])]
            if L in (2, 3):
                phases.append(S.half_integer_phases(q[:L], S.SEED, N))
            for phase in phases:
                assert S.bgv_decrypt_mod_t(phase, q[:L], t) == _ints(ctx.decrypt_mod_t(L, phase)), (t, L)


@pytest.mark.parametrize("bits", S.BGV_CHAINS, ids=str)
def test_bgv_mod_switch_against_the_oracle(O, bits):
    """through the oracle's transforms: coefficient form -> NTT -> mod_t_and_divide_q_last_ntt -> coefficient form.  Levels at which q_last has no
    inverse mod t are left out on both sides (the oracle would go on with an inverse of 1, the specification raises)"""
    q = _chain(O, bits)
    for t in S.bgv_plain_moduli(N):
        ctx = O.Context("bgv", N, q, t)
        for L in range(len(q), 1, -1):
            if math.gcd(q[L - 1] % t, t) != 1:
                with pytest.raises(ValueError):
                    S.bgv_mod_t_and_divide_q_last(_uniform(O, 1, q[:L]), q[:L], t)
                continue
            for x in (_uniform(O, 21 + L, q[:L]), S.tile_columns(S.bgv_last_limb_edges(q[:L], t, S.SEED), N, _uniform(O, 23, q[:L]))):
                got = ctx.from_ntt(ctx.mod_t_and_divide_q_last_ntt(L, ctx.to_ntt(x[None], 1, L)), 1, L - 1)[0]
                assert np.array_equal(S.bgv_mod_t_and_divide_q_last(x, q[:L], t), got), (t, L)
            assert (pow(q[L - 1], -1, t) == 1) == (q[L - 1] % t == 1)


@pytest.mark.parametrize("bits", S.DIVIDE_CHAINS, ids=str)
def test_bfv_divide_and_round_and_drop_against_the_oracle(O, bits):
    q = _chain(O, bits)
    ctx = O.Context("bfv", N, q, 65537)
    for L in range(len(q), 1, -1):
        for x in (_uniform(O, 31 + L, q[:L]), S.tile_columns(S.residue_rows(S.divide_edges(q[:L]), q[:L]), N, _uniform(O, 33, q[:L]))):
            assert np.array_equal(S.divide_and_round_q_last(x, q[:L]), ctx.mod_switch_scale_to_next(L, x[None])[0]), L
            assert np.array_equal(S.mod_switch_drop(x, L - 1), ctx.mod_switch_drop_to_next(L, x[None])[0]), L


@pytest.mark.parametrize("bits", S.CENTRALIZE_CHAINS, ids=str)
def test_plain_centralize_against_the_oracle(O, bits):
    """The oracle has the fast plain lift only and refuses a level with t >= some q_l; there the specification stands alone:
    {30,30,30} with every t of its list (a 40-bit prime, 2 q_0, q_1, 2^45) at every level; {60,40,40,60} with t = 2^59 at L >= 2."""
    q = _chain(O, bits)
    alone = []
    for t in S.centralize_plain_moduli(bits, q):
        ctx = O.Context("bfv", N, q, t)
        m = O.fill_uniform(5, t, N)
        m[:5] = [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2]
        for L in range(1, len(q) + 1):
            want = S.plain_centralize(m, q[:L], t)
            if any(t >= v for v in q[:L]):
                with pytest.raises(ValueError):
                    ctx.plain_centralize(L, m)
                alone.append((t, L))
                lifted = [int(v) - t if int(v) >= (t + 1) // 2 else int(v) for v in m]
                assert all(-(t // 2) <= v <= t // 2 for v in lifted)
                for l in range(L):
                    assert [v % q[l] for v in lifted] == _ints(want[l])
            else:
                assert np.array_equal(want, ctx.plain_centralize(L, m)), (t, L)
    assert len(alone) == (12 if list(bits) == [30, 30, 30] else 3)


def test_reference_known_answers():
    """test/utils/rns_tool.cu through tests/golden/ref_kats.json; gamma of a bare tool at poly_modulus_degree 2 is the second 61-bit prime = 1 mod 4"""
    for c in KATS["decrypt_scale_and_round"]:
        assert S.bfv_decrypt_scale_and_round(np.array(c["input"], dtype=np.uint64).reshape(len(c["q"]), 2), c["q"], c["t"], _kat_gamma()) == c["output"]
    for c in KATS["mod_t_and_divide_q_last_inplace"]:
        L = len(c["q"])
        x = np.array(c["input"], dtype=np.uint64).reshape(L, 2)
        x = np.stack([x[j] % np.uint64(c["q"][j]) for j in range(L)])
        assert _ints(S.bgv_mod_t_and_divide_q_last(x, c["q"], c["t"])) == c["output"]
    for c in KATS["decrypt_mod_t"]:
        assert S.bgv_decrypt_mod_t(np.array(c["input"], dtype=np.uint64).reshape(len(c["q"]), 2), c["q"], c["t"]) == c["output"]


def _kat_gamma():
    return [v for v in range((1 << 61) - 1, (1 << 61) - 2000, -1) if v % 4 == 1 and S.is_prime(v)][1]


def test_known_answer_gamma_is_the_oracles(O):
    assert O.RNSTool(2, [5, 7], 3).gamma == _kat_gamma()


@pytest.mark.parametrize("bits", S.SCALE_UP_CHAINS, ids=str)
def test_scale_up_is_what_bfv_encryption_adds(O, bits):
    """encrypt_asymmetric_bfv(m) - encrypt_asymmetric_bfv(0) under the same generator state: c1 is the same and c0 differs by bfv_scale_up(m)"""
    q = _chain(O, list(bits) + [bits[0]])            # the data level and a special prime
    L = len(bits)
    for t in S.scale_up_plain_moduli():
        ctx = O.Context("bfv", N, q, t)
        rng = O.Rng(77)
        pk = ctx.public_key(rng, ctx.secret_key(rng))
        edges = S.scale_up_edges(q[:L], t, S.SEED)
        m = O.fill_uniform(9, t, N)
        m[:len(edges)] = edges[:N]
        zero = ctx.encrypt_asymmetric_bfv(O.Rng(5), pk, np.zeros(N, dtype=np.uint64))
        ct = ctx.encrypt_asymmetric_bfv(O.Rng(5), pk, m)
        assert np.array_equal(ct[1], zero[1])
        assert np.array_equal(ct[0], S.bfv_scale_up(m, q[:L], t, src=zero[0])), t
        assert np.array_equal(zero[0], S.bfv_scale_up(m, q[:L], t, src=ct[0], subtract=True)), t
        short = S.bfv_scale_up(m[:N - 7], q[:L], t, n=N)
        assert not short[:, N - 7:].any() and np.array_equal(short[:, :N - 7], S.bfv_scale_up(m, q[:L], t)[:, :N - 7])


@pytest.mark.parametrize("bits", S.SCALE_UP_CHAINS, ids=str)
def test_exact_rounding_away_from_the_boundary(O, bits):
    """decrypt_scale_and_round(scale_up(m) + e) = m = true_round for |e| <= Q // (4t), both ends included (levels with Q < 4t have no room for
    noise and are left out: the 30-bit chain at L = 1 under the wide t, ...)"""
    q = _chain(O, bits)
    checked = 0
    for t in S.scale_up_plain_moduli():
        ctx = O.Context("bfv", N, q, t)
        for L in range(len(q), 0, -1):
            Q = S.product(q[:L])
            bound = Q // (4 * t)
            if bound == 0:
                continue
            gamma = int(O.lib().orc_rns_tool_gamma(ctx.rns_tool(L)))
            m = S.scale_up_inputs(q[:L], t, S.SEED, _ints(O.fill_uniform(13, t, N)))
            x = S.noisy_scale_ups(m, q[:L], t)
            assert S.bfv_decrypt_scale_and_round(S.residue_rows(x, q[:L]), q[:L], t, gamma) == m, (t, L)
            assert [S.true_round(v, Q, t) for v in x] == m, (t, L)
            checked += 1
    assert checked >= 8


@pytest.mark.parametrize("bits", S.SCALE_UP_CHAINS, ids=str)
def test_round_boundaries_hold_both_neighbours(O, bits):
    """next to t x / Q = k + 1/2 the gamma correction may differ from true_round (the GPU is compared with the algorithm there): only the inputs are checked"""
    q = _chain(O, bits)
    for t in S.scale_up_plain_moduli():
        for L in range(len(q), 0, -1):
            Q = S.product(q[:L])
            xs = S.round_boundaries(q[:L], t, S.SEED)
            assert len(xs) == 69 and all(0 <= v < Q for v in xs) and xs[64:] == [0, 1 % Q, Q - 1, Q // 2, (Q // 2 + 1) % Q]
            if Q < t:
                continue
            for i, k in enumerate(S.round_boundary_ks(t, S.SEED)):
                assert S.true_round(xs[2 * i], Q, t) == (k + 1) % t and S.true_round(xs[2 * i + 1], Q, t) == k, (t, L, k)


@pytest.mark.parametrize("bits", S.DECRYPT_MOD_T_CHAINS, ids=str)
@pytest.mark.parametrize("n", [N, 512, 1024])
def test_half_integer_phases_are_half_integers(O, bits, n):
    """every coefficient: exactly k + 1/2 + d / (2Q), and a double sum within 2 ulp of k + 1/2.  Both outcomes of the rounding occur in every
    parameter set (a chain at one ring size, L = 2 and 3 together).  With two 40-bit primes the double sum is ALWAYS exactly k + 1/2 (y_i < 2^53
    converts exactly, each quotient is off by at most half an ulp, and their sum is then at most a tie away from k + 1/2, which is the even
    neighbour): a tie, so those coefficients pin the rounding of halves away from zero, and only the sets with three primes or 60-bit primes
    have sums on both sides."""
    outcomes = set()
    for L in (2, 3):
        q = _chain(O, bits, n)[:L]
        Q = S.product(q)
        ph = S.half_integer_phases(q, S.SEED)
        assert ph.shape == (L, 64)
        for c in range(ph.shape[1]):
            y = S.bgv_fast_conversion_terms(ph[:, c], q)
            total = sum(yi * (Q // qi) for yi, qi in zip(y, q))
            k, rest = divmod(total, Q)
            d = 2 * rest - Q
            assert d % 2 != 0 and abs(d) < (1 << 20) and (c > 1 or d == (1, -1)[c])                  # exactly k + 1/2 + d / (2Q)
            v = S.bgv_double_sum(y, q)
            assert abs(v - (k + 0.5)) <= 2 * math.ulp(k + 0.5), (c, v)
            outcomes.add(S.round_half_away(v) - k)
            if list(bits) == [40, 40, 40] and L == 2:
                assert v == k + 0.5
    assert outcomes == {0, 1}                                                                     # both k and k + 1 occur


@pytest.mark.parametrize("bits", S.SCALE_UP_CHAINS, ids=str)
def test_scale_up_edges_reach_the_high_word(O, bits):
    q = _chain(O, bits)
    for n in (N, 1024):
        q = _chain(O, bits, n)
        for t in S.scale_up_plain_moduli():
            edges = S.scale_up_edges(q, t, S.SEED)
            assert all(0 <= v < t for v in edges) and {0, 1 % t, t - 1, (t - 1) // 2, (t + 1) // 2} <= set(edges)
            r, h = S.product(q) % t, (t + 1) // 2
            if math.gcd(r, t) == 1:
                assert {(v * r + h) % t for v in edges} >= {0, 1 % t, t - 1}
            if t >= (1 << 40) - 87:
                assert any((v * r + h) >> 64 for v in edges), t


def test_centralize_and_bgv_sets_take_every_branch(O):
    for n in (N, 512, 1024):
        kinds = set()
        for bits in S.CENTRALIZE_CHAINS:
            q = _chain(O, bits, n)
            for t in S.centralize_plain_moduli(bits, q):
                for ql in q:
                    kinds.add("below" if t < ql else "multiple" if t % ql == 0 else "above")
        assert kinds == {"below", "multiple", "above"}
        one, other = 0, 0
        for bits in S.BGV_CHAINS:
            q = _chain(O, bits, n)
            for t in S.bgv_plain_moduli(n):
                for L in range(2, len(q) + 1):
                    if math.gcd(q[L - 1], t) == 1:
                        one += q[L - 1] % t == 1
                        other += q[L - 1] % t != 1
        assert one and other
        assert all(v % (2 * n) == 1 for bits in S.BGV_CHAINS for v in _chain(O, bits, n))
