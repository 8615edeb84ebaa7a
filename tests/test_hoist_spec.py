"""The specification of the hoisted rotations (tests/hoist_spec.py) tied to what exists already, on the CPU:
  * with one term and the identity map in place of the automorphism it IS the key-switch specification (tests/ks_spec.py,
    OverwriteExceptFirst), so the two share the decomposition, the inner product and the rounded division;
  * with genuine Galois keys its outputs decrypt, through the oracle's BFV decryption, to exactly the plaintexts the oracle's own
    apply_galois results decrypt to (their sum modulo t for the sum form).  The words differ from the oracle's (include/troyn.h says why);
    the messages do not."""
import numpy as np

from hoist_spec import apply_galois_many_spec, apply_galois_sum_spec, sigma
from ks_spec import switch_key_spec
from test_keyswitch_spec import make_case


def test_sigma_is_the_reference_automorphism(O):
    """sigma on canonical residues (negations reduced modulo q) is GaloisTool::apply of the oracle, for elements that negate and 2N - 1"""
    n = 32
    q = O.coeff_modulus_create(n, [40, 40])
    ctx = O.Context("bfv", n, q, 257)
    x = ctx.random_ct(3, 1, 2)[0]
    for g in (3, 5, 25, 2 * n - 1):
        got = ctx.apply_galois(2, False, g, x[None])[0]
        for l in range(2):
            assert [v % q[l] for v in sigma([int(v) for v in x[l]], g)] == [int(v) for v in got[l]], (g, l)


def test_one_term_identity_map_is_the_key_switch_spec(O):
    for n, bits, L, order in ((32, [50, 50, 50, 50], 3, None), (32, [50, 50, 50], 2, "reversed")):
        q = O.coeff_modulus_create(n, bits)
        if order == "reversed":
            q = sorted(q, reverse=True)
        digits, keys, _, _ = make_case(O, n, q, L, 17 + L, True)
        rng = np.random.default_rng(4)
        c0 = [[int(v) for v in rng.integers(0, q[l], size=n, dtype=np.uint64)] for l in range(L)]
        got = apply_galois_sum_spec(q, L, c0, digits, [3], [keys], automorphism=lambda x, g: list(x))
        assert got == switch_key_spec(q, L, digits, keys, [c0, c0], 2)


def test_genuine_keys_decrypt_to_the_reference_plaintexts(O):
    n, t = 32, 257          # the smallest ring the oracle's batching BFV encrypt / decrypt accepts with this plain modulus
    q = [int(v) for v in O.coeff_modulus_create(n, [36, 36, 37])]
    K, L = len(q), len(q) - 1
    ctx = O.Context("bfv", n, q, t)
    rng = O.Rng(21)
    sk = ctx.secret_key(rng)
    pk = ctx.public_key(rng, sk)
    ct = ctx.encrypt_asymmetric_bfv(rng, pk, ctx.batch_encode(list(range(1, n + 1))))
    elements = [3, 2 * n - 1]
    keys_ntt = [ctx.galois_key(rng, sk, g) for g in elements]
    # keys to coefficient form under all K moduli (the oracle's transform, pinned to the by-definition one in test_keyswitch_spec.py)
    keys_c = [[[[[int(v) for v in row] for row in ctx.from_ntt(kj[c][None], 1, K)[0]] for c in range(2)] for kj in keys_ntt[i]] for i in range(len(elements))]
    want = [ctx.decrypt_bfv(sk, ctx.apply_galois_ct(L, False, g, ct, keys_ntt[i])) for i, g in enumerate(elements)]
    assert not np.array_equal(want[0], want[1])
    c0 = [[int(v) for v in ct[0][l]] for l in range(L)]
    c1 = [[int(v) for v in ct[1][l]] for l in range(L)]
    many = apply_galois_many_spec(q, L, c0, c1, elements, keys_c)
    for i in range(len(elements)):
        got = np.array(many[i], dtype=np.uint64)
        assert np.array_equal(ctx.decrypt_bfv(sk, got), want[i]), elements[i]
        # ... and the words are indeed not the reference's: the contract is the specification
        assert not np.array_equal(got, ctx.apply_galois_ct(L, False, elements[i], ct, keys_ntt[i]))
    summed = np.array(apply_galois_sum_spec(q, L, c0, c1, elements, keys_c), dtype=np.uint64)
    assert np.array_equal(ctx.decrypt_bfv(sk, summed), (want[0] + want[1]) % np.uint64(t))
