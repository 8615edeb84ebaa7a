"""What the four `create` calls refuse (error class, code and message text), that a refused create leaves the plan usable, and the size of the
auxiliary base a BEHZ handle works in.  The messages quote the reference's (utils/rns_tool.cu, modulus.h, app/bfv_ring2k.cu) where it has one.
Everything but the construction of the N = 32768 handle runs at N = 4096."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_N, N = 12, 4096
E_INVALID, E_MODULUS = -1, -2
T_PLAIN = 65537


@pytest.fixture(scope="module")
def chain(O):
    return O.coeff_modulus_create(N, [40, 40, 40])


@pytest.fixture(scope="module")
def plan(pkg, dev, chain):
    return pkg.Plan(dev, LOG_N, chain)


def _refused(pkg, code, text, create):
    with pytest.raises(pkg.capi.TroynInvalidArgument) as e:
        create()
    assert str(e.value) == "%s (troyn code %d)" % (text, code)


def _still_works(pkg, dev, plan, make_handle):
    """after a refusal: one small successful create and one add on the same plan"""
    make_handle().close()
    rng = np.random.default_rng(5)
    a = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in plan.moduli])
    b = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in plan.moduli])
    got = pkg.to_host(plan.add(pkg.to_device(a, dev), pkg.to_device(b, dev), plan.K))
    want = (a + b) % np.array(plan.moduli, dtype=np.uint64)[:, None]
    assert np.array_equal(got.reshape(want.shape).astype(np.uint64), want)


def _plan_create(pkg, log_n, moduli, count=None):
    """troyn_plan_create itself: a count of 0 or 65 is refused before the array is read"""
    arr = (C.c_uint64 * max(len(moduli), 1))(*moduli)
    h = C.c_void_p()
    pkg.capi.check(pkg.capi.lib().troyn_plan_create(C.byref(h), 0, log_n, len(moduli) if count is None else count, arr, None))
    pkg.capi.lib().troyn_plan_destroy(h)


@pytest.mark.parametrize("case", ["log_n_0", "log_n_18", "no_moduli", "65_moduli", "modulus_1", "modulus_2^61", "repeated", "no_root"])
def test_plan_create_refusals(pkg, dev, chain, case):
    degree, count, set_value = ("[troyn_plan_create] Invalid poly_modulus_degree.", "[troyn_plan_create] Invalid coeff modulus count.",
                                "[Modulus::set_value] Value can be at most 61-bit and cannot be 1.")
    code, text, args = {
        "log_n_0": (E_INVALID, degree, (0, chain)),
        "log_n_18": (E_INVALID, degree, (18, chain)),
        "no_moduli": (E_INVALID, count, (LOG_N, chain, 0)),
        "65_moduli": (E_INVALID, count, (LOG_N, chain, 65)),
        "modulus_1": (E_MODULUS, set_value, (LOG_N, [chain[0], 1])),
        "modulus_2^61": (E_MODULUS, set_value, (LOG_N, [chain[0], 1 << 61])),
        "repeated": (E_MODULUS, "[troyn_plan_create] coeff_modulus must be pairwise coprime.", (LOG_N, [chain[0], chain[1], chain[0]])),
        "no_root": (E_MODULUS, "[troyn::make_ntt_table] Invalid modulus, unable to find primitive root.", (LOG_N, [chain[0], 1000003])),   # 1000002 = 2 * 3 * 166667
    }[case]
    _refused(pkg, code, text, lambda: _plan_create(pkg, *args))
    small = pkg.Plan(dev, LOG_N, chain[:1])
    _still_works(pkg, dev, small, lambda: pkg.Bgv(small, 1, T_PLAIN))


@pytest.mark.parametrize("scheme", ["behz", "bgv"])
@pytest.mark.parametrize("case", ["L_0", "L_K+1", "t_0", "t_1", "t_2^61"])
def test_behz_and_bgv_create_refusals(pkg, dev, plan, scheme, case):
    make = pkg.Behz if scheme == "behz" else pkg.Bgv
    length = (E_INVALID, "[RNSTool::RNSTool] RNSBase length is invalid.")
    modulus = (E_MODULUS, "[troyn_behz_create] BFV needs a plain modulus in [2, 2^61)." if scheme == "behz" else "[troyn_bgv_create] BGV needs a plain modulus in [2, 2^61).")
    (code, text), L, t = {"L_0": (length, 0, T_PLAIN), "L_K+1": (length, plan.K + 1, T_PLAIN),
                          "t_0": (modulus, 2, 0), "t_1": (modulus, 2, 1), "t_2^61": (modulus, 2, 1 << 61)}[case]
    _refused(pkg, code, text, lambda: make(plan, L, t))
    _still_works(pkg, dev, plan, lambda: make(plan, 2, T_PLAIN))


@pytest.mark.parametrize("case", ["L_0", "L_K+1", "elem_bytes_3", "t_bits_half_32", "t_bits_above_32", "t_bits_half_64", "t_bits_above_64"])
def test_ring2k_create_refusals(pkg, dev, plan, case):
    P = "[PolynomialEncoderRNSHelper::PolynomialEncoderRNSHelper]"
    count, elem, bits = P + " modulus count out of range", P + " T must be uint32_t, uint64_t or uint128_t", P + " t_bit_length must be greater than type_bits<T>() / 2"
    text, L, t_bits, elem_bits = {"L_0": (count, 0, 20, 32), "L_K+1": (count, plan.K + 1, 20, 32), "elem_bytes_3": (elem, 2, 20, 24),
                                  "t_bits_half_32": (bits, 2, 16, 32), "t_bits_above_32": (bits, 2, 33, 32),
                                  "t_bits_half_64": (bits, 2, 32, 64), "t_bits_above_64": (bits, 2, 65, 64)}[case]
    _refused(pkg, E_INVALID, text, lambda: pkg.Ring2k(plan, L, t_bits, elem_bits))
    _still_works(pkg, dev, plan, lambda: pkg.Ring2k(plan, 2, 20, 32))


# (working_base_size, len(base_Bsk)) by chain and by what the plan was created under: what the library returned before troyn_behz_create was split into steps
# (the choice of base is host arithmetic).  The reference sizes B as |q| primes of 61 bits (+ m_sk) on all three chains; the working base differs only where
# every q_i is below 2^50, the second generation runs and the reference's base was not asked for: {40} x 2 with t of 17 bits needs more than
# 32 + 17 + 80 + 2 bits, which 2 + 1 primes below 2^50 carry as well; {50} x 10 with t of 20 bits needs more than 554 bits: 11 + 1 such primes against 10 + 1 of 61 bits.
WORKING_BASE = {
    "4096_40x3": (4096, [40, 40, 40], T_PLAIN, {"default": (3, 3), "ref": (3, 3), "v1": (3, 3)}),
    "4096_60_40_40_60": (4096, [60, 40, 40, 60], T_PLAIN, {"default": (4, 4), "ref": (4, 4), "v1": (4, 4)}),
    "32768_50x11": (32768, [50] * 11, 1032193, {"default": (12, 11), "ref": (11, 11), "v1": (11, 11)}),
}


@pytest.mark.parametrize("env", ["default", "ref", "v1"])
@pytest.mark.parametrize("name", list(WORKING_BASE))
def test_working_base_size(O, pkg, dev, monkeypatch, name, env):
    n, bits, t, expected = WORKING_BASE[name]
    for k in ("TROYN_BEHZ", "TROYN_BEHZ_BASE"):
        monkeypatch.delenv(k, raising=False)
    if env == "ref":
        monkeypatch.setenv("TROYN_BEHZ_BASE", "ref")
    elif env == "v1":
        monkeypatch.setenv("TROYN_BEHZ", "v1")
    q = O.coeff_modulus_create(n, bits)
    p = pkg.Plan(dev, n.bit_length() - 1, q)
    behz = pkg.Behz(p, len(q) - 1, t)
    got = (behz.working_base_size, len(behz.base_Bsk))
    print("working base", name, env, got)
    assert got == expected[env]
