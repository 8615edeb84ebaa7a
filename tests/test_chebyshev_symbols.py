"""The product-plus-affine step exists in every layer below the C++ mirror, and its header block states the contract (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes", "troyn_ckks_multiply_affine_relinearize_rescale")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    start = text.index("Product plus affine part, relinearized and rescaled")
    block = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("size_t troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(")])
    assert "ADDITION" in block
    for word in ("P_0 = alpha_i (a0 . b0) + w_i c0 + k_i", "P_1 = alpha_i (a0 . b1 + a1 . b0) + w_i c1", "P_2 = alpha_i (a1 . b1)",
                 "divide_and_round_q_last_ntt( relinearize( P ) )", "canonical form", "only the first L limbs are read", "or NULL", "w_i is ignored",
                 "`constant` may be NULL", "Contract on integers", "bit-identical to this sequence per item", "troyn_dyadic_convolute",
                 "troyn_multiply_scalar by alpha", "troyn_multiply_scalar and troyn_add of the addend", "troyn_relinearize",
                 "troyn_divide_and_round_q_last_ntt", "does not depend on where the reductions happen", "each word of a, b and c is read once",
                 "TROYN_E_INVALID", "L < 2", "a null table", "a null a[i] or b[i]", "a misaligned pointer", "c_nmod[i] < L",
                 "a scalar word >= its modulus", "overlapping an input", "TROYN_E_WORKSPACE", "batch == 0", "read before the call returns"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_plan_has_the_method(pkg):
    assert callable(getattr(pkg.Plan, "multiply_affine_relinearize_rescale"))


def test_kernel_is_built_and_its_resource_usage_is_recorded():
    text = open(os.path.join(ROOT, "troy-nova_amd", "csrc", "poly_kernels.hpp")).read()
    assert "void multiply_affine_kernel(" in text
    usage = open(os.path.join(ROOT, "profiles", "chebyshev_resource_usage.txt")).read()
    assert "multiply_affine_kernel" in usage and "ScratchSize [bytes/lane]: 0" in usage and "VGPRs Spill: 0" in usage


def test_mirror_header_states_the_contracts():
    text = open(os.path.join(ROOT, "troy-nova_amd", "troy", "troy.h")).read()
    start = text.index("the Chebyshev basis on a fused product-plus-affine step")
    block = re.sub(r"\s*\n\s*//\s*", " ", text[start:text.index("void multiply_affine_relinearize_rescale(", start)])
    for word in ("rescale_to_next(relinearize(alpha * e1 * e2 + gamma * addend + constant))", "non-zero signed integer",
                 "gamma * (S / addend.scale())", "rounded half away from zero", "2^62", "formed in 128 bits", "S / q_last, set exactly",
                 "may sit at a higher level", "SUM_m coefficients[m] T_m(x / K)", "costs no level", "T_i T_jk = (T_(jk+i) + T_(jk-i)) / 2",
                 "2 T_(m/2)^2 - 1", "2 T_a T_(m-a) - T_(2a-m)", "one batched call", "depth(T_m) = ceil(log2 m)", "Degrees up to 127",
                 "sin(2 pi x) / (2 pi)", "cos(2 pi (K y - 1/4) / 2^r)", "alpha = 2, no addend, constant -1", "depth(evaluate_chebyshev) + r"):
        assert word in block, word
    for name in ("multiply_affine_relinearize_rescale_new", "multiply_affine_relinearize_rescale_batched", "evaluate_chebyshev_new", "eval_mod_new"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    for name in ("multiply_affine_relinearize_rescale", "multiply_affine_relinearize_rescale_new", "multiply_affine_relinearize_rescale_batched",
                 "evaluate_chebyshev", "evaluate_chebyshev_new", "eval_mod", "eval_mod_new"):
        assert 'ev.def("%s"' % name in binder, name
