"""The entries of the CKKS bootstrap (real / imaginary parts of slots, batched EvalMod, BootstrapPlan) exist in every layer (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_complex_split", "troyn_ckks_complex_join")


def test_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("Real and imaginary parts of CKKS slots"):text.index("int troyn_ckks_complex_split")]
    for word in ("generator 3", "i (-1)^j", "X^(N/2)", "no key switch, no level and no scale", "(-1)^j 2 Im w", "word for word", "troyn_add, troyn_sub and troyn_dyadic_product",
                 "transformed monomial", "q_l - iota_l", "tests/bootstrap_spec.py", "No workspace", "do not synchronise", "batch == 0", "TROYN_E_INVALID", "L == 0"):
        assert word in block, word


def test_binding_library_and_engine(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name
    assert callable(getattr(pkg.Plan, "ckks_complex_split")) and callable(getattr(pkg.Plan, "ckks_complex_join"))


def test_the_kernels_and_their_launches():
    csrc = os.path.join(ROOT, "troy-nova_amd", "csrc")
    kernels = open(os.path.join(csrc, "poly_kernels.hpp")).read()
    unit = open(os.path.join(csrc, "troyn.hip")).read()
    for name in ("ckks_complex_split_kernel", "ckks_complex_join_kernel"):
        assert re.search(r"__global__[^\n]*%s" % name, kernels), name
        assert re.search(r"hipLaunchKernelGGL\(%s" % name, unit), name
    usage = open(os.path.join(ROOT, "profiles", "bootstrap_resource_usage.txt")).read()
    for name in ("ckks_complex_split_kernel", "ckks_complex_join_kernel"):
        row = [line for line in usage.splitlines() if line.startswith(name)][0]
        assert row.split("/")[3].strip() == "0", "scratch must be 0: " + row


def test_the_mirror_and_the_binding_name_the_methods():
    troy = os.path.join(ROOT, "troy-nova_amd", "troy")
    header = open(os.path.join(troy, "troy.h")).read()
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    for name in ("split_real_imag", "split_real_imag_new", "join_real_imag", "join_real_imag_new", "eval_mod_batched", "eval_mod_new_batched",
                 "evaluate_chebyshev_batched", "evaluate_chebyshev_new_batched", "bootstrap", "bootstrap_new"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert '"%s"' % name in binder, name
    assert "(-1)^j 2 Im w" in header and "squares it" in header
    own = open(os.path.join(troy, "bootstrap.h")).read()
    for word in ("class BootstrapPlan", "levels()", "output_parms_id", "output_scale", "rotation_steps", "key_switches", "K - 1 >= ||I||_inf", "6.5 sqrt((N + 1) / 12)",
                 "2^-7", "Sparse packing", "sparse secrets", "c1 = q_w / (2 K s1)", "ADDITION to the reference's interface"):
        assert word in own, word
    assert '"BootstrapPlan"' in binder
    steps = open(os.path.join(troy, "device_steps.h")).read()
    assert "ckks_complex_split_step" in steps and "ckks_complex_join_step" in steps
    assert "bootstrap.cpp" in open(os.path.join(troy, "Makefile")).read()
    assert "bootstrap.h" in open(os.path.join(ROOT, "troy-nova_amd", "pybind", "Makefile")).read()
