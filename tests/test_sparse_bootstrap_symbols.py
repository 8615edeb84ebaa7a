"""The sparse-packing additions exist in every layer (no GPU needed): the sub-ring DFT factors, SubSum and the plans' n."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_dft_factor_diagonals_sparse_count", "troyn_ckks_dft_factor_diagonals_sparse")


def test_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("Factors of the special DFT on n slots"):text.index("size_t troyn_ckks_dft_factor_diagonals_sparse_count")]
    for word in ("2 <= n <= N/2", "tests/sparse_bootstrap_spec.py", "tests/dft_factors_spec.py", "root_powers", "no FMA", "ONE product", "[nd][n][2]", "TROYN_E_INVALID",
                 "count == 0", "No workspace", "n = N/2 the words are those of troyn_ckks_dft_factor_diagonals", "order 2"):
        assert word in block, word


def test_binding_library_and_engine(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name
    assert callable(getattr(pkg.CkksEncoder, "dft_factor_diagonals_sparse"))


def test_the_kernel_and_its_launch():
    csrc = os.path.join(ROOT, "troy-nova_amd", "csrc")
    kernels = open(os.path.join(csrc, "ckks_kernels.hpp")).read()
    assert re.search(r"__global__[^\n]*ckks_dft_factor_sparse_kernel", kernels) and re.search(r"__global__[^\n]*ckks_dft_factor_kernel", kernels)
    assert "launch_ckks_dft_factor_sparse" in open(os.path.join(csrc, "troyn_ckks.hip")).read()
    assert "launch_ckks_dft_factor_sparse" in open(os.path.join(csrc, "launch.hpp")).read()
    usage = open(os.path.join(ROOT, "profiles", "coeff_to_slot_resource_usage.txt")).read()
    assert "ckks_dft_factor_sparse_kernel" in usage


def test_the_mirror_and_the_binding_name_the_methods():
    troy = os.path.join(ROOT, "troy-nova_amd", "troy")
    header = open(os.path.join(troy, "troy.h")).read()
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    for name in ("sub_sum", "sub_sum_new", "sub_sum_steps", "sub_sum_stages"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert '"%s"' % name in binder, name
    assert 'py::arg("sub_sum_radix")' in binder and binder.count('py::arg("n") = 0') == 3
    assert "ckks_dft_factor_diagonals_sparse_step" in open(os.path.join(troy, "device_steps.h")).read()
    plans = open(os.path.join(troy, "slot_transform.h")).read()
    own = open(os.path.join(troy, "bootstrap.h")).read()
    for text in (plans, own):
        assert "size_t n = 0" in text and "out of scope" not in text and "not supported" not in text
    for word in ("Sparse packing.", "sub_sum_radix", "sub_sum_key_switches", "c1 = q_w / (2 K s1 s)", "||I'||_inf <= ||I||_inf", "would halve EvalMod"):
        assert word in own, word


def test_pytroy_signatures():
    """the binding's own documentation of the new arguments (importing pytroy needs no GPU)"""
    import sys
    pkg_dir = os.path.join(ROOT, "troy-nova_amd")
    if pkg_dir not in sys.path:
        sys.path.insert(0, pkg_dir)
    import torch  # noqa: F401  (first: one HIP runtime per process -- torch bundles its own libamdhip64)
    import pytroy
    assert re.search(r"\bn: [^,]* = 0, sub_sum_radix: [^,)]* = 0\)", pytroy.BootstrapPlan.__init__.__doc__)
    for cls in (pytroy.CoeffToSlotPlan, pytroy.SlotToCoeffPlan):
        assert re.search(r"\bn: [^,)]* = 0\)", cls.__init__.__doc__), cls
    assert pytroy.Evaluator.sub_sum_stages(512, 64, 4) == [[64, 128, 192], [256]] and pytroy.Evaluator.sub_sum_steps(512, 64, 2) == [64, 128, 256]
    assert pytroy.Evaluator.sub_sum_steps(512, 512) == []
