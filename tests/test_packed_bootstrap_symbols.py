"""The packed sparse bootstrap exists in every layer (no GPU needed): the packed DFT factors, the plans' `packed` and the device step."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_dft_factor_diagonals_packed_count", "troyn_ckks_dft_factor_diagonals_packed")


def test_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("both halves on period 2n"):text.index("size_t troyn_ckks_dft_factor_diagonals_packed_count")]
    for word in ("2 <= n <= N/4", "tests/packed_bootstrap_spec.py", "troyn_ckks_dft_factor_diagonals_sparse", "no FMA", "ONE product", "[nd][2n][2]", "TROYN_E_INVALID",
                 "count == 0", "No workspace", "-0.0", "(re, im) -> (im, -re)", "(re, im) -> (-im, re)", "v + conj(v)", "V + rot_n(V)", "n = 2n"):
        assert word in block, word
    # the entry takes no masks and no conjugate flag
    decl = re.search(r"int troyn_ckks_dft_factor_diagonals_packed\(([^)]*)\)", code).group(1)
    assert "mask" not in decl and "conjugate" not in decl and decl.count(",") == 7


def test_binding_library_and_engine(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name
    assert callable(getattr(pkg.CkksEncoder, "dft_factor_diagonals_packed"))


def test_the_kernel_and_its_launch():
    csrc = os.path.join(ROOT, "troy-nova_amd", "csrc")
    kernels = open(os.path.join(csrc, "ckks_kernels.hpp")).read()
    assert re.search(r"__global__[^\n]*ckks_dft_factor_packed_kernel", kernels) and re.search(r"__global__[^\n]*ckks_dft_factor_sparse_kernel", kernels)
    assert "launch_ckks_dft_factor_packed" in open(os.path.join(csrc, "troyn_ckks.hip")).read()
    assert "launch_ckks_dft_factor_packed" in open(os.path.join(csrc, "launch.hpp")).read()
    usage = open(os.path.join(ROOT, "profiles", "coeff_to_slot_resource_usage.txt")).read()
    assert "ckks_dft_factor_packed_kernel" in usage


def test_the_mirror_and_the_binding_name_the_argument():
    troy = os.path.join(ROOT, "troy-nova_amd", "troy")
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    assert binder.count('py::arg("packed")') == 3 and '"packed"' in binder and '"packed_group"' in binder
    assert "ckks_dft_factor_diagonals_packed_step" in open(os.path.join(troy, "device_steps.h")).read()
    assert re.search(r"\bdft_factor_diagonals_packed\s*\(", open(os.path.join(troy, "troy.h")).read())
    plans = open(os.path.join(troy, "slot_transform.h")).read()
    own = open(os.path.join(troy, "bootstrap.h")).read()
    for text in (plans, own):
        assert "bool packed = false" in text and "Not done" not in text
    assert plans.count("bool packed = false") == 2 and "bool packed() const" in plans and "bool packed() const" in own
    for word in ("Packed", "v + conj(v)", "rot_n(V)", "key_switches() is its count + 1", "ONE eval_mod operand"):
        assert word in own, word


def test_pytroy_signatures():
    """the binding's own documentation of the new argument (importing pytroy needs no GPU)"""
    import sys
    pkg_dir = os.path.join(ROOT, "troy-nova_amd")
    if pkg_dir not in sys.path:
        sys.path.insert(0, pkg_dir)
    import torch  # noqa: F401  (first: one HIP runtime per process -- torch bundles its own libamdhip64)
    import pytroy
    for cls in (pytroy.BootstrapPlan, pytroy.CoeffToSlotPlan, pytroy.SlotToCoeffPlan):
        assert re.search(r"\bpacked: bool\)", cls.__init__.__doc__), cls
        assert callable(cls.packed)
    assert callable(pytroy.CoeffToSlotPlan.packed_group)
