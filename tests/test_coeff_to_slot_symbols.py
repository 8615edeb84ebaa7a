"""The entries of the factored special DFT (CoeffToSlot / SlotToCoeff) exist in every layer (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_dft_factor_diagonals_count", "troyn_ckks_dft_factor_diagonals")


def test_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("Factors of the special DFT"):text.index("size_t troyn_ckks_dft_factor_diagonals_count")]
    for word in ("generator 3", "(-3)^j", "tests/dft_factors_spec.py", "troyn_ckks_get_tables", "root_powers", "no FMA", "ONE product", "[nd][n][2]", "col_mask / row_mask",
                 "TROYN_E_INVALID", "count == 0", "does not synchronise", "No workspace", "not finite", "unknown mask"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_engine_has_the_wrapper(pkg):
    assert callable(getattr(pkg.CkksEncoder, "dft_factor_diagonals"))


def test_the_kernel_and_its_launch():
    csrc = os.path.join(ROOT, "troy-nova_amd", "csrc")
    kernels = open(os.path.join(csrc, "ckks_kernels.hpp")).read()
    assert re.search(r"__global__[^\n]*ckks_dft_factor_kernel", kernels)
    assert "launch_ckks_dft_factor" in open(os.path.join(csrc, "troyn_ckks.hip")).read()
    assert "launch_ckks_dft_factor" in open(os.path.join(csrc, "launch.hpp")).read()
    assert "-ffp-contract=off" in open(os.path.join(csrc, "Makefile")).read()


def test_the_mirror_and_the_binding_name_the_methods():
    troy = os.path.join(ROOT, "troy-nova_amd", "troy")
    header = open(os.path.join(troy, "troy.h")).read()
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    for name in ("coeff_to_slot", "coeff_to_slot_new", "slot_to_coeff", "slot_to_coeff_new"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert '"%s"' % name in binder, name
    own = open(os.path.join(troy, "slot_transform.h")).read()
    for name in ("class CoeffToSlotPlan", "class SlotToCoeffPlan", "rotation_steps", "needs_conjugate", "layers_per_group", "baby_count for strided diagonals",
                 "Slot order of the result", "ADDITIONS to the reference's interface", "Sparse packing"):
        assert name in own, name
    assert '"CoeffToSlotPlan"' in binder and '"SlotToCoeffPlan"' in binder
    assert "ckks_dft_factor_diagonals_step" in open(os.path.join(troy, "device_steps.h")).read()
    assert "slot_transform.cpp" in open(os.path.join(troy, "Makefile")).read()
    assert "slot_transform.h" in open(os.path.join(ROOT, "troy-nova_amd", "pybind", "Makefile")).read()
