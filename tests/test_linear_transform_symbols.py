"""The diagonal encoder's entries exist in every layer (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_encode_diagonals_workspace_bytes", "troyn_ckks_encode_diagonals")


def test_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("Matrix diagonals encoded into BSGS weights"):text.index("size_t troyn_ckks_encode_diagonals_workspace_bytes")]
    for word in ("troyn_ckks_encode_simd", "is the specification", "count = N/2", "diags[a_t][(i - s_t) mod n]", "matrix[j][(j + a_t) mod n]", "s_t is masked", "a_t is clamped",
                 "TROYN_E_INVALID", "TROYN_E_WORKSPACE", "items == 0", "does not synchronise", "power of two"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_engine_has_the_wrapper(pkg):
    assert callable(getattr(pkg.CkksEncoder, "encode_diagonals"))


def test_the_source_is_a_selector_of_the_encoder_kernel():
    csrc = os.path.join(ROOT, "troy-nova_amd", "csrc")
    kernels = open(os.path.join(csrc, "ckks_kernels.hpp")).read()
    assert re.search(r"template <int LOGN, int TB, bool DEC, bool STRIDED, int SRC = CKKS_SRC_VALUES>\s*__global__[^\n]*ckks_fft_kernel", kernels)
    unit = open(os.path.join(csrc, "troyn_ckks.hip")).read()
    assert "CKKS_SRC_DIAGONALS" in unit and "CKKS_SRC_MATRIX" in unit
    assert "-ffp-contract=off" in open(os.path.join(csrc, "Makefile")).read()


def test_the_mirror_and_the_binding_name_the_methods():
    troy = os.path.join(ROOT, "troy-nova_amd", "troy")
    header = open(os.path.join(troy, "troy.h")).read()
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    for name in ("linear_transform", "linear_transform_new", "linear_transform_single_hoisted", "linear_transform_single_hoisted_new"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert '"%s"' % name in binder, name
    assert "ALREADY ROTATED BACK" not in header and "LinearTransform" in header
    own = open(os.path.join(troy, "linear_transform.h")).read()
    for name in ("class LinearTransform", "baby_steps", "giant_steps", "rotation_steps", "ADDITION to the reference's interface"):
        assert name in own, name
    assert '"LinearTransform"' in binder
    assert "ckks_encode_diagonals_step" in open(os.path.join(troy, "device_steps.h")).read()
    assert "linear_transform.cpp" in open(os.path.join(troy, "Makefile")).read()
