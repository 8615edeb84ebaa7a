"""The ModRaise entries exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_mod_raise_workspace_bytes", "troyn_ckks_mod_raise")


def test_header_declares_the_entries_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("CKKS ModRaise"):text.index("size_t troyn_ckks_mod_raise_workspace_bytes")]
    for word in ("centred representative", "(-Q/2, Q/2]", "must not overlap", "TROYN_E_UNSUPPORTED", "TROYN_E_INVALID", "TROYN_E_WORKSPACE", "batch == 0",
                 "no entry synchronises", "word for word", "NTT o extend o INTT"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_the_kernel_has_a_unit_of_its_own():
    make = open(os.path.join(ROOT, "troy-nova_amd", "csrc", "Makefile")).read()
    assert "troyn_raise.hip" in make
    csrc = os.path.join(ROOT, "troy-nova_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "troyn_raise.hip")) and os.path.exists(os.path.join(csrc, "raise_kernels.hpp"))
    # ... and is not compiled into the encoder's unit
    assert "raise_kernels.hpp" not in open(os.path.join(csrc, "troyn_ckks.hip")).read()


def test_engine_has_the_wrapper(pkg):
    assert callable(getattr(pkg.CkksEncoder, "mod_raise"))


def test_the_mirror_and_the_binding_name_the_methods():
    header = open(os.path.join(ROOT, "troy-nova_amd", "troy", "troy.h")).read()
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    for name in ("mod_raise", "mod_raise_new", "mod_raise_inplace", "mod_raise_batched"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert '"%s"' % name in binder, name
    steps = open(os.path.join(ROOT, "troy-nova_amd", "troy", "device_steps.h")).read()
    assert "mod_raise_step" in steps
