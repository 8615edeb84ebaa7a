"""The fused BGV chain (multiply -> relinearize -> mod-switch in one call) exists in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_bgv_multiply_relinearize_mod_switch_workspace_bytes",
         "troyn_bgv_multiply_relinearize_mod_switch")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("Fused BGV chain"):text.index("size_t troyn_bgv_multiply_relinearize_mod_switch_workspace_bytes(")]
    # the three calls the words equal
    for call in ("troyn_dyadic_convolute", "troyn_bgv_relinearize", "troyn_bgv_mod_t_and_divide_q_last_ntt"):
        assert call in block, call
    assert "word for word" in block and "ADDITION" in block
    # the refusals and the empty batch
    for word in ("TROYN_E_INVALID", "TROYN_E_MODULUS", "TROYN_E_WORKSPACE", "batch == 0 returns TROYN_OK", "misaligned", "overlapping",
                 "Unable to invert q[last] mod t", "does not synchronise"):
        assert word in block, word
    assert "troyn_bgv_inv_q_last_mod_t" in block               # the correction factor stays with the caller


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_bgv_has_the_method(pkg):
    assert callable(getattr(pkg.Bgv, "multiply_relinearize_mod_switch"))
