"""The BFV inner-product entries (sum of BEHZ tensor products, one scale-down) exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_bfv_multiply_accumulate_workspace_bytes",
         "troyn_bfv_multiply_accumulate",
         "troyn_bfv_multiply_accumulate_relinearize_workspace_bytes",
         "troyn_bfv_multiply_accumulate_relinearize")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("BFV inner product"):text.index("size_t troyn_bfv_multiply_accumulate_workspace_bytes(")]
    for cited in ("evaluator.cu:29-116", "evaluator_keyswitching.cu:119-144"):
        assert cited in block
    assert "ADDITIONS" in block and "bit-identical" in block
    assert "1024" in block                                      # the cap on the number of terms is part of the contract


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_behz_has_the_methods(pkg):
    assert callable(getattr(pkg.Behz, "bfv_multiply_accumulate"))
    assert callable(getattr(pkg.Behz, "bfv_multiply_accumulate_relinearize"))
