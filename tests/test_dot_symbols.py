"""The dot-product entries (sum of ciphertext products, one relinearize and rescale) exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_dyadic_convolute_accumulate",
         "troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes",
         "troyn_ckks_multiply_accumulate_relinearize_rescale")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    # the header says they are additions, names what they compose and states the contract
    for cited in ("evaluator.cu:118-145", "evaluator_keyswitching.cu:119-144", "utils/rns_tool.cu:499-694"):
        assert cited in text
    block = text[text.index("Dot product of ciphertexts"):text.index("int troyn_dyadic_convolute_accumulate(")]
    assert "ADDITIONS" in block and "bit-identical" in block


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_plan_has_the_methods(pkg):
    assert callable(getattr(pkg.Plan, "dyadic_convolute_accumulate"))
    assert callable(getattr(pkg.Plan, "ckks_multiply_accumulate_relinearize_rescale"))
