"""The sum over different ciphertexts and the baby-step/giant-step transform exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_apply_galois_sum_each_workspace_bytes", "troyn_apply_galois_sum_each",
         "troyn_linear_transform_bsgs_workspace_bytes", "troyn_linear_transform_bsgs")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"^#define TROYN_HOIST_EACH_GROUP \d+$", code, flags=re.M)
    # the block follows the weighted entry, says it is an addition, states both contracts, the pre-rotated weights, the bounded workspace,
    # what is out of scope, and leaves BGV out
    start = text.index("The sum of key-switched automorphisms of DIFFERENT ciphertexts")
    assert start > text.index("int troyn_apply_galois_weighted_sums(")
    block = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("#define TROYN_HOIST_EACH_GROUP")])      # the comment's line breaks do not matter
    assert "ADDITION" in block
    for word in ("one ciphertext PER TERM", "The element 1 IS allowed", "ONE rounded division by the special prime",
                 "the words equal troyn_apply_galois_sum's", "the plain sum", "TROYN_HOIST_EACH_GROUP", "does not grow",
                 "ALREADY ROTATED BACK", "rot_{-G_g}(diag_{g,b})", "followed by troyn_apply_galois_sum_each", "never visible",
                 "double hoisting", "BGV is left out", "TROYN_E_INVALID", "TROYN_E_WORKSPACE", "batch == 0", "giants == 0", "babies == 0",
                 "a giant step with no weight", "The tables are read before the call returns"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_plan_has_the_methods(pkg):
    assert callable(getattr(pkg.Plan, "apply_galois_sum_each"))
    assert callable(getattr(pkg.Plan, "linear_transform_bsgs"))
