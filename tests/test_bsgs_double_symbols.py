"""The double-hoisted baby-step/giant-step transform exists in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_linear_transform_bsgs_double_hoisted_workspace_bytes", "troyn_linear_transform_bsgs_double_hoisted")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    # the block follows the single-hoisted entry, states the contract on integers, says that the words differ, and leaves BGV out
    start = text.index("The double-hoisted BSGS linear transform")
    assert start > text.index("int troyn_linear_transform_bsgs(")
    block = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("size_t troyn_linear_transform_bsgs_double_hoisted_workspace_bytes(")])
    for word in ("ADDITION", "X^(g)_c[m]", "the ONLY inner division, on component 1 alone", "the special one included",
                 "no division, no key", "ONE division for the transform", "The words are NOT those of troyn_linear_transform_bsgs",
                 "one rounding per giant step fewer", "TROYN_HOIST_EACH_GROUP", "BGV is left out", "TROYN_E_INVALID", "TROYN_E_WORKSPACE",
                 "batch == 0", "The tables are read before the call returns"):
        assert word in block, word
    # the single-hoisted block no longer sets the step aside: it points here
    single = re.sub(r"\s*\n \*\s*", " ", text[text.index("troyn_linear_transform_bsgs: out ="):text.index("#define TROYN_HOIST_EACH_GROUP")])
    assert "Out of scope" not in single and "troyn_linear_transform_bsgs_double_hoisted" in single


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name
    # the same argument lists as the single-hoisted entries
    for name in NAMES:
        assert pkg.capi.SYMBOLS[name] == pkg.capi.SYMBOLS[name.replace("_double_hoisted", "")], name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_plan_has_the_method(pkg):
    assert callable(getattr(pkg.Plan, "linear_transform_bsgs_double_hoisted"))
