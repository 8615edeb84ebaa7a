"""The plaintext-weighted hoisted-rotation entries exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_apply_galois_weighted_workspace_bytes", "troyn_apply_galois_weighted_sums")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    # the block follows troyn_apply_galois_sum, says it is an addition, states the exactness argument of the two routes, that the words are
    # not the composed form's, and leaves BGV out
    start = text.index("Plaintext-weighted hoisted rotations")
    assert start > text.index("int troyn_apply_galois_sum(")
    block = text[start:text.index("size_t troyn_apply_galois_weighted_workspace_bytes(")]
    assert "ADDITION" in block
    assert "((X + q_special * y) - r) * q_special^-1 = (X - r) * q_special^-1 + y" in block
    assert "the words equal troyn_apply_galois_sum's" in block
    assert "NOT" in block and "troyn_apply_galois + troyn_switch_key" in block
    assert "BGV is left out" in block
    for word in ("TROYN_E_INVALID", "TROYN_E_WORKSPACE", "batch == 0", "slots == 0", "The element 1 IS allowed"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_plan_has_the_method(pkg):
    assert callable(getattr(pkg.Plan, "apply_galois_weighted_sums"))
