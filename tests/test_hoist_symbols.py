"""The hoisted-rotation entries (one digit decomposition for many Galois keys) exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_apply_galois_hoisted_workspace_bytes", "troyn_apply_galois_many", "troyn_apply_galois_sum")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    # the header says they are additions, that the words are not apply_galois's, and leaves BGV out
    block = text[text.index("Hoisted rotations"):text.index("size_t troyn_apply_galois_hoisted_workspace_bytes(")]
    assert "ADDITIONS" in block
    assert "NOT bit-identical to troyn_apply_galois + troyn_switch_key" in block and "words differ from apply_galois" in block
    assert "BGV is left out" in block
    for word in ("TROYN_E_INVALID", "TROYN_E_WORKSPACE", "batch == 0"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_plan_has_the_methods(pkg):
    assert callable(getattr(pkg.Plan, "apply_galois_many"))
    assert callable(getattr(pkg.Plan, "apply_galois_sum"))
