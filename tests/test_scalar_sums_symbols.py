"""The scalar-weighted sum of ciphertexts exists in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_scalar_weighted_sums_workspace_bytes", "troyn_scalar_weighted_sums")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    start = text.index("Scalar-weighted sums of ciphertexts")
    block = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("size_t troyn_scalar_weighted_sums_workspace_bytes(")])
    assert "ADDITION" in block
    for word in ("first nmod limbs", "Contract on integers", "c == 0 and (i == 0 or !constant_at_index0) ? constants[s][l] : 0", "canonical form",
                 "bit-identical to folding troyn_multiply_scalar and troyn_add", "does not depend on where the reductions happen",
                 "TROYN_E_INVALID", "terms == 0", "slots == 0", "pcount == 0", "a null table or entry", "a misaligned pointer", "in_nmod[t] < nmod",
                 "a modulus slice outside the plan", "a scalar or constant word >= its modulus", "`out` overlapping an input",
                 "TROYN_E_WORKSPACE", "batch == 0", "read before the call returns"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_plan_has_the_method(pkg):
    assert callable(getattr(pkg.Plan, "scalar_weighted_sums"))
