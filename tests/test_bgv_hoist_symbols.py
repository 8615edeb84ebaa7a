"""The hoisted BGV entries exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_bgv_apply_galois_many", "troyn_bgv_apply_galois_sum", "troyn_bgv_apply_galois_weighted_sums",
         "troyn_bgv_apply_galois_sum_each", "troyn_bgv_linear_transform_bsgs")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(\s*const troyn_bgv\* key_level" % name, code), name
    # the block follows troyn_bgv_relinearize and precedes the fused chain; it says it is an addition, states the division, that the words
    # are neither the composition's nor the reference's, what the BSGS entry equals, where the workspace sizes come from, and its refusals
    start = text.index("Hoisted BGV rotations")
    assert text.index("int troyn_bgv_relinearize(") < start < text.index("int troyn_bgv_apply_galois_many(") < text.index("Fused BGV chain")
    block = re.sub(r"\s*\n \*\s*", " ", text[start:text.index("int troyn_bgv_apply_galois_many(")])      # the comment's line breaks do not matter
    for word in ("ADDITIONS", "in place of `plan, is_ckks, is_ntt_form`", "as for troyn_bgv_switch_key", "Operands are in NTT form",
                 "KEY-LEVEL layout", "tests/bgv_hoist_spec.py", "the same signed hoisted digits", "the same injection of the unkeyed terms",
                 "exactly as in troyn_bgv_switch_key: result_c[l] = (X_c[q_l] - dk_l(s_c)) * q_special^-1 mod q_l",
                 "in coefficient form, canonical", "[-s * q_special^-1 mod t]_{q_l} * q_special + [s]_{q_l}",
                 "NEITHER troyn_apply_galois + troyn_bgv_switch_key NOR the reference",
                 "equal troyn_bgv_apply_galois_weighted_sums (slots = giants) followed by troyn_bgv_apply_galois_sum_each",
                 "is_ntt_form = 1", "troyn_apply_galois_hoisted_workspace_bytes", "troyn_apply_galois_weighted_workspace_bytes",
                 "troyn_apply_galois_sum_each_workspace_bytes", "troyn_linear_transform_bsgs_workspace_bytes",
                 "Unable to invert q[last] mod t", "TROYN_E_INVALID", "TROYN_E_WORKSPACE", "TROYN_E_MODULUS", "batch == 0",
                 "The tables are read before the call returns", "troyn_linear_transform_bsgs_double_hoisted has no BGV form"):
        assert word in block, word
    # the BFV/CKKS blocks keep their scope sentence and point here
    assert text.count("BGV is left out") == 4
    assert text.count("hoisted BGV block below") == 4 and "The hoisted BGV block below has no double-hoisted entry" in text


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name
        namesake = pkg.capi.SYMBOLS[name.replace("troyn_bgv_", "troyn_")]
        # the namesake's arguments with the handle in place of (plan, is_ckks, is_ntt_form)
        assert pkg.capi.SYMBOLS[name][1] == namesake[1][:2] + namesake[1][4:], name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_bgv_handle_has_the_methods(pkg):
    for name in ("apply_galois_many", "apply_galois_sum", "apply_galois_weighted_sums", "apply_galois_sum_each", "linear_transform_bsgs"):
        assert callable(getattr(pkg.Bgv, name)), name


def test_no_bgv_workspace_query_was_added(pkg):
    """the BGV entries size their workspaces with the plan's queries (is_ntt_form = 1): no troyn_bgv_* query of the hoisted family exists, and the
    plan's queries keep their argument lists.  (That their VALUES are those of the parent is shown on the device, where the BFV / CKKS tests
    of the family run against workspaces of exactly the queried size.)"""
    hoisted = ("galois", "linear_transform")
    assert not [n for n in pkg.capi.SYMBOLS if n.startswith("troyn_bgv_") and any(h in n for h in hoisted) and "workspace" in n]
    C = pkg.capi.C
    assert pkg.capi.SYMBOLS["troyn_apply_galois_hoisted_workspace_bytes"][1] == [C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int]
    for name in ("troyn_apply_galois_sum_each_workspace_bytes",):
        assert pkg.capi.SYMBOLS[name][1] == [C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int], name
    for name in ("troyn_apply_galois_weighted_workspace_bytes", "troyn_linear_transform_bsgs_workspace_bytes"):
        assert pkg.capi.SYMBOLS[name][1] == [C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int], name
