"""The CKKS encoder entries exist in every layer below the C++ mirror (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("troyn_ckks_create", "troyn_ckks_destroy", "troyn_ckks_get_tables", "troyn_ckks_workspace_bytes", "troyn_ckks_encode_workspace_bytes", "troyn_ckks_encode_simd",
         "troyn_ckks_encode_polynomial", "troyn_ckks_decode_polynomial", "troyn_ckks_decode_simd")


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    block = text[text.index("CKKS encoder on the device"):text.index("typedef struct troyn_ckks troyn_ckks;")]
    # the block quotes the host loops it mirrors and states both contracts and the house rules
    for word in ("ENCODING CONTRACT", "DECODING CONTRACT", "d.re * r.re - d.im * r.im", "w.re * r.re - w.im * r.im", "ties to even", "too_large",
                 "TROYN_E_INVALID", "TROYN_E_WORKSPACE", "TROYN_E_UNSUPPORTED", "batch == 0", "count == 0", "no entry synchronises"):
        assert word in block, word


def test_binding_lists_the_entries(pkg):
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS, name


def test_library_exports_the_entries(pkg):
    lib = pkg.capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), "libtroyn.so does not export %s" % name


def test_the_kernels_have_a_unit_of_their_own_without_fused_multiply_add():
    make = open(os.path.join(ROOT, "troy-nova_amd", "csrc", "Makefile")).read()
    assert "troyn_ckks.hip" in make and "-ffp-contract=off" in make


def test_engine_has_the_wrapper(pkg):
    assert callable(getattr(pkg.Plan, "ckks_handle"))
    for name in ("encode_simd", "encode_polynomial", "decode_simd", "decode_polynomial", "tables"):
        assert callable(getattr(pkg.CkksEncoder, name)), name
