"""The fixed-Hamming-weight sampler and the sparse-secret encapsulation exist in every layer (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAME = "troyn_sample_ternary_sparse"


def test_header_declares_the_entry_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "troyn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\b%s\s*\(([^;]*)\);" % NAME, code)
    assert decl, NAME
    args = decl.group(1)
    assert "workspace" not in args and "hamming_weight" in args and "blocks_used" in args and "troyn_stream_t" in args
    block = text[text.index("Context PRNG = AES-128"):text.index("int troyn_prng_block")]
    for word in (NAME, "*blocks_used = N/2", "word j & 1 of block counter + (j >> 1)", "(w_j & ~0xFFFF) | j", "smallest keys", "bit 0 of w_j", "no workspace",
                 "[RandomGenerator::sample_poly_ternary_sparse]", "TROYN_E_INVALID", "hamming_weight == 0 or > N", "N <= 65536"):
        assert word in block, word


def test_binding_library_and_engine(pkg):
    lib = pkg.capi.lib()
    assert NAME in pkg.capi.SYMBOLS
    assert hasattr(lib, NAME), "libtroyn.so does not export %s" % NAME
    assert callable(getattr(pkg.Prng, "ternary_sparse"))


def test_the_kernel_and_its_launch():
    csrc = os.path.join(ROOT, "troy-nova_amd", "csrc")
    kernels = open(os.path.join(csrc, "crypto_kernels.hpp")).read()
    unit = open(os.path.join(csrc, "troyn.hip")).read()
    assert re.search(r"__global__[^\n]*sample_ternary_sparse_kernel", kernels)
    assert re.search(r"hipLaunchKernelGGL\(sample_ternary_sparse_kernel, dim3\(1\), dim3\(SPARSE_TERNARY_THREADS\)", unit)
    usage = open(os.path.join(ROOT, "profiles", "sparse_secret_resource_usage.txt")).read()
    row = [line for line in usage.splitlines() if line.startswith("sample_ternary_sparse_kernel")][0]
    assert row.split("/")[3].strip() == "0", "scratch must be 0: " + row
    assert int(row.split("/")[5]) < 2048, "LDS: " + row


def test_the_mirror_and_the_binding_name_the_methods():
    troy = os.path.join(ROOT, "troy-nova_amd", "troy")
    header = open(os.path.join(troy, "troy.h")).read()
    binder = open(os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")).read()
    for name in ("sample_poly_ternary_sparse", "create_sparse", "create_sparse_encapsulation_keys"):
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("create_sparse", "create_sparse_encapsulation_keys", "SparseEncapsulationKeys", "to_sparse", "to_dense", "half_width_for", "encapsulation_keys"):
        assert '"%s"' % name in binder, name
    assert len(re.findall(r"void bootstrap\(", header)) == 2 and len(re.findall(r"Ciphertext bootstrap_new\(", header)) == 2
    own = open(os.path.join(troy, "bootstrap.h")).read()
    for word in ("struct SparseEncapsulationKeys", "KSwitchKeys to_sparse, to_dense", "hamming_weight", "half_width_for", "sqrt((h + 1) / 12)", "digit 0, limbs {0, K_key - 1}",
                 "never holds a seed", "Sparse packing"):
        assert word in own, word
    assert "dense ternary secrets only" not in own
