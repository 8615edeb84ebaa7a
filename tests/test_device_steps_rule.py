"""The rule of troy/device_steps.h, read off the sources (no GPU and no built library needed): every C-ABI entry that takes a workspace is called from
exactly one place of the C++ mirror, its step in device_steps.cpp, and no other file asks for a workspace size."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TROY = os.path.join(ROOT, "troy-nova_amd", "troy")

# entries that take a workspace whose size query is not spelled NAME + "_workspace_bytes": they share another entry's query
SHARED_QUERY = (
    "troyn_apply_galois_many", "troyn_apply_galois_sum", "troyn_apply_galois_weighted_sums", "troyn_gather", "troyn_scatter",
    "troyn_divide_and_round_q_last_ntt", "troyn_bgv_mod_t_and_divide_q_last_ntt", "troyn_bgv_switch_key", "troyn_bgv_relinearize",
    "troyn_ckks_encode_simd", "troyn_ckks_encode_polynomial", "troyn_ckks_decode_simd", "troyn_ckks_decode_polynomial",
    "troyn_bgv_apply_galois_many", "troyn_bgv_apply_galois_sum", "troyn_bgv_apply_galois_weighted_sums", "troyn_bgv_apply_galois_sum_each",
    "troyn_bgv_linear_transform_bsgs",
)


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def mirror_sources():
    paths = sorted(glob.glob(os.path.join(TROY, "*.cpp"))) + [os.path.join(ROOT, "troy-nova_amd", "pybind", "binder.cpp")]
    assert os.path.join(TROY, "device_steps.cpp") in paths and len(paths) >= 10, paths
    return {os.path.relpath(p, ROOT): strip_comments(open(p).read()) for p in paths}


def capi_symbols():
    """the keys of capi.SYMBOLS, read as text: importing the package loads the library"""
    text = open(os.path.join(ROOT, "troy-nova_amd", "capi.py")).read()
    body = text[text.index("SYMBOLS = {"):text.index("\n}\n", text.index("SYMBOLS = {"))]
    names = re.findall(r'^\s+"(troyn_\w+)":', body, flags=re.M)
    assert len(names) > 100 and len(set(names)) == len(names)
    return names


def workspace_entries():
    names = capi_symbols()
    entries = [n for n in names if n + "_workspace_bytes" in names]
    for n in SHARED_QUERY:
        assert n in names, n
        if n not in entries:
            entries.append(n)
    return entries


def test_only_device_steps_asks_for_a_workspace_size():
    for path, code in mirror_sources().items():
        if os.path.basename(path) != "device_steps.cpp":
            assert "_workspace_bytes" not in code, path
    # ... and it asks for every one the binding lists
    steps = strip_comments(open(os.path.join(TROY, "device_steps.cpp")).read())
    for name in capi_symbols():
        if name.endswith("_workspace_bytes"):
            assert re.search(r"\b%s\b" % name, steps), name


def test_every_workspace_entry_has_one_caller_and_it_is_its_step():
    sources = mirror_sources()
    entries = workspace_entries()
    assert len(entries) >= 35, entries
    for entry in entries:
        hits = {path: len(re.findall(r"\b%s\b" % entry, code)) for path, code in sources.items()}
        hits = {path: count for path, count in hits.items() if count}
        assert hits == {os.path.join("troy-nova_amd", "troy", "device_steps.cpp"): 1}, (entry, hits)


def test_the_hoisted_steps_take_the_scheme():
    header = strip_comments(open(os.path.join(TROY, "device_steps.h")).read())
    declared = re.findall(r"\b(\w+)\s*\(", header)
    assert not [name for name in declared if name.startswith(("bgv_apply_galois_", "bgv_linear_transform_"))], declared
    for name in ("apply_galois_many_step", "apply_galois_sum_step", "apply_galois_weighted_sums_step", "apply_galois_sum_each_step", "linear_transform_bsgs_step"):
        assert name in declared, name
        signature = header[header.index("void %s(" % name):]
        signature = signature[:signature.index(";")]
        assert re.search(r"const troyn_plan\*\s*plan,\s*const troyn_bgv\*\s*bgv,\s*uint32_t L,\s*bool ckks,\s*bool ntt_form", signature), signature
    assert "mod_raise_step" in declared
