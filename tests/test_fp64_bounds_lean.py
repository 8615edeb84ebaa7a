"""tools/fp64_lean_check.cpp: a host build of csrc/dev_math_f64.hpp replays the lean FP64 transform body's changed sequences (the centred hand-over inside
mrr_tail_kernel, a1 (.) b1 entering its inverse transform as it is, TAIL_RESCALE's single re-centring, digits stored as doubles) over the flagship chain
and the ends of the 50-bit class at N = 16384.  It exits non-zero when a value reaches 2^53 or a result differs from 128-bit integer arithmetic."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_lean_sequences_exact_and_below_2_53(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found at %s (the check is a host-only build of a HIP header)" % HIPCC)
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler for the oracle"
    obj, exe = str(tmp_path / "troy_oracle.o"), str(tmp_path / "fp64_lean_check")
    subprocess.check_call([cc, "-O2", "-c", os.path.join(ROOT, "oracle", "troy_oracle.c"), "-o", obj])
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma",
                           "-I", os.path.join(ROOT, "troy-nova_amd", "csrc"), os.path.join(ROOT, "tools", "fp64_lean_check.cpp"),
                           "-x", "none", obj, "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = "\n".join(res.stdout.splitlines()[-25:])
    assert res.returncode == 0, tail
    assert "ALL EXACT" in res.stdout and "MISMATCH" not in res.stdout and "RANGE" not in res.stdout, tail
    # the worst case of the class (p -> 2^50) stays below 2^53 with the margin the header comments state
    worst = [ln for ln in res.stdout.splitlines() if ln.startswith("largest value seen")]
    assert worst and float(worst[0].split()[3]) < 0.97, worst
