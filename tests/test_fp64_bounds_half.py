"""tools/fp64_half_check.cpp: a host build of csrc/dev_math_f64.hpp replays mulpair_half_kernel's arithmetic (csrc/mulpair_half_kernels.hpp: the inverse
transform of a1 (.) b1 at N = 16384 as 5 + 5 + 3 + 1 Gentleman-Sande layers, the sums of every block's 2nd and 4th layer re-centred) over the flagship
chain, both ends of the 50-bit class and the smallest prime of the ring.  It exits non-zero when an intermediate reaches 2^53, a block exceeds its
derived bound, or a butterfly or a digit differs from 128-bit integer arithmetic / the oracle's inverse transform."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_half_limb_sequences_exact_and_below_2_53(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found at %s (the check is a host-only build of a HIP header)" % HIPCC)
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler for the oracle"
    obj, exe = str(tmp_path / "troy_oracle.o"), str(tmp_path / "fp64_half_check")
    subprocess.check_call([cc, "-O2", "-c", os.path.join(ROOT, "oracle", "troy_oracle.c"), "-o", obj])
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma",
                           "-I", os.path.join(ROOT, "troy-nova_amd", "csrc"), os.path.join(ROOT, "tools", "fp64_half_check.cpp"),
                           "-x", "none", obj, "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = "\n".join(res.stdout.splitlines()[-25:])
    assert res.returncode == 0, tail
    assert "ALL EXACT" in res.stdout and not any(w in res.stdout for w in ("MISMATCH", "RANGE", "BOUND")), tail
    # the supremum of the class (p -> 2^50): round A's 4th layer peaks at 7.25 p = 0.906 x 2^53; every intermediate is strictly below 2^53
    peak = [ln for ln in res.stdout.splitlines() if ln.startswith("worst case peak")]
    assert peak and float(peak[0].split()[3]) <= 7.2501, peak
    worst = [ln for ln in res.stdout.splitlines() if ln.startswith("largest value seen")]
    assert worst and float(worst[0].split()[3]) < 0.91, worst
