"""The division of the mean, checked on the CPU: scone_amd/csrc/scone_mean_div.h is plain C, so tests/mean_div_host.c includes
the very helper the kernels call and compares it with `x / k` (one IEEE division) over every subnormal numerator below 2^16
of both signs, 2^24 random bit patterns of the whole fp32 space, patterns whose quotient lies around FLT_MIN and the special
values, for k = 2..64 and a few large k.  -ffp-contract=off / -fno-fast-math: the same rounding rules as the device build.
The GPU tests (tests/test_gpu_edge_values.py) then only have to show that the device executes the same arithmetic."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def test_mean_div_helper_equals_ieee_division(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not on PATH")
    exe = str(tmp_path / "mean_div_host")
    cmd = ["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp"]
    if _has_fma():
        cmd.append("-mfma")           # fmaf() as one instruction instead of a libm call: same value, a fraction of the time
    cmd += [os.path.join(ROOT, "tests", "mean_div_host.c"), "-o", exe, "-lm"]
    subprocess.run(cmd, check=True, capture_output=True)
    env = dict(os.environ, OMP_NUM_THREADS=str(min(8, os.cpu_count() or 1)))
    p = subprocess.run([exe], capture_output=True, text=True, timeout=1500, env=env)
    tail = p.stdout[-3000:]
    m = re.search(r"checked (\d+) mismatches (\d+)", p.stdout)
    assert m, tail + p.stderr[-1000:]
    assert int(m.group(1)) > 74 * (2 ** 24 + 2 ** 17), tail
    assert p.returncode == 0 and int(m.group(2)) == 0, tail
    assert int(re.search(r"in range (\d+)", p.stdout).group(1)) > 74 * 2 ** 22, tail      # the short form was exercised too
    # the inputs can tell: the bare shortcut is wrong on thousands of the subnormal numerators and on inf (2^32 flag)
    bare = int(re.search(r"bare shortcut mismatches (\d+)", p.stdout).group(1))
    assert bare >= 2 ** 32 + 1000, tail
