"""scone_mean_div_of_sum (scone_amd/csrc/scone_mean_div.h), the mean's division in the MXFP4 lookups, checked on the CPU as
tests/test_mean_div_cpu.py checks its siblings: tests/mean_div_of_sum_host.c includes the helper the kernels call and compares
it with `x / k` for every x a sum can be (everything but -0): +0, every subnormal numerator below 2^16 of both signs, random
bit patterns of the whole fp32 space, quotients around FLT_MIN and the function's own threshold 2^-125 k, alone and beside
zeros, for k = 2..64 and a few large k."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mean_div_of_sum_equals_ieee_division(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not on PATH")
    exe = str(tmp_path / "mean_div_of_sum_host")
    cmd = ["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math"]
    try:
        if " fma " in open("/proc/cpuinfo").read().replace("\n", " "):
            cmd.append("-mfma")       # fmaf() as one instruction instead of a libm call: same value, a fraction of the time
    except OSError:
        pass
    cmd += [os.path.join(ROOT, "tests", "mean_div_of_sum_host.c"), "-o", exe, "-lm"]
    subprocess.run(cmd, check=True, capture_output=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    tail = p.stdout[-3000:]
    m = re.search(r"checked (\d+) mismatches (\d+) zero_blocks_fast (\d+) of (\d+)", p.stdout)
    assert m, tail + p.stderr[-1000:]
    assert int(m.group(1)) > 74 * 2 * (2 ** 19 + 2 ** 18 + 2 ** 17 - 4), tail
    assert p.returncode == 0 and int(m.group(2)) == 0 and m.group(3) == m.group(4), tail
