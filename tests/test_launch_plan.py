"""plan_launch (parsip_amd/csrc/psgpu_plan.h), the one place a run's launch shape is decided,
against the table recorded from the code it replaced (launch_plan_util): for every row the same
kernels in the same order with the same grids, the same Params fields and the same launchFlags
bits.  Equal, not close.  No GPU: the header compiles with plain g++."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from launch_plan_util import IN_COLS, KERNELS, OUT_COLS, check_coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    with np.load(os.path.join(ROOT, "tests", "golden", "launch_plan.npz")) as z:
        assert list(z["in_cols"]) == IN_COLS and list(z["out_cols"]) == OUT_COLS and list(z["kernels"]) == KERNELS
        return z["inputs"], z["expected"]


def test_table_reaches_every_branch(table):
    inputs, expected = table
    assert inputs.shape == (len(expected), len(IN_COLS)) and expected.shape[1] == len(OUT_COLS) and len(inputs) > 500
    check_coverage(inputs, expected)


def test_plan_equals_recorded_launches(table, tmp_path):
    gpp = shutil.which("g++")
    if gpp is None:
        pytest.skip("no g++")
    inputs, expected = table
    exe = tmp_path / "plan_check"
    subprocess.run([gpp, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "parsip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "plan_check.cpp"), "-o", str(exe)], check=True)
    text = "\n".join(" ".join(str(int(x)) for x in row) for row in inputs) + "\n"
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()], dtype=np.int64)
    assert got.shape == expected.shape
    bad = np.flatnonzero((got != expected).any(axis=1))
    assert bad.size == 0, "\n".join(
        f"row {n}: {dict(zip(IN_COLS, inputs[n].tolist()))}\n  " + ", ".join(
            f"{c} {got[n, j]} != {expected[n, j]}" for j, c in enumerate(OUT_COLS) if got[n, j] != expected[n, j])
        for n in bad[:5])
