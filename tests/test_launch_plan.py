"""plan_launch (parsip_amd/csrc/psgpu_plan.h), the one place a run's launch shape is decided,
against the table recorded from the code it replaced (launch_plan_util): for every row the same
kernels in the same order with the same grids, the same Params fields and the same launchFlags
bits.  Equal, not close.  No GPU: the header compiles with plain g++."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import run_verdict_util
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


def test_run_verdict_equals_recorded(tmp_path):
    """judge_run, grown and mesh_info (psgpu_plan.h), the verdict psgpu_finish passes on a finished
    run, against the table recorded from the arithmetic they replaced (run_verdict_util): the four
    capacities met and exceeded by one, the plain and the k_front grid tests at their bounds, an
    empty range with stale counters, the protocol errors, firstOverflow and every launchFlags bit.
    Equal, not close."""
    import json

    gpp = shutil.which("g++")
    if gpp is None:
        pytest.skip("no g++")
    with open(os.path.join(ROOT, "tests", "golden", "run_verdict.json")) as f:
        gold = json.load(f)
    assert gold["in_cols"] == run_verdict_util.IN_COLS and gold["out_cols"] == run_verdict_util.OUT_COLS
    cases = run_verdict_util.cases()
    assert list(cases) == list(gold["cases"])
    table = {}
    for name, (inputs, shards) in cases.items():
        g = gold["cases"][name]
        assert g["in"] == inputs and {int(k): tuple(v) for k, v in g["shards"].items()} == shards, name
        table[name] = (inputs, shards, g["out"])
    run_verdict_util.check_coverage(table)
    exe = tmp_path / "run_verdict_check"
    subprocess.run([gpp, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "parsip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "run_verdict_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], input=run_verdict_util.text(cases.values()), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for (name, (_, _, want)), row in zip(table.items(), got):
        assert row == want, f"{name}: " + ", ".join(
            f"{c} {a} != {b}" for c, a, b in zip(run_verdict_util.OUT_COLS, row, want) if a != b)
