"""Every GEMM kernel on every form: the form table (tests/_gemm_forms.py) once per forced configuration, each in a child
process of its own (TMI_GEMM_CFG and TMI_GEMM_GENERIC are read once per process).

Children run strictly one at a time, each a fresh ``subprocess.run`` with a copy of the environment plus the one variable and
a timeout of its own.  A child that ends by a signal or at its timeout is not retried, and the remaining children of the
session are skipped with that reason: nothing more is started on a device that may have faulted.

Per child: every case within its bound and redzone-clean, exact / repeatable where the table says so; the cases the forced
value CAN run (``_gemm_forms.can_run``: the conditions at the top of launch_fast) must report that kernel, the others fall
back to the rules and are checked all the same.  The eight-phase values (10: 256-row tiles, 14: 192-row tiles) also run
the persistent-form shapes, which no small shape reaches."""
import json
import os
import subprocess
import sys

import pytest

import _gemm_forms as F
from _margins import within

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gemm_forms_child.py")
_STOP = {}   # reason, once a child died


def _run_child(var, value, big):
    if _STOP:
        pytest.skip(f"not started: an earlier child {_STOP['why']}")
    env = dict(os.environ)
    env[var] = str(value)
    cmd = [sys.executable, CHILD] + (["--big"] if big else [])
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _STOP["why"] = f"({var}={value}) ran into its timeout"
        pytest.fail(f"child {var}={value} timed out")
    if p.returncode < 0:
        _STOP["why"] = f"({var}={value}) ended by signal {-p.returncode}"
        pytest.fail(f"child {var}={value} ended by signal {-p.returncode}: {p.stderr[-2000:]}")
    rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    # the child exits non-zero only when a launch or a synchronisation raised (comparisons are printed, not raised): the
    # device may have faulted, so nothing more is started on it
    if p.returncode != 0 or any("error" in r for r in rows):
        _STOP["why"] = f"({var}={value}) ended with status {p.returncode}: {[r for r in rows if 'error' in r][-1:]}"
        pytest.fail(f"child {var}={value} ended with status {p.returncode}: {rows[-1:]} {p.stderr[-2000:]}")
    return {r["case"]: r for r in rows}


def _check(var, value, rows, kernel_of):
    expected = [c for c in F.CASES if c["children"] == "all" or c["children"] == "p8" and var == "TMI_GEMM_CFG" and value in (10, 14)]
    assert sorted(rows) == sorted(c["name"] for c in expected)
    report = {}
    for case in expected:
        r = rows[case["name"]]
        print(f"{var}={value} {case['name']}: paths {r['paths']} worst err/bound {r['ratio']:.4f} redzone {r['redzone']}")
        report[case["name"]] = r["paths"]
    for case in expected:
        r = rows[case["name"]]
        within(f"gemm_forced/{var}={value}/{case['name']}", r["ratio"], 1.0, r["paths"])
        assert r["redzone"], case["name"]
        if case["exact"]:
            assert r["exact"], case["name"]
        # (run-to-run identity is a property of slab splits and of at most two atomic contributions per element: a kernel
        # that sums this case with more atomics than that owes none)
        if case["repeat_equal"] and not any(p[2] & F.ATOMIC and p[1] > 2 for p in r["paths"]):
            assert r["repeat"], case["name"]
        for L, path in zip(case["launches"], r["paths"]):
            want = kernel_of(case, L)
            if want is not None:
                assert path[0] == want, (case["name"], path, want)
    out = os.environ.get("TMI_GEMM_PATHS_DIR")    # (test-side: where tools/gemm_path_report.py finds the recorded paths)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"gemm_paths_{var}_{value}.json"), "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("cfg", F.FORCED)
def test_gemm_forms_under_forced_kernel(dev, cfg):
    rows = _run_child("TMI_GEMM_CFG", cfg, big=cfg in (10, 14))
    _check("TMI_GEMM_CFG", cfg, rows, lambda case, L: cfg if F.can_run(L, case["in_f32"], cfg) else None)
    ran = [c["name"] for c in F.CASES if c["name"] in rows and any(F.can_run(L, c["in_f32"], cfg) for L in c["launches"])]
    assert ran, f"no case ran on kernel {cfg}"
    if cfg in (10, 14):   # the persistent form, on this value's tile height
        for name, r in rows.items():
            if name.startswith("persistent_"):
                assert r["paths"][0][0] == cfg and r["paths"][0][2] & F.PERSISTENT, (name, r["paths"])


def test_gemm_forms_on_the_generic_kernel(dev):
    rows = _run_child("TMI_GEMM_GENERIC", 1, big=False)
    _check("TMI_GEMM_GENERIC", 1, rows, lambda case, L: F.GENERIC)
