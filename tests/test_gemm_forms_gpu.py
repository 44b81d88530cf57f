"""tmi_gemm in every form the training step calls it (tests/_gemm_forms.py), against the descriptor-level float64
reference with its per-element bound (tests/_gemm_ref.py; checked on the CPU by tests/test_gemm_ref_cpu.py).

Per case: every element of every window within its bound (so NaN-free although everything the contract does not address
holds NaN), everything outside the written windows bit-identical to what was there, the kernel / split / epilogue the
library chose (tmi_gemm_last_path) equal to the expectation written in the table - a dispatch threshold that moves fails
here instead of silently taking the case off its kernel - and, where the case says so, exact or run-to-run identical
results.  With TMI_GEMM_PATHS_DIR set (a test-side variable, not the library's) the paths taken are written to
gemm_paths.json in that directory, for tools/gemm_path_report.py."""
import json
import os

import pytest

import _gemm_forms as F
from _margins import within

pytestmark = pytest.mark.gpu

_PATHS = {}
_DEVICE_ERROR = []   # a launch or a synchronisation raised: nothing more is launched by this module
_FORCED_ENV = bool(os.environ.get("TMI_GEMM_CFG") or os.environ.get("TMI_GEMM_GENERIC"))


@pytest.fixture(scope="module", autouse=True)
def _write_paths():
    yield
    out = os.environ.get("TMI_GEMM_PATHS_DIR")
    if _PATHS and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "gemm_paths.json"), "w") as f:
            json.dump(_PATHS, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("name", [c["name"] for c in F.CASES])
def test_gemm_form(dev, name):
    case = F.BY_NAME[name]
    if _DEVICE_ERROR:
        pytest.fail(f"not launched: {_DEVICE_ERROR[0]}")
    try:
        res = F.run_case(case, dev)
    except Exception as e:  # noqa: BLE001
        _DEVICE_ERROR.append(f"{name} raised {type(e).__name__}: {e}")
        raise
    _PATHS[name] = res["paths"]
    print(f"{name}: paths {res['paths']} worst err/bound {res['ratio']:.4f} redzone {res['redzone']} exact {res['exact']} "
          f"repeat {res['repeat']}")
    within(f"gemm_form/{name}", res["ratio"], 1.0, res["paths"])
    assert res["redzone"], "an element outside the written windows changed"
    if not _FORCED_ENV:   # (a forced configuration in the environment: the rules' expectations do not apply)
        for p in res["paths"]:
            assert p == tuple(case["expect"]), (p, case["expect"])
    if case["exact"]:
        assert res["exact"], "an exact case differs from the exactly rounded reference"
    if case["repeat_equal"]:
        assert res["repeat"], "two runs differ bit-wise"
