"""Runs the GEMM form table (tests/_gemm_forms.py) in THIS interpreter and prints one JSON line per case: the path taken, the
worst err / bound, the redzone result.  Started by tests/test_gemm_forced_gpu.py in a fresh process per forced kernel
(TMI_GEMM_CFG / TMI_GEMM_GENERIC are read once per process).  ``--big`` includes the persistent-form shapes (the eight-phase values).  The first
error ends the run: nothing more is launched on a device that may have faulted."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    import torch
    import _gemm_forms as F
    big = "--big" in argv
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}), flush=True)
        return 2
    dev = torch.device("cuda:0")
    for case in F.CASES:
        if case["children"] == "none" or (case["children"] == "p8" and not big):
            continue
        try:
            res = F.run_case(case, dev, rules=False)
        except Exception as e:  # noqa: BLE001
            print(json.dumps({"case": case["name"], "error": f"{type(e).__name__}: {e}"}), flush=True)
            return 1
        print(json.dumps(dict(case=case["name"], paths=res["paths"], ratio=res["ratio"], redzone=res["redzone"],
                              exact=res["exact"], repeat=res["repeat"])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
