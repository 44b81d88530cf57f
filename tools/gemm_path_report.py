"""Which GEMM kernel ran which test case: the table of launch paths recorded by tests/test_gemm_forms_gpu.py (the library's
own rules: gemm_paths.json), the path-named tests of tests/test_kernels_gpu.py (rules too: gemm_paths_kernel_tests.json) and
tests/test_gemm_forced_gpu.py (one file per forced kernel), grouped by path.  All write
them to the directory TMI_GEMM_PATHS_DIR names when it is set.

  TMI_GEMM_PATHS_DIR=<dir> python -m pytest -m gpu tests/test_gemm_forms_gpu.py tests/test_gemm_forced_gpu.py tests/test_kernels_gpu.py
  python tools/gemm_path_report.py <dir> > profiles/rNN_gemm_paths.txt

A path is (kernel, K ranges, flags) as tmi_gemm_last_path reports it."""
import glob
import json
import os
import sys

KERNELS = {1: "gemm.hip::launch (generic kernel)", 4: "launch_fast Tile128x128", 5: "launch_fast Tile256x256",
           6: "launch_fast Tile64Waves2", 10: "launch_p8, 256-row tiles", 12: "launch_fast Tile64Waves4",
           13: "launch_fast Tile64Waves4Ring4", 14: "launch_p8, 192-row tiles", 15: "launch_fast Tile64KGroups2Ring4",
           16: "launch_fast Tile64KGroups2Ring2", 32: "launch_f32 (fp32 operands)"}
FLAGS = ((1, "persistent"), (2, "atomic split-K"), (4, "slab split-K"), (8, "K ranges over XCD groups"),
         (16, "16/32 K ranges dealt per XCD"), (32, "wide epilogue"))


def describe(path):
    kern, nsplit, flags = path
    words = [name for bit, name in FLAGS if flags & bit]
    if not flags & 32:
        words.append("element epilogue")
    return f"{KERNELS.get(kern, kern)}, {nsplit} K range{'s' if nsplit != 1 else ''}, " + ", ".join(words)


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    d = argv[1]
    reached = {}
    for f in sorted(glob.glob(os.path.join(d, "gemm_paths*.json"))):
        tag = os.path.basename(f)[len("gemm_paths"):-len(".json")].lstrip("_") or "rules"   # (TMI_...: a forced kernel)
        for case, paths in json.load(open(f)).items():
            for p in paths:
                reached.setdefault(tuple(p), {}).setdefault(tag, []).append(case)
    for path in sorted(reached):
        print(describe(path) + f"   {list(path)}")
        for tag in sorted(reached[path], key=lambda t: (t.startswith("TMI_"), t)):
            print(f"    {tag}: " + ", ".join(sorted(set(reached[path][tag]))))
    # reachability per (kernel, split form) and per (kernel, epilogue form): under the library's own rules alone, and with
    # the forced kernels added; what is left is named with the reason the dispatch code gives
    def tags_of(path):
        return set(reached[path])
    rules = {p for p in reached if any(not t.startswith("TMI_") for t in tags_of(p))}
    for title, got in (("under the library's own rules", rules), ("under the rules or a forced kernel", set(reached))):
        have = {(p[0], form(p)) for p in got} | {(p[0], "wide epilogue" if p[2] & 32 else "element epilogue") for p in got}
        print(f"never reached {title}:")
        missing = [(k, f) for k in sorted(UNIVERSE) for f in UNIVERSE[k] + ["wide epilogue", "element epilogue"] if (k, f) not in have]
        for k, f in missing:
            print(f"    {KERNELS[k]}: {f}" + (f"  - {WHY[(k, f)]}" if (k, f) in WHY else ""))
        if not missing:
            print("    nothing")


def form(path):
    _, nsplit, fl = path
    if fl & 1:
        return "persistent"
    if fl & 2:
        return "atomic split over XCD groups" if fl & 8 else "atomic split"
    if fl & 4:
        return "slab split dealt per XCD" if fl & 16 else "slab split over XCD groups" if fl & 8 else "slab split on grid.y"
    return "no split"


_TILE = ["no split", "atomic split", "atomic split over XCD groups", "slab split on grid.y", "slab split over XCD groups"]
_P8 = ["no split", "persistent", "slab split on grid.y", "slab split over XCD groups", "slab split dealt per XCD"]
UNIVERSE = {1: ["no split", "atomic split"], 4: _TILE, 5: _TILE, 6: _TILE, 12: ["no split"], 13: ["no split"], 15: ["no split"],
            16: ["no split"], 10: _P8, 14: _P8, 32: ["no split", "atomic split", "slab split on grid.y"]}
_ONLY_BF16 = "the rules pick this tile for bf16 outputs only and a split needs an fp32 output: forced kernel only"
_W2 = "the rules pick this tile only for a caller-chosen split (atomics on grid.y): forced kernel only"
_GRIDY = "2, 4 and 8 K ranges of an unbatched launch are always dealt over XCD groups; grid.y is left to 3, 5, 6, 7 ranges or nbatch > 1"
WHY = {(5, "atomic split"): _ONLY_BF16, (5, "atomic split over XCD groups"): _ONLY_BF16, (5, "slab split on grid.y"): _ONLY_BF16,
       (5, "slab split over XCD groups"): _ONLY_BF16, (6, "no split"): _W2, (6, "atomic split over XCD groups"): _W2,
       (6, "slab split on grid.y"): _W2, (6, "slab split over XCD groups"): _W2, (6, "element epilogue"): _W2,
       (4, "atomic split"): _GRIDY, (10, "slab split on grid.y"): _GRIDY, (14, "slab split on grid.y"): _GRIDY,
       (14, "slab split on grid.y"): _GRIDY,
       (13, "element epilogue"): "no case with an unaligned C on this tile", (16, "element epilogue"): "reached by tests/test_kernels_gpu.py only when its paths are recorded",
       (10, "element epilogue"): "the eight-phase rules need N >= 256 and the callers' ldc is a multiple of 8 there: no case",
       (14, "element epilogue"): "the eight-phase rules need N >= 256 and the callers' ldc is a multiple of 8 there: no case",
       (1, "atomic split"): "the step's weight gradients all meet the fast kernels' alignment: TMI_GEMM_GENERIC=1 only",
       (10, "slab split dealt per XCD"): "the deep-K rule takes 192-row tiles whenever they pad fewer rows than 256-row ones, and the forced value 10 does not apply that rule: no case",
       (14, "slab split dealt per XCD"): "the deep-K rule is switched off under a forced kernel: rules only",
       (12, "element epilogue"): "the unaligned-C case has K >= 512 and runs the K-groups under the rules: forced kernel only",
       (5, "element epilogue"): "no case with an unaligned C on this tile", (1, "wide epilogue"): "the generic kernel has the element epilogue only"}


if __name__ == "__main__":
    main(sys.argv)
