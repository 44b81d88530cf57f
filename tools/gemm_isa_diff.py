"""Does a refactor of a .hip file leave the device code of its kernels as it was?  Compares two gfx950 assembly files
(hipcc <the Makefile's flags> --save-temps -c FILE.hip writes FILE-hip-amdgcn-amd-amdhsa-gfx950.s) kernel by kernel:

  * the set of kernels (names demangled; --rename 'REGEX=REPLACEMENT' rewrites BASE names whose template arguments changed);
  * per kernel the .amdhsa_ resource block (VGPR / AGPR / SGPR counts, LDS and scratch size, ...), line by line;
  * per kernel the instruction sequence, with labels renumbered and comments dropped.  One difference is allowed and
    counted: the immediate offset of a scalar load (s_load_dword*) whose other operands are unchanged - a field that
    leaves the kernel-argument struct moves the ones behind it.

usage: gemm_isa_diff.py BASE.s HEAD.s [--rename 'REGEX=REPL' ...] [-v]
Prints one line per kernel and a summary; exit status 1 if a kernel is missing, new or different.
(profiles/r08_gemm_refactor_isa.txt is its output for the refactor that retired the experimental GEMM configurations.)"""
import argparse, difflib, re, shutil, subprocess, sys


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return dict(zip(names, names))
    # (binutils' c++filt does not know DF16b, the mangling of __bf16: it goes through as Dh, "half", which these kernels never use)
    out = subprocess.run([tool], input="\n".join(n.replace("DF16b", "Dh") for n in names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"\bhalf\b", "__bf16", o.replace("(anonymous namespace)::", "")) for n, o in zip(names, out)}


def parse(path):
    """-> {mangled kernel name: (descriptor lines, instruction lines)}"""
    lines = open(path).read().split("\n")
    desc, body, i = {}, {}, 0
    while i < len(lines):
        t = lines[i].strip()
        if t.startswith(".amdhsa_kernel "):
            name, block = t.split()[1], []
            i += 1
            while not lines[i].strip().startswith(".end_amdhsa_kernel"):
                block.append(lines[i].strip())
                i += 1
            desc[name] = block
        i += 1
    label = re.compile(r"^([A-Za-z_.$][\w.$]*):")
    i = 0
    while i < len(lines):
        m = label.match(lines[i])
        if m and m.group(1) in desc:
            name, ins = m.group(1), []
            i += 1
            while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
                t = lines[i].split(";")[0].strip()
                if t and not t.startswith(".") or re.match(r"^\.LBB\d+_\d+:", t):
                    t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t)
                    ins.append(re.sub(r"\s+", " ", t.replace(name, "KERNEL")))
                i += 1
            body[name] = ins
        i += 1
    return {n: (desc[n], body.get(n, [])) for n in desc}


SLOAD = re.compile(r"^(s_load_dword\w* \S+ \S+) (0x[0-9a-f]+|\d+)$")


def compare(b_ins, h_ins):
    """-> (number of scalar-load offset differences, unified diff of everything else)"""
    if len(b_ins) == len(h_ins):
        moved, other = 0, []
        for x, y in zip(b_ins, h_ins):
            if x == y:
                continue
            mx, my = SLOAD.match(x), SLOAD.match(y)
            if mx and my and mx.group(1) == my.group(1):
                moved += 1
            else:
                other += ["- " + x, "+ " + y]
        return moved, other
    return 0, [l for l in difflib.unified_diff(b_ins, h_ins, "base", "head", n=1, lineterm="")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("head")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("-v", action="store_true", help="print the differing lines")
    a = ap.parse_args()
    base, head = parse(a.base), parse(a.head)
    bn, hn = demangle(list(base)), demangle(list(head))
    for r in a.rename:
        pat, repl = r.split("=", 1)
        bn = {k: re.sub(pat, repl, v) for k, v in bn.items()}
    B, H = {bn[k]: v for k, v in base.items()}, {hn[k]: v for k, v in head.items()}
    assert len(B) == len(base) and len(H) == len(head), "kernel names collide after renaming"
    bad = 0
    for n in sorted(set(B) - set(H)):
        print(f"LOST      {n}")
        bad += 1
    for n in sorted(set(H) - set(B)):
        print(f"NEW       {n}")
        bad += 1
    same = moved_only = 0
    for n in sorted(set(B) & set(H)):
        ddiff = [l for l in difflib.unified_diff(B[n][0], H[n][0], "base", "head", n=0, lineterm="")]
        moved, other = compare(B[n][1], H[n][1])
        res = {k: next((l.split()[1] for l in H[n][0] if l.startswith(k + " ")), "?") for k in
               (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size")}
        info = f"{len(H[n][1]):6d} lines  vgpr+agpr {res['.amdhsa_next_free_vgpr']:>3s} (acc at {res['.amdhsa_accum_offset']:>3s}) sgpr {res['.amdhsa_next_free_sgpr']:>3s} " \
               f"lds {res['.amdhsa_group_segment_fixed_size']} scratch {res['.amdhsa_private_segment_fixed_size']}"
        if ddiff or other:
            bad += 1
            print(f"DIFFERENT {n}: {len(ddiff)} descriptor, {len(other)} instruction diff lines")
            if a.v:
                print("\n".join("    " + l for l in ddiff + other))
        elif moved:
            moved_only += 1
            print(f"same*     {info}  {n}   (* {moved} scalar-load offsets)")
        else:
            same += 1
            print(f"same      {info}  {n}")
    print(f"\n{len(B)} kernels in base, {len(H)} in head: {same} identical, {moved_only} identical but for scalar-load offsets, {bad} lost / new / different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
