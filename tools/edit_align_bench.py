"""Edit-distance alignment, measured: tmi_edit_align and tmi_edit_confusion (csrc/edit.hip), ``evaluate_generate(
return_alignment=True)`` and ``Wav2Vec2ForCTC.evaluate(edit_ops=True, confusion=True)``.  Writes ONE JSON document (default
profiles/r24_edit_align.json) and prints it.

Kernel, on the five shapes of tools/edit_distance_bench.py (the same generator and seeds), all in one process:
  align_us        tmi_edit_align, the C call on buffers allocated once outside the timed calls
  distance_us     tmi_edit_distance, the kernel without the alignment, on the same tensors
  sweep_only_us   tmi_edit_align of a private build of csrc/edit.hip with -DTMI_EDIT_ALIGN_NO_TRACE (tools/build/, made by
                  ``--build-only`` or on first use): the compaction with columns and the sweep with its move stores, no walk
                  back.  align_us - sweep_only_us is the trace, sweep_only_us - distance_us the move stores and columns.
  host_trace_us   the reference table and backtrace of tests/_edit_align_ref.py looped over the pairs on the host (wall
                  clock, one pass, the tokens already on the host), with its paths compared with the kernel's
  confusion_us    tmi_edit_confusion adding the steps to a table of V = 1024 (the ids folded into it)
Model: ``evaluate_generate`` with and without ``return_alignment`` (Whisper small, bf16, B 8, 24 tokens) and
``Wav2Vec2ForCTC.evaluate(edit_ops=True)`` with and without ``confusion`` (base, bf16, B 8, 5 s clips, 60 labels).

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/edit_align_bench.py [--out profiles/r24_edit_align.json] [--iters 20] [--build-only]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "tethys-speech_amd", "csrc")
SWEEP_ONLY = os.path.join(ROOT, "tools", "build", "libtmi_edit_sweep_only.so")


def build_sweep_only():
    """csrc/edit.hip without the walk back, linked against the package's library for the launch helpers."""
    src = os.path.join(CSRC, "edit.hip")
    if os.path.exists(SWEEP_ONLY) and os.path.getmtime(SWEEP_ONLY) >= os.path.getmtime(src):
        return SWEEP_ONLY
    os.makedirs(os.path.dirname(SWEEP_ONLY), exist_ok=True)
    lib_dir = os.path.dirname(CSRC)
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950",
                    "-Wno-unused-result", "-DTMI_EDIT_ALIGN_NO_TRACE", "-shared", "-I", CSRC, src, "-o", SWEEP_ONLY, "-L", lib_dir,
                    "-ltethys_mi", f"-Wl,-rpath,{lib_dir}"], check=True)
    return SWEEP_ONLY


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_edit_align.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--build-only", action="store_true", help="build the sweep-only library and exit (needs no GPU)")
    args = ap.parse_args()
    build_sweep_only()
    if args.build_only:
        return

    import numpy as np
    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops, wav2vec2, whisper
    import _edit_align_ref as A
    from edit_distance_bench import corrupt, timed_us

    _lib.lib()  # the package's library first: the private one resolves its launch helpers there
    sweep_only = C.CDLL(SWEEP_ONLY)
    sweep_only.tmi_edit_align.restype, sweep_only.tmi_edit_align.argtypes = _lib.SIGNATURES["tmi_edit_align"]
    dev = torch.device("cuda:0")

    def kernel(name, N, n, m, vocab, iters, rate=0.15, exact=False):
        rng = np.random.default_rng(N * 7 + n)
        hyp, ref = np.full((N, n), -1, np.int32), np.full((N, m), -1, np.int32)
        hl, rl = np.zeros(N, np.int32), np.zeros(N, np.int32)
        for i in range(N):
            rl[i] = m if exact else int(rng.integers(max(1, m - m // 8), m + 1))
            hl[i] = n if exact else int(rng.integers(max(1, n - n // 8), n + 1))
            ref[i, :rl[i]] = rng.integers(0, vocab, rl[i])
            hyp[i, :hl[i]] = corrupt(rng, ref[i, :rl[i]], vocab, rate, hl[i])
        h, r, hlen, rlen = (torch.from_numpy(a).to(dev) for a in (hyp, ref, hl, rl))
        ws = torch.empty(ops.edit_align_workspace_elems(N, n, m), dtype=torch.int32, device=dev)
        out = torch.empty(N, 6, dtype=torch.int32, device=dev)
        o2 = torch.empty(N, 6, dtype=torch.int32, device=dev)
        s2 = torch.empty(N, n + m, 3, dtype=torch.int32, device=dev)
        n2 = torch.empty(N, dtype=torch.int32, device=dev)

        def align_call(lib):  # the C call on preallocated buffers: the three forms differ in nothing but the kernel
            def call():
                rc = lib.tmi_edit_align(h.data_ptr(), n, n, hlen.data_ptr(), r.data_ptr(), m, m, rlen.data_ptr(), N, 1, -1, 0, 0,
                                        o2.data_ptr(), 6, s2.data_ptr(), 3 * (n + m), n2.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                        ops.stream())
                assert rc == 0
            return call

        def distance():
            rc = _lib.lib().tmi_edit_distance(h.data_ptr(), n, n, hlen.data_ptr(), r.data_ptr(), m, m, rlen.data_ptr(), N, 1, -1, 0, 0,
                                              out.data_ptr(), 6, ops.stream())
            assert rc == 0

        # the three forms alternate, twice: a drift of the clock shows as a difference between the two rounds
        rounds = []
        for _ in range(2):
            rounds.append((timed_us(align_call(_lib.lib()), iters), timed_us(distance, iters), timed_us(align_call(sweep_only), iters)))
        align_us, dist_us, sweep_us = (min(a, b) for a, b in zip(*rounds))
        got_out, steps, ns = ops.edit_align(h, r, hlen, rlen, workspace=ws)
        same_out = bool(torch.equal(got_out, out)) and bool(torch.equal(o2, out))
        th, tr = (h % 1024).to(torch.int32), (r % 1024).to(torch.int32)  # the ids folded into a table of V = 1024
        counts = ops.edit_confusion(steps, ns, th, tr, 1024)
        conf_us = timed_us(lambda: ops.edit_confusion(steps, ns, th, tr, 1024, counts=counts), iters)
        steps_host, ns_host = steps.cpu().numpy(), ns.cpu().numpy()
        t0 = time.perf_counter()
        want = [A.align(hyp[i, :hl[i]].tolist(), ref[i, :rl[i]].tolist())[1] for i in range(N)]
        host_us = (time.perf_counter() - t0) * 1e6
        same = all([tuple(t) for t in steps_host[i, :ns_host[i]].tolist()] == want[i] for i in range(N))
        return {"shape": name, "pairs": N, "hyp_cols": n, "ref_cols": m, "align_us": round(align_us, 1), "distance_us": round(dist_us, 1),
                "sweep_only_us": round(sweep_us, 1), "trace_us": round(align_us - sweep_us, 1),
                "moves_and_columns_us": round(sweep_us - dist_us, 1), "align_over_distance": round(align_us / dist_us, 2),
                "rounds_us": [[round(x, 1) for x in rd] for rd in rounds], "confusion_us": round(conf_us, 1),
                "host_trace_us": round(host_us, 1), "host_over_align": round(host_us / align_us, 1),
                "mean_steps": float(ns_host.mean()), "workspace_bytes": int(ws.numel() * 4), "out_equal_to_distance_kernel": same_out,
                "paths_equal_to_host": bool(same)}

    it = args.iters
    res = {"device": torch.cuda.get_device_name(0), "iters": it,
           "timing": "HIP events around `iters` back-to-back calls after 3 warm-up calls; the three kernel forms alternate in two "
                     "rounds and the smaller time of each is reported (both rounds are kept); host trace: one pass, wall clock, "
                     "tokens already on the host; the model calls include their host work and read-backs",
           "kernel": [kernel("whisper", 8, 448, 448, 50000, it), kernel("whisper", 64, 448, 448, 50000, it),
                      kernel("ctc", 8, 300, 200, 31, it, rate=0.3), kernel("words", 64, 40, 40, 5000, it),
                      kernel("limit", 1, 4096, 4096, 50000, max(3, it // 4), exact=True)]}

    B = 8
    m = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = (torch.randn(B, m.config.n_mels, 3000, generator=torch.Generator().manual_seed(0)) * 0.5).to(dev)
    labels = torch.randint(3, 50000, (B, 24), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    itm = max(2, it // 5)
    w = {"B": B, "max_length": 24, "iters": itm}
    for name, kw in (("greedy", {}), ("beam4_nbest4", dict(num_beams=4, num_return_sequences=4))):
        w[f"evaluate_generate_{name}_us"] = round(timed_us(lambda: m.evaluate_generate(feats, labels, max_length=24, **kw), itm, warm=1), 1)
        w[f"evaluate_generate_{name}_alignment_us"] = round(
            timed_us(lambda: m.evaluate_generate(feats, labels, max_length=24, return_alignment=True, **kw), itm, warm=1), 1)
    res["whisper_small_bf16"] = w
    del m

    c = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16")
    audio = (torch.randn(B, 5 * 16000, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    V = c.config.vocab_size
    lab = torch.randint(1, V, (B, 60), generator=torch.Generator().manual_seed(2))
    lab[lab == c.config.ctc_blank_id] = (c.config.ctc_blank_id + 1) % V
    e = {"B": B, "seconds": 5.0, "labels": 60, "iters": it}
    for name, kw in (("greedy", {}), ("num_beams_4", dict(num_beams=4))):
        e[f"evaluate_{name}_edit_ops_us"] = round(timed_us(lambda: c.evaluate(audio, lab, edit_ops=True, **kw), it), 1)
        e[f"evaluate_{name}_edit_ops_confusion_us"] = round(timed_us(lambda: c.evaluate(audio, lab, edit_ops=True, confusion=True, **kw), it), 1)
        a, b = c.evaluate(audio, lab, edit_ops=True, **kw), c.evaluate(audio, lab, edit_ops=True, confusion=True, **kw)
        e[f"{name}_same_counts"] = all(a[k] == b[k] for k in a)
        e[f"{name}_table_sum"] = int(b["confusion"].sum())
    res["wav2vec2_base_bf16"] = e
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
