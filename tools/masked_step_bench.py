"""The training step on the weighted loss (decoder_attention_mask = labels != 0, W:596-598) against the plain-mean step, measured:
Whisper small-ref, bf16, B = 8, 30 s clips, the reference's dropout active - the step ``bench.py`` times - through
``train.planned_step``.  One model, one process: the two-input and the three-input step have a launch plan each (keyed by
the input signature); after both are recorded and warmed, the two are timed in alternating blocks of ``--steps`` steps
(>= 50) between device events.  Per kind: the mean over the blocks of the block's ms per step, and the block-to-block
spread (largest minus smallest block).  Both kinds train the same model, so they see the same weights drift.

Also: the cross-entropy entry alone at the step's [800, 51904] bf16 logits, unweighted (tmi_xent_fwd_bwd) and weighted
(tmi_xent_weighted under the first batch's mask), rotating over copies of the logits as tools/xent_bench.py does.

Writes one JSON file (default profiles/r12_masked_step.json) and prints it.
usage: python tools/masked_step_bench.py [--blocks 6] [--steps 50] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, optim, train, whisper  # noqa: E402
from tethys_speech_amd.data import create_dummy_dataset  # noqa: E402
from tethys_speech_amd.dist import DataParallelStrategy  # noqa: E402


def block_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def xent_alone(dev, labels, mask, reps=5, n=8):
    """us per launch of the two entries at [B*S, 51904] bf16, V = 51865: the median of ``reps`` alternating groups of n."""
    B, S = labels.shape
    V, ld = 51865, 51904
    torch.manual_seed(0)
    src = (torch.randn(B * S, ld, device=dev) * 2).to(torch.bfloat16)
    bufs = [src.clone() for _ in range(n)]  # (the kernel overwrites its input: every launch reads logits-like data)
    row_loss, row_w, inv = torch.empty(B * S, device=dev), torch.empty(B * S, device=dev), torch.empty(1, device=dev)
    ops.xent_weights(mask, B, S, row_w, inv)
    kinds = {"unweighted": lambda i: ops.xent_fwd_bwd(bufs[i], ld, labels, row_loss, B, S, V, 1.0 / (B * (S - 1))),
             "weighted": lambda i: ops.xent_fwd_bwd_weighted(bufs[i], ld, labels, row_w, inv, row_loss, B, S, V, 1.0)}
    us = {k: [] for k in kinds}
    for rep in range(reps + 1):
        for k, f in kinds.items():
            for b in bufs:
                b.copy_(src)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                f(i)
            e1.record()
            torch.cuda.synchronize()
            if rep:  # (the first group warms up)
                us[k].append(e0.elapsed_time(e1) * 1e3 / n)
    return {k: round(statistics.median(v), 2) for k, v in us.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_masked_step.json"))
    args = ap.parse_args(argv)
    if args.steps < 50 or args.blocks < 2:
        ap.error("--steps must be at least 50 and --blocks at least 2")
    dev = "cuda:0"
    B = 8
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    model.refresh_shadows()
    model.enable_dropout(model.config.dropout, model.config.attention_dropout, seed=1234 * 1000003)
    opt = optim.Adam(1e-4)
    step = train.planned_step(DataParallelStrategy(0, 1, init=False), model, opt, "whisper", pipelined=True)
    if step.planned is None:
        raise SystemExit("launch plans are switched off (TMI_PLAN=0): this tool times the planned step")
    it = iter(create_dummy_dataset(B, device=dev, drop_remainder=True, with_mask=True))
    batches = [next(it) for _ in range(6)]  # the six full batches of a pass over the 50-sample pool
    pos = [0]

    def run(masked):
        f, l, m = batches[pos[0] % len(batches)]
        pos[0] += 1
        return step(f, l, m) if masked else step(f, l)

    for masked in (False, True):  # two eager steps, the recording, three replays - per kind
        for _ in range(6):
            run(masked)
    torch.cuda.synchronize()
    plans = {len(sig): st["plan"] for sig, st in step.planned._by_sig.items() if st.get("plan") is not None}
    assert set(plans) == {2, 3}, "both plans must be recorded before anything is timed"
    ms = {False: [], True: []}
    for _ in range(args.blocks):
        for masked in (False, True):
            ms[masked].append(block_ms(lambda: run(masked), args.steps))
    model.finish_late()
    torch.cuda.synchronize()
    S = batches[0][1].shape[1]
    unscored = [float((m[:, :-1] == 0).sum()) + m.shape[0] for _, _, m in batches]  # (weight 0, and the B rows t = S-1)
    kern = xent_alone(dev, batches[0][1], batches[0][2])
    two, three = ms[False], ms[True]
    out = {"model": "whisper small-ref", "precision": "bf16", "batch": B, "dropout": True, "blocks": args.blocks,
           "steps_per_block": args.steps,
           "two_input_step_ms": round(statistics.mean(two), 4), "two_input_block_spread_ms": round(max(two) - min(two), 4),
           "three_input_step_ms": round(statistics.mean(three), 4), "three_input_block_spread_ms": round(max(three) - min(three), 4),
           "two_input_blocks_ms": [round(v, 4) for v in two], "three_input_blocks_ms": [round(v, 4) for v in three],
           "plan_launches": {"two_input": plans[2].launches, "three_input": plans[3].launches},
           "unscored_row_fraction": round(sum(unscored) / (len(batches) * B * S), 4),
           "unscored_row_fraction_without_the_last_position": round((sum(unscored) - len(batches) * B) / (len(batches) * B * S), 4),
           "xent_unweighted_us": kern["unweighted"], "xent_weighted_us": kern["weighted"],
           "xent_rows_unscored_in_kernel_timing": round((float((batches[0][2][:, :-1] == 0).sum()) + B) / (B * S), 4),
           "gate_three_le_two_plus_spread": statistics.mean(three) <= statistics.mean(two) + (max(two) - min(two))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
