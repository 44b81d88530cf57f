#!/usr/bin/env python3
"""Evaluation job: held-out contrastive loss, accuracy, codebook perplexity and code usage of a Wav2Vec2 pre-training model
(the objective of speech_jobs/wav2vec2_dist.py V:866-899 and V:1220, forward only).

Loads ``--weights`` (a ``save_checkpoint`` or ``save_weights`` file, through ``train.load_weights``; without one the
model keeps its seeded initialisation) and evaluates ``--num_batches`` batches of ``--batch_size`` clips of the dummy
pool drawn with ``--seed`` (the training pool's seed is 1234: any other seed is held-out data; the project ships no real
dataset), with negatives drawn from ``--seed + 1``.  ``--ragged`` gives every clip a length of its own in
[clip_samples / 4, clip_samples], drawn from the seed: the tail is zero-filled and the frames behind a clip's end are
masked (``frame_attention_mask``).  Prints one line and writes the result as one JSON file (``--out``).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser(description="Wav2Vec2 held-out contrastive loss / accuracy / perplexity / code usage")
    parser.add_argument("--model_size", default="base", choices=["tiny", "small", "base"])
    parser.add_argument("--weights", default=None, help="checkpoint or weights file to evaluate")
    parser.add_argument("--batch_size", type=int, default=8)
    parser.add_argument("--num_batches", type=int, default=5)
    parser.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    parser.add_argument("--clip_samples", type=int, default=32000, help="samples per (padded) clip")
    parser.add_argument("--seed", type=int, default=4321, help="seed of the evaluation pool")
    parser.add_argument("--ragged", action="store_true", help="clips of different lengths, padded and masked")
    parser.add_argument("--out", default="wav2vec2_eval.json", help="result file")
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.batch_size < 1 or args.num_batches < 1:
        parser.error("--batch_size and --num_batches must be at least 1")
    if args.clip_samples < 4:
        parser.error("--clip_samples must be at least 4")
    return args


def ragged_lengths(rng, batch_size, clip_samples):
    """A length per clip in [clip_samples / 4, clip_samples], drawn from ``rng``."""
    return [int(v) for v in rng.integers(max(1, clip_samples // 4), clip_samples + 1, size=batch_size)]


def main(argv=None):
    args = parse_args(argv)

    import numpy as np
    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, wav2vec2
    from tethys_speech_amd.data import W2VDummyDataset

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    model = wav2vec2.create_full_model("pretraining", args.model_size, device=device, precision=args.precision)
    if args.weights:
        train.load_weights(model, args.weights)
    cfg = model.config
    ds = iter(W2VDummyDataset(args.batch_size, length=args.clip_samples, device=device, seed=args.seed))
    rng = np.random.default_rng(args.seed + 1)
    T = wav2vec2.frame_lengths(cfg, [args.clip_samples])[0]

    def batches():
        for _ in range(args.num_batches):
            audio = next(ds)
            neg = torch.from_numpy(wav2vec2.sample_negative_indices(rng, audio.shape[0], T, cfg.num_negatives)).to(device)
            if not args.ragged:
                yield audio, neg
                continue
            lengths = ragged_lengths(rng, audio.shape[0], args.clip_samples)
            audio = audio.clone()
            for b, n in enumerate(lengths):
                audio[b, n:] = 0.0
            yield audio, neg, wav2vec2.frame_attention_mask(cfg, lengths, args.clip_samples)

    torch.cuda.synchronize()
    t0 = time.time()
    res = train.evaluate_wav2vec2(None, model, batches())
    dt = time.time() - t0
    out = {"model_size": args.model_size, "precision": args.precision, "weights": args.weights, "batch_size": args.batch_size,
           "num_batches": args.num_batches, "clip_samples": args.clip_samples, "ragged": bool(args.ragged),
           "loss": res["loss"], "contrastive_loss": res["contrastive_loss"], "accuracy": res["accuracy"],
           "perplexity": res["perplexity"], "code_usage": res["code_usage"], "n_frames": res["n_frames"],
           "n_correct": res["n_correct"], "loss_sum": res["loss_sum"], "seconds": round(dt, 4)}
    print(f"Loss: {out['loss']:.4f}, Accuracy: {out['accuracy']:.4f}, Perplexity: {out['perplexity']:.4f}, "
          f"Code usage: {out['code_usage']:.4f}", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
