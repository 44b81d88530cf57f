#!/usr/bin/env python3
"""Evaluation job: teacher-forced loss, token accuracy and perplexity of a Whisper model on held-out batches (the metrics
the reference compiles its model with, speech_jobs/whisper_dist.py W:904-907, and the loss of W:585-600, forward only).

Loads ``--weights`` (a ``save_checkpoint`` or ``save_weights`` file, through ``train.load_weights``; without one the
model keeps its seeded initialisation) and evaluates ``--num_batches`` batches of ``--batch_size`` items of the dummy
pool drawn with ``--seed`` (the training pool's seed is 1234: any other seed is held-out data; the project ships no real
dataset).  Prints loss, accuracy and perplexity = exp(loss) and writes them as one JSON file (``--out``).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Whisper held-out loss / accuracy / perplexity")
    parser.add_argument("--model_type", default="small", choices=["tiny", "base", "small", "medium", "large"])
    parser.add_argument("--weights", default=None, help="checkpoint or weights file to evaluate")
    parser.add_argument("--batch_size", type=int, default=8)
    parser.add_argument("--num_batches", type=int, default=5)
    parser.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    parser.add_argument("--seq_len", type=int, default=3000, help="feature frames per item")
    parser.add_argument("--max_target_length", type=int, default=100, help="target tokens per item")
    parser.add_argument("--seed", type=int, default=4321, help="seed of the evaluation pool")
    parser.add_argument("--out", default="whisper_eval.json", help="result file")
    parser.add_argument("--mask_padding", action="store_true",
                        help="score with decoder_attention_mask = (labels != 0), the objective of a --mask_padding training run")
    args = parser.parse_args(argv)
    if args.batch_size < 1 or args.num_batches < 1:
        parser.error("--batch_size and --num_batches must be at least 1")

    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, whisper
    from tethys_speech_amd.data import create_dummy_dataset

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    model = whisper.create_whisper_model(args.model_type, device=device, precision=args.precision)
    whisper.check_evaluate_args(model.config, (args.batch_size, args.max_target_length), None)
    if args.weights:
        train.load_weights(model, args.weights)
    ds = iter(create_dummy_dataset(args.batch_size, n_mels=model.config.n_mels, seq_len=args.seq_len,
                                   max_target_length=args.max_target_length, device=device, seed=args.seed,
                                   with_mask=args.mask_padding))
    torch.cuda.synchronize()
    t0 = time.time()
    res = train.evaluate_whisper(None, model, (next(ds) for _ in range(args.num_batches)))
    dt = time.time() - t0
    out = {"model_type": args.model_type, "precision": args.precision, "weights": args.weights, "batch_size": args.batch_size,
           "num_batches": args.num_batches, "loss": res["loss"], "accuracy": res["accuracy"],
           "perplexity": math.exp(res["loss"]) if res["loss"] < 700 else float("inf"), "n_tokens": res["n_tokens"],
           "n_correct": res["n_correct"], "loss_sum": res["loss_sum"], "seconds": round(dt, 4)}
    print(f"Loss: {out['loss']:.4f}, Accuracy: {out['accuracy']:.4f}, Perplexity: {out['perplexity']:.4f}", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
