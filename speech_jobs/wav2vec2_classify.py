#!/usr/bin/env python3
"""Utterance classification job: Wav2Vec2ForSequenceClassification (speech_jobs/wav2vec2_dist.py V:1004-1067) at
inference, evaluation, and training of the head alone on pooled features of the frozen encoder (a linear probe).

``--weights FILE`` loads the base model of a pre-training ``save_weights`` file (``load_pretrained_encoder``; the head keeps
its seeded initialisation); without it the whole model keeps its initialisation.  The data are ``--num_clips`` clips of
the dummy pool drawn with ``--seed``, each with the label ``data.w2v_dummy_labels`` gives its index (the project ships no
real dataset: the job exercises the path, the labels are not learnable).  ``--ragged`` gives every clip a length of its
own in [clip_samples / 4, clip_samples]: the tail is zero-filled and the frames behind a clip's end are masked.

  --predict    prints one line "Clip i: class c (log-prob x)" per clip
  --eval       prints "Loss: .., Accuracy: .., Top-k accuracy: .." over all clips; --confusion PATH.npy saves the table
  --fit_head   pools every clip once, trains the head for --epochs epochs of --batch_size rows (``fit_head``), prints one
               "Epoch e: loss .." line per epoch, then "Fit: loss .., accuracy .." of the trained head on the same clips
The result goes to ``--out`` as one JSON file and is printed as the last line.
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
    parser = argparse.ArgumentParser(description="Wav2Vec2 utterance classification: predict / evaluate / linear probe")
    parser.add_argument("--model_size", default="base", choices=["tiny", "small", "base"])
    parser.add_argument("--num_labels", type=int, default=2)
    parser.add_argument("--weights", default=None, help="save_weights file of a pre-training model (the encoder)")
    parser.add_argument("--predict", action="store_true")
    parser.add_argument("--eval", action="store_true")
    parser.add_argument("--fit_head", action="store_true")
    parser.add_argument("--epochs", type=int, default=3)
    parser.add_argument("--batch_size", type=int, default=8)
    parser.add_argument("--learning_rate", type=float, default=1e-3)
    parser.add_argument("--num_clips", type=int, default=16)
    parser.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    parser.add_argument("--clip_samples", type=int, default=32000, help="samples per (padded) clip")
    parser.add_argument("--top_k", type=int, default=1)
    parser.add_argument("--seed", type=int, default=4321, help="seed of the clip pool, the lengths and the probe's batches")
    parser.add_argument("--ragged", action="store_true", help="clips of different lengths, padded and masked")
    parser.add_argument("--confusion", default=None, metavar="PATH.npy", help="with --eval: save the confusion table")
    parser.add_argument("--out", default="wav2vec2_classify.json", help="result file")
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not (args.predict or args.eval or args.fit_head):
        parser.error("give at least one of --predict, --eval, --fit_head")
    if args.batch_size < 1 or args.num_clips < 1 or args.epochs < 0:
        parser.error("--batch_size and --num_clips must be at least 1, --epochs at least 0")
    if not 1 <= args.num_labels <= 1024 or not 1 <= args.top_k <= args.num_labels:
        parser.error("1 <= --num_labels <= 1024 and 1 <= --top_k <= --num_labels")
    if args.clip_samples < 4:
        parser.error("--clip_samples must be at least 4")
    if args.confusion and not args.eval:
        parser.error("--confusion comes with --eval")
    return args


def main(argv=None):
    args = parse_args(argv)

    import numpy as np
    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    from tethys_speech_amd.data import W2VDummyDataset, w2v_dummy_labels

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    model = wav2vec2.create_classification_model(args.model_size, num_labels=args.num_labels, device=device,
                                                 precision=args.precision)
    if args.weights:
        wav2vec2.load_pretrained_encoder(model, args.weights)
    cfg = model.config
    pool = W2VDummyDataset(1, length=args.clip_samples, device=device, seed=args.seed, num_samples=args.num_clips).audio
    labels = w2v_dummy_labels(args.num_clips, args.num_labels)
    rng = np.random.default_rng(args.seed + 1)
    ks = tuple(sorted({1, args.top_k}))

    def batches():
        for s in range(0, args.num_clips, args.batch_size):
            audio, lab = pool[s:s + args.batch_size], torch.from_numpy(labels[s:s + args.batch_size])
            if not args.ragged:
                yield s, audio, lab, None
                continue
            lengths = [int(v) for v in rng.integers(max(1, args.clip_samples // 4), args.clip_samples + 1, size=audio.shape[0])]
            audio = audio.clone()
            for b, n in enumerate(lengths):
                audio[b, n:] = 0.0
            yield s, audio, lab, wav2vec2.frame_attention_mask(cfg, lengths, args.clip_samples)

    out = {"model_size": args.model_size, "precision": args.precision, "weights": args.weights, "num_labels": args.num_labels,
           "num_clips": args.num_clips, "clip_samples": args.clip_samples, "ragged": bool(args.ragged)}
    torch.cuda.synchronize()
    t0 = time.time()
    if args.predict:
        preds = []
        for s, audio, _, mask in batches():
            r = model(audio, attention_mask=mask)
            best = r["log_probs"].gather(1, r["predictions"].long()[:, None])[:, 0]
            for i, (c, lp) in enumerate(zip(r["predictions"].tolist(), best.tolist())):
                print(f"Clip {s + i}: class {c} (log-prob {lp:.4f})", flush=True)
                preds.append(c)
        out["predictions"] = preds
    if args.eval:
        tot = {"n_items": 0, "nll_sum": 0.0, "n_correct": 0, "topk_correct": {k: 0 for k in ks}}
        table = bool(args.confusion)
        for _, audio, lab, mask in batches():
            r = model.evaluate(audio, lab, attention_mask=mask, top_k=ks, confusion=table)
            table = r.get("confusion", False)   # (the device table, passed back in: accumulated there)
            for k in ("n_items", "nll_sum", "n_correct"):
                tot[k] += r[k]
            for k in ks:
                tot["topk_correct"][k] += r["topk_correct"][k]
        n = max(tot["n_items"], 1)
        out["eval"] = {"loss": tot["nll_sum"] / n, "accuracy": tot["n_correct"] / n, "n_items": tot["n_items"],
                       "topk_accuracy": {str(k): tot["topk_correct"][k] / n for k in ks}}
        print(f"Loss: {out['eval']['loss']:.4f}, Accuracy: {out['eval']['accuracy']:.4f}, "
              f"Top-{ks[-1]} accuracy: {out['eval']['topk_accuracy'][str(ks[-1])]:.4f}", flush=True)
        if args.confusion:
            np.save(args.confusion, table.cpu().numpy())
            out["confusion"] = args.confusion
    if args.fit_head:
        feats = torch.cat([model.pool_features(audio, attention_mask=mask) for _, audio, _, mask in batches()])
        hist = wav2vec2.fit_head(model, feats, labels, args.epochs, args.batch_size, learning_rate=args.learning_rate,
                                 seed=args.seed)
        for h in hist:
            print(f"Epoch {h['epoch'] + 1}: loss {h['loss']:.4f}", flush=True)
        ev = model.evaluate_features(feats, labels)
        print(f"Fit: loss {ev['loss']:.4f}, accuracy {ev['accuracy']:.4f}", flush=True)
        out["fit_head"] = {"history": hist, "loss": ev["loss"], "accuracy": ev["accuracy"], "epochs": args.epochs,
                           "batch_size": args.batch_size, "learning_rate": args.learning_rate}
    torch.cuda.synchronize()
    out["seconds"] = round(time.time() - t0, 4)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
