#!/usr/bin/env python3
"""Inference job: CTC transcripts of padded clips from a Wav2Vec2ForCTC model (the reference's ``create_full_model("asr")``,
speech_jobs/wav2vec2_dist.py V:940-1001, forward only).

Loads weights (``--weights``: a ``save_checkpoint`` or ``save_weights`` file of a CTC model; ``--pretrained_encoder``: a
``save_weights`` file of a pre-training model, whose base model is copied and whose heads are ignored; without either the
model keeps its seeded initialisation), pads the ``--wav`` clips (16-bit PCM mono 16 kHz) to the longest of them - or,
without one, takes ``--batch_size`` dummy clips of ``--seconds``, every second one cut to 60 % - builds the frame mask
(``wav2vec2.frame_attention_mask``) and decodes greedily.  ``--labels FILE`` (one line of space-separated token ids per
clip; an empty line: no labels) also scores the clips (``evaluate``) and aligns the labels to the frames (``align``);
``--posteriors`` adds, after the aligned times, each token's expected number of frames and its centre time under ALL paths
that spell the labels (``posteriors``: ``expected_frames``, ``center_time``), where ``align`` gives the best path's.
``--num_beams K`` (2..16) decodes by CTC prefix beam search instead (``decode(num_beams=K)``): the line then carries the best
sequence, its score ``sequence_score`` and, with ``--nbest R``, the R best sequences and scores under ``nbest``; the
timestamps are those of the best sequence's forced alignment, and with labels the edit distance is the best sequence's.
``--lm PATH.npy`` (with ``--num_beams``; ``--lm_alpha``, ``--lm_beta``) fuses an n-gram table of log-probabilities, shape
[vocab_size] * order, into the search (``decode(lm=...)``): ``sequence_score`` is then the fused score, and the line and
every ``nbest`` entry also carry ``ctc_score`` and ``lm_score``.  ``--build_lm LABELS_FILE --lm_order N --lm_out PATH.npy``
builds such a table from a file of label lines (``wav2vec2.ngram_lm_table``, add-one smoothing), writes it and exits:
no model is created and no GPU is needed.
Prints one JSON line per clip: the token ids, with ``--timestamps`` their start and end times in seconds, the best path's
log-probability, and with labels the nll, the edit distance of the transcript and the aligned times; then one summary line.
``--edit_ops`` (with ``--labels``): the error counts come from the device kernel (``evaluate(edit_ops=True)``) and the
summary line adds the substitutions, deletions and insertions and, with ``--num_beams``, the n-best oracle error rate.
``--confusion PATH.npy`` (with ``--edit_ops``): the confusion table of the transcripts against the labels, int64
[vocab_size + 1, vocab_size + 1] (row = the label, column = the transcript's token, the last index = none), is folded on the
device (``evaluate(confusion=True)``) and saved.
``--fit_head`` (with ``--labels``; ``--epochs``, ``--train_batch_size``, ``--learning_rate``, ``--save FILE``): before anything
is decoded the CTC head is trained on the clips with the encoder frozen - the clips are encoded once
(``encode_features``), ``wav2vec2.fit_ctc_head`` runs the epochs and prints one JSON line per epoch, then the line of
``evaluate_features`` on the same clips; ``--save`` writes the model with ``train.save_weights``.  The rest of the job then
reports the trained head.  Clips without labels (an empty line) train as an empty transcript.
``--layer_mix`` (with ``--fit_head``): the probe reads a learned softmax-weighted sum of ALL encoder layers instead of the last
one (``encode_features(layers="all")``, ``fit_ctc_head(layer_mix=...)``): every epoch's line adds the layer weights,
``--save FILE`` also writes ``FILE.layermix.npy`` (the K logits), and the mix stays attached (``set_layer_mix``) so the rest of
the job decodes through it.  ``--layer_mix_file F.npy`` attaches a saved mix for the rest of the job (without ``--fit_head``:
to a model loaded with ``--weights``; with ``--fit_head --layer_mix``: the logits the fit starts from).
``--mask_time_prob P --mask_time_length L --mask_feature_prob P --mask_feature_length L`` (with ``--fit_head``, with or without
``--layer_mix``): SpecAugment on the cached features - every step of the fit zeroes spans of frames and of columns inside the
head kernels (``fit_ctc_head(spec_augment=wav2vec2.SpecAugment(...))``; a flag that is not given keeps ``SpecAugment``'s
default: 0.05 / 10 for the time mask, 0 / 10 for the feature mask) and every epoch's line adds ``masked_frame_fraction``.
The evaluation and the rest of the job never mask.
There is no tokenizer: ids in, ids out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_labels(path, n_clips):
    rows = [[int(t) for t in line.split()] for line in open(path).read().splitlines()]
    if len(rows) != n_clips:
        raise SystemExit(f"--labels holds {len(rows)} lines for {n_clips} clips")
    return rows


def main(argv=None):
    parser = argparse.ArgumentParser(description="Wav2Vec2 CTC transcripts of padded clips (greedy decode, loss, alignment)")
    parser.add_argument("--model_size", default="base", choices=["tiny", "small", "base"])
    parser.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    parser.add_argument("--weights", default=None, help="checkpoint of a CTC model to load")
    parser.add_argument("--pretrained_encoder", default=None, help="save_weights file of a pre-training model: its base model is loaded")
    parser.add_argument("--vocab_size", type=int, default=32)
    parser.add_argument("--wav", action="append", default=[], help="16-bit PCM mono 16 kHz .wav file (repeatable)")
    parser.add_argument("--batch_size", type=int, default=2, help="number of dummy clips when no --wav is given")
    parser.add_argument("--seconds", type=float, default=2.0, help="length of the dummy clips")
    parser.add_argument("--timestamps", action="store_true", help="print token start and end times")
    parser.add_argument("--labels", default=None, help="file of token ids, one line per clip: evaluate and align")
    parser.add_argument("--posteriors", action="store_true",
                        help="with --labels: each token's expected frames and centre time over all paths (forward-backward)")
    parser.add_argument("--num_beams", type=int, default=None, help="CTC prefix beam search with this many beams (2..16)")
    parser.add_argument("--nbest", type=int, default=1, help="with --num_beams: print this many sequences per clip")
    parser.add_argument("--lm", default=None, help="with --num_beams: .npy n-gram table [vocab_size] * order fused into the search")
    parser.add_argument("--lm_alpha", type=float, default=0.5, help="weight of the table's log-probabilities")
    parser.add_argument("--lm_beta", type=float, default=0.0, help="bonus per token")
    parser.add_argument("--edit_ops", action="store_true",
                        help="with --labels: count substitutions / deletions / insertions on the device (and the n-best oracle)")
    parser.add_argument("--confusion", default=None, help="with --labels --edit_ops: save the confusion table as this .npy file")
    parser.add_argument("--fit_head", action="store_true", help="with --labels: train the CTC head on the clips, the encoder frozen")
    parser.add_argument("--epochs", type=int, default=10, help="with --fit_head")
    parser.add_argument("--train_batch_size", type=int, default=8, help="with --fit_head: clips per head step")
    parser.add_argument("--learning_rate", type=float, default=1e-3, help="with --fit_head: Adam's")
    parser.add_argument("--save", default=None, help="with --fit_head: write the trained model here (train.save_weights)")
    parser.add_argument("--layer_mix", action="store_true",
                        help="with --fit_head: train a softmax-weighted sum over all encoder layers in front of the head")
    parser.add_argument("--layer_mix_file", default=None, help=".npy of K mixing logits: attach this layer mix for the rest of the job")
    parser.add_argument("--mask_time_prob", type=float, default=None,
                        help="with --fit_head: SpecAugment, the probability that a frame starts a masked span (default 0.05)")
    parser.add_argument("--mask_time_length", type=int, default=None, help="with --fit_head: frames per span, 1..64 (default 10)")
    parser.add_argument("--mask_feature_prob", type=float, default=None,
                        help="with --fit_head: SpecAugment, the probability that a column starts a masked span (default 0)")
    parser.add_argument("--mask_feature_length", type=int, default=None, help="with --fit_head: columns per span, 1..64 (default 10)")
    parser.add_argument("--build_lm", default=None, help="file of token ids, one line per sequence: build a table and exit")
    parser.add_argument("--lm_order", type=int, default=2, help="with --build_lm: the order of the table (1..4)")
    parser.add_argument("--lm_out", default=None, help="with --build_lm: where the .npy table goes")
    args = parser.parse_args(argv)
    if args.confusion and not (args.edit_ops and args.labels):
        parser.error("--confusion comes with --labels and --edit_ops")
    if args.fit_head and not args.labels:
        parser.error("--fit_head comes with --labels")
    if args.save and not args.fit_head:
        parser.error("--save comes with --fit_head")
    if args.layer_mix and not args.fit_head:
        parser.error("--layer_mix comes with --fit_head")
    spec_flags = {k: getattr(args, k) for k in ("mask_time_prob", "mask_time_length", "mask_feature_prob", "mask_feature_length")
                  if getattr(args, k) is not None}
    if spec_flags and not args.fit_head:
        parser.error("--" + sorted(spec_flags)[0] + " comes with --fit_head")
    spec = None
    if spec_flags:
        import tethys_speech_amd  # noqa: F401
        from tethys_speech_amd import wav2vec2 as w2v
        spec = w2v.SpecAugment(**spec_flags)
        try:
            w2v.check_spec_augment_args(spec, 1, 8)  # the probabilities and lengths; T and H are checked by the fit
        except ValueError as e:
            parser.error(str(e))

    import numpy as np
    if args.build_lm:
        if not args.lm_out:
            raise SystemExit("--build_lm comes with --lm_out")
        import tethys_speech_amd  # noqa: F401
        from tethys_speech_amd import wav2vec2 as w2v
        cfg = w2v.make_config(args.model_size, vocab_size=args.vocab_size)
        rows = [[int(t) for t in line.split()] for line in open(args.build_lm).read().splitlines()]
        width = max([len(r) for r in rows] + [1])
        table = w2v.ngram_lm_table([r + [0] * (width - len(r)) for r in rows], [len(r) for r in rows], args.lm_order,
                                   cfg.vocab_size, cfg.ctc_blank_id)
        np.save(args.lm_out, table)
        print(json.dumps({"lm": args.lm_out, "order": args.lm_order, "vocab_size": cfg.vocab_size, "sequences": len(rows),
                          "tokens": sum(len(r) for r in rows)}), flush=True)
        return
    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, wav2vec2, whisper

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    model = wav2vec2.create_full_model("asr", args.model_size, device=device, precision=args.precision,
                                       vocab_size=args.vocab_size)
    if args.pretrained_encoder:
        wav2vec2.load_pretrained_encoder(model, args.pretrained_encoder)
    if args.weights:
        train.load_weights(model, args.weights)
    if args.wav:
        clips = [(p, whisper.read_wav(p)) for p in args.wav]
    else:
        n = max(1, int(args.seconds * 16000))
        wave = whisper.dummy_waveform()[:n]
        clips = [(f"dummy{i}", wave if i % 2 == 0 else wave[:max(1, (3 * n) // 5)]) for i in range(max(1, args.batch_size))]
    lengths = [len(w) for _, w in clips]
    T_in = max(lengths)
    batch = np.zeros((len(clips), T_in), dtype=np.float32)
    for row, (_, w) in zip(batch, clips):
        row[:len(w)] = w
    mask = wav2vec2.frame_attention_mask(model.config, lengths, T_in)
    audio = torch.from_numpy(batch).to(device)
    rows = read_labels(args.labels, len(clips)) if args.labels else None
    mix = None
    if args.layer_mix or args.layer_mix_file:
        mix = wav2vec2.LayerMix(model.config.num_hidden_layers + 1, device)
        if args.layer_mix_file:
            mix.load_state_dict({"logits": np.load(args.layer_mix_file)})

    def masked(rec):  # the epoch line's share of SpecAugment
        return {"masked_frame_fraction": rec["masked_frame_fraction"]} if "masked_frame_fraction" in rec else {}

    if args.fit_head and mix is not None and args.layer_mix:
        L = max([len(r) for r in rows] + [1])
        fit_labels = np.zeros((len(rows), L), dtype=np.int64)
        for i, r in enumerate(rows):
            fit_labels[i, :len(r)] = r
        fit_lens = [len(r) for r in rows]
        feats = model.encode_features(audio, attention_mask=mask, layers="all")
        hist = wav2vec2.fit_ctc_head(model, feats["hidden_layers"], feats["frame_lengths"], fit_labels, fit_lens, args.epochs,
                                     args.train_batch_size, learning_rate=args.learning_rate, layer_mix=mix, spec_augment=spec)
        for rec in hist:
            print(json.dumps({"fit_head_epoch": rec["epoch"] + 1, "loss": rec["loss"], "n_infeasible": rec["n_infeasible"],
                              "layer_weights": rec["layer_weights"], **masked(rec)}), flush=True)
        fit = model.evaluate_features(feats["hidden_layers"], feats["frame_lengths"], fit_labels, fit_lens, layer_mix=mix)
        print(json.dumps({"fit_head": {k: fit[k] for k in ("loss", "nll_sum", "n_infeasible", "n_edits", "n_ref_tokens",
                                                           "token_error_rate")}, "epochs": len(hist),
                          "layer_weights": mix.weights().cpu().tolist()}), flush=True)
        if args.save:
            train.save_weights(model, args.save)
            np.save(args.save + ".layermix.npy", mix.state_dict()["logits"].numpy())
    elif args.fit_head:
        L = max([len(r) for r in rows] + [1])
        fit_labels = np.zeros((len(rows), L), dtype=np.int64)
        for i, r in enumerate(rows):
            fit_labels[i, :len(r)] = r
        fit_lens = [len(r) for r in rows]
        feats = model.encode_features(audio, attention_mask=mask)
        hist = wav2vec2.fit_ctc_head(model, feats["hidden"], feats["frame_lengths"], fit_labels, fit_lens, args.epochs,
                                     args.train_batch_size, learning_rate=args.learning_rate, spec_augment=spec)
        for rec in hist:
            print(json.dumps({"fit_head_epoch": rec["epoch"] + 1, "loss": rec["loss"], "n_infeasible": rec["n_infeasible"],
                              **masked(rec)}), flush=True)
        fit = model.evaluate_features(feats["hidden"], feats["frame_lengths"], fit_labels, fit_lens)
        print(json.dumps({"fit_head": {k: fit[k] for k in ("loss", "nll_sum", "n_infeasible", "n_edits", "n_ref_tokens",
                                                           "token_error_rate")}, "epochs": len(hist)}), flush=True)
        if args.save:
            train.save_weights(model, args.save)
    if mix is not None:
        model.set_layer_mix(mix)
    torch.cuda.synchronize()
    t0 = time.time()
    beam = args.num_beams is not None and args.num_beams > 1
    if args.nbest != 1 and not beam:
        raise SystemExit("--nbest comes with --num_beams >= 2")
    if args.lm and not beam:
        raise SystemExit("--lm comes with --num_beams >= 2")
    lm_kw = dict(lm=np.load(args.lm), lm_alpha=args.lm_alpha, lm_beta=args.lm_beta) if args.lm else {}
    if beam:
        wav2vec2.check_ctc_beam_args(model.config, args.num_beams, args.nbest)
        dec = model.decode(audio, attention_mask=mask, num_beams=args.num_beams, num_return_sequences=args.nbest,
                           return_timestamps=args.timestamps, **lm_kw)
    else:
        dec = model.decode(audio, attention_mask=mask)
    if args.posteriors and rows is None:
        raise SystemExit("--posteriors comes with --labels")
    ev = al = post = None
    if rows is not None:
        L = max(len(r) for r in rows)
        labels = torch.zeros(len(rows), L, dtype=torch.int64)
        for i, r in enumerate(rows):
            labels[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
        lens = [len(r) for r in rows]
        ev = model.evaluate(audio, labels, lens, attention_mask=mask, return_items=True,
                            num_beams=args.num_beams if beam else None, edit_ops=args.edit_ops, confusion=bool(args.confusion),
                            **lm_kw)
        al = model.align(audio, labels, lens, attention_mask=mask)
        if args.posteriors:
            post = model.posteriors(audio, labels, lens, attention_mask=mask)
    torch.cuda.synchronize()
    dt = time.time() - t0
    frames = [int(x) for x in mask.sum(1).tolist()]
    for i, (name, _) in enumerate(clips):
        if beam:
            seqs, lens_, scores = (dec[n] if args.nbest > 1 else dec[n][:, None] for n in ("sequences", "lengths", "sequences_scores"))
            k = int(lens_[i, 0])
            line = {"clip": name, "frames": frames[i], "tokens": seqs[i, 0, :k].tolist(), "sequence_score": float(scores[i, 0]),
                    "n_beams": int(dec["n_beams"][i])}
            if args.nbest > 1:
                line["nbest"] = [{"tokens": seqs[i, r, :int(lens_[i, r])].tolist(), "score": float(scores[i, r])}
                                 for r in range(min(args.nbest, int(dec["n_beams"][i])))]
            if args.lm:
                ctc, lms = (dec[n] if args.nbest > 1 else dec[n][:, None] for n in ("ctc_scores", "lm_scores"))
                line.update(ctc_score=float(ctc[i, 0]), lm_score=float(lms[i, 0]))
                for r, entry in enumerate(line.get("nbest", [])):
                    entry.update(ctc_score=float(ctc[i, r]), lm_score=float(lms[i, r]))
        else:
            k = int(dec["lengths"][i])
            line = {"clip": name, "frames": frames[i], "tokens": dec["sequences"][i, :k].tolist(),
                    "best_path_logprob": float(dec["best_path_logprob"][i])}
        if args.timestamps:
            line["start"] = [round(t, 4) for t in dec["token_start_times"][i, :k].tolist()]
            line["end"] = [round(t, 4) for t in dec["token_end_times"][i, :k].tolist()]
        if rows is not None:
            n = len(rows[i])
            line["labels"] = rows[i]
            line["nll"] = float(ev["nll"][i])
            line["infeasible"] = bool(ev["infeasible"][i])
            line["edits"] = wav2vec2.edit_distance(np.asarray(line["tokens"]), np.asarray(rows[i]))
            line["path_logprob"] = float(al["path_logprob"][i])
            line["aligned_start"] = [round(t, 4) for t in al["token_start_times"][i, :n].tolist()]
            line["aligned_end"] = [round(t, 4) for t in al["token_end_times"][i, :n].tolist()]
            if post is not None:
                line["expected_frames"] = [round(t, 3) for t in post["token_expected_frames"][i, :n].tolist()]
                line["center_time"] = [round(t, 4) for t in post["token_center_times"][i, :n].tolist()]
        print(json.dumps(line), flush=True)
    summary = {"clips": len(clips), "samples": T_in, "seconds": round(dt, 4)}
    if ev is not None:
        summary.update({k: ev[k] for k in ("loss", "nll_sum", "n_infeasible", "n_edits", "n_ref_tokens", "token_error_rate")})
        if args.edit_ops:
            summary.update({k: ev[k] for k in ("n_sub", "n_del", "n_ins", "n_hyp_tokens", "n_oracle_edits", "oracle_error_rate")
                            if k in ev})
        if args.confusion:
            np.save(args.confusion, ev["confusion"].cpu().numpy())
            summary["confusion"] = args.confusion
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
