#!/usr/bin/env python3
"""Inference job: greedy, beam-search or sampled transcription with a Whisper model (the reference's ``transcribe_audio`` / ``generate``,
speech_jobs/whisper_dist.py W:962-986 / W:636-709, which its job scripts never call).

Loads a checkpoint (``--resume_from``: a ``save_checkpoint`` or ``save_weights`` file; without one the model keeps its
seeded initialisation), turns each ``--wav`` clip (16-bit PCM mono 16 kHz) or, without one, ``--batch_size`` copies of
the reference's seeded 30 s dummy clip into log-mel features on the GPU, and decodes them greedily or, with
``--num_beams`` > 1, by beam search, or with ``--do_sample`` by seeded sampling (``--temperature --top_k --top_p
--min_length --seed``; adds "logprob", the sum of the tokens' log-probabilities).  Prints one JSON line per returned sequence, {"clip", "ids", "n_tokens"} (ids start
with the decoder start token; beam search adds "rank" and "score"), then one timing line.  No tokenizer ships
with the project, so the output is token ids.

``--repetition_penalty``, ``--no_repeat_ngram_size``, ``--suppress_tokens 1,2,3``, ``--begin_suppress_tokens`` and
``--prompt_ids`` are ``generate``'s decode constraints and decoder prompt, in every mode: the logit of a token already
in the transcript is divided (or, when negative, multiplied) by the penalty, a token that would repeat an n-gram cannot be
emitted, the suppressed ids never appear (the begin-suppressed ones not as the first token), and the prompt's tokens
follow the start token in the printed ids ("n_tokens" counts them; ``--max_length`` still counts generated tokens and is
capped so that both fit the decoder).

``--save_cross_attentions PATH`` writes, after decoding, the cross-attention weights of each clip's (best) transcript to
an ``.npz``: one more forward pass over [start, tokens] with ``output_attentions=("cross",)`` - under the reference's
inverted decoder mask every decoding step recomputes the whole prefix, so this pass is the last step's computation -
saved as ``attn_<i>`` fp32 [decoder_layers, S, T] (the mean over the heads), ``ids_<i>`` int32 [S] and ``clips`` (names).

``--timestamps`` prints, after each transcript, one ``[start -> end] id`` line per token: the seconds at which the token
begins and ends (``model.align``: dynamic time warping over the cross-attention weights, on the GPU).  Aligning the last
token needs one more decoder position than choosing it, so ``--max_length`` is capped at 447.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Whisper transcription, greedy or beam search (token ids)")
    parser.add_argument("--model_type", default="small", choices=["tiny", "base", "small", "medium", "large"])
    parser.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    parser.add_argument("--resume_from", default=None, help="checkpoint to load the weights from")
    parser.add_argument("--wav", action="append", default=[], help="16-bit PCM mono 16 kHz .wav file (repeatable)")
    parser.add_argument("--batch_size", type=int, default=1, help="number of dummy clips when no --wav is given")
    parser.add_argument("--max_length", type=int, default=448, help="decoding steps at most (<= 448)")
    parser.add_argument("--num_beams", type=int, default=1, help="1: greedy; 2 to 8: beam search")
    parser.add_argument("--length_penalty", type=float, default=1.0, help="beam search: score = sum log p / length ** this")
    parser.add_argument("--num_return_sequences", type=int, default=1, help="beam search: hypotheses per clip (<= num_beams)")
    parser.add_argument("--do_sample", action="store_true", help="sampled decoding (not with --num_beams > 1)")
    parser.add_argument("--temperature", type=float, default=1.0, help="sampling: the logits are divided by this")
    parser.add_argument("--top_k", type=int, default=50, help="sampling: keep the k largest (0: no filter; at most 64)")
    parser.add_argument("--top_p", type=float, default=1.0, help="sampling: nucleus mass within the top_k, in (0, 1]")
    parser.add_argument("--min_length", type=int, default=0, help="sampling: no end-of-text in the first this many tokens")
    parser.add_argument("--seed", type=int, default=0, help="sampling: the seed (a seeded run repeats)")
    parser.add_argument("--save_cross_attentions", default=None, metavar="PATH",
                        help="write the head-mean cross-attention weights [layers, S, T] of each transcript to this .npz")
    parser.add_argument("--timestamps", action="store_true",
                        help="after each transcript, one '[start -> end] id' line per token (seconds; DTW over the "
                             "cross-attention weights); caps --max_length at 447")
    id_list = lambda text: [int(v) for v in text.split(",") if v.strip()]  # noqa: E731
    parser.add_argument("--repetition_penalty", type=float, default=None,
                        help="logits of tokens already in the transcript: / this when positive, * this otherwise (1: off)")
    parser.add_argument("--no_repeat_ngram_size", type=int, default=0, help="no n-gram of this size appears twice (0: off)")
    parser.add_argument("--suppress_tokens", type=id_list, default=[], metavar="1,2,3", help="ids that are never emitted")
    parser.add_argument("--begin_suppress_tokens", type=id_list, default=[], metavar="1,2,3",
                        help="ids that are not emitted as the first token")
    parser.add_argument("--prompt_ids", type=id_list, default=[], metavar="1,2,3",
                        help="decoder prompt: these ids follow the start token")
    parser.add_argument("--segment_timestamps", action="store_true",
                        help="decode under Whisper's timestamp-token grammar; every result carries its segments "
                             "(start / end in units of 0.02 s and the text ids)")
    parser.add_argument("--long", action="store_true",
                        help="long-form transcription: walk each clip in 30 s windows by its timestamp tokens "
                             "(whisper.transcribe_long) and print its segments in seconds; implies the timestamp grammar")
    parser.add_argument("--max_initial_timestamp", type=float, default=1.0,
                        help="with --segment_timestamps / --long: the first timestamp of a window is at most this (seconds)")
    parser.add_argument("--no_condition_on_previous_text", action="store_true",
                        help="with --long: do not prompt a window with the text of the windows before it")
    args = parser.parse_args(argv)
    if args.do_sample and args.num_beams > 1:
        parser.error("--do_sample does not go with --num_beams > 1")

    import numpy as np
    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, whisper
    from tethys_speech_amd.frontend import LogMelFrontend

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    model = whisper.create_whisper_model(args.model_type, device=device, precision=args.precision)
    if args.timestamps:
        args.max_length = min(args.max_length, model.config.max_target_positions - 1)
    if args.prompt_ids:
        room = model.config.max_target_positions - (1 if args.timestamps else 0) - len(args.prompt_ids)
        args.max_length = max(0, min(args.max_length, room))
    cons = dict(repetition_penalty=args.repetition_penalty, no_repeat_ngram_size=args.no_repeat_ngram_size,
                suppress_tokens=args.suppress_tokens, begin_suppress_tokens=args.begin_suppress_tokens,
                prompt_ids=args.prompt_ids or None)
    whisper.check_constraint_args(model.config, args.max_length, args.num_beams, return_token_timestamps=args.timestamps,
                                  **cons)
    ts = dict(segment_timestamps=True, max_initial_timestamp=args.max_initial_timestamp) \
        if args.segment_timestamps or args.long else {}
    if ts:
        whisper.check_timestamp_rule_args(model.config, suppress_tokens=args.suppress_tokens,
                                          min_length=args.min_length if args.do_sample else None, **ts)
    seg = lambda out, r: {"segments": out["segments"][r]} if ts else {}  # noqa: E731
    beam = args.num_beams > 1
    sample = dict(do_sample=True, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                  min_length=args.min_length, seed=args.seed) if args.do_sample else None
    if sample:
        whisper.check_sample_args(model.config, args.max_length, args.num_beams, args.temperature, args.top_k, args.top_p,
                                  args.min_length)
    elif beam:
        whisper.check_beam_args(model.config, args.max_length, args.num_beams, 1.0, args.length_penalty,
                                args.num_return_sequences)
    else:
        whisper.check_generate_args(model.config, args.max_length)
    if args.resume_from:
        train.load_weights(model, args.resume_from)
    if args.wav:
        clips = [(p, whisper.read_wav(p)) for p in args.wav]
    else:
        clips = [(f"dummy{i}", whisper.dummy_waveform()) for i in range(max(1, args.batch_size))]
    fe = LogMelFrontend(device=device, n_mels=model.config.n_mels)
    torch.cuda.synchronize()
    t0 = time.time()
    n_tok = 0
    if args.long:
        for name, wav in clips:
            res = whisper.transcribe_long(
                model, wav, condition_on_previous_text=not args.no_condition_on_previous_text,
                max_initial_timestamp=args.max_initial_timestamp, max_length=args.max_length, num_beams=args.num_beams,
                length_penalty=args.length_penalty, do_sample=args.do_sample, temperature=args.temperature,
                top_k=args.top_k, top_p=args.top_p, seed=args.seed, **cons)
            n_tok += len(res["ids"])
            print(json.dumps({"clip": name, "n_windows": res["n_windows"], "n_tokens": len(res["ids"]),
                              "segments": [{"start": round(s["start"], 2), "end": round(s["end"], 2), "ids": s["ids"]}
                                           for s in res["segments"]]}), flush=True)
        torch.cuda.synchronize()
        dt = time.time() - t0
        print(json.dumps({"clips": len(clips), "seconds": round(dt, 4), "tokens": n_tok,
                          "tokens_per_s": round(n_tok / dt, 1) if dt > 0 else None}), flush=True)
        return
    # clips of one length are decoded as one batch (the dummy clips, or wav files of equal length)
    groups = {}
    for name, wav in clips:
        groups.setdefault(len(wav), []).append((name, wav))
    saved = {"clips": []}

    def save_cross(name, feats_row, ids):
        """One clip: forward over its transcript, head-mean of every layer's cross-attention weights."""
        if not args.save_cross_attentions:
            return
        ids = list(ids)[:model.config.max_target_positions]
        dec = torch.tensor([ids], dtype=torch.int32, device=device)
        out = model.forward_infer(feats_row[None], decoder_input_ids=dec, output_attentions=("cross",),
                                  attentions_dtype=torch.float32)
        i = len(saved["clips"])
        saved["clips"].append(name)
        saved[f"attn_{i}"] = torch.stack([a[0].mean(dim=0) for a in out["cross_attentions"]]).cpu().numpy()
        saved[f"ids_{i}"] = np.asarray(ids, dtype=np.int32)

    def stamps(feats, seqs, lens, wav_len, rows):
        """The token lines of the sequences ``rows`` (indices into seqs) -> {row: text}."""
        if not args.timestamps:
            return {}
        frames = (fe.num_frames(wav_len) + 1) // 2  # encoder frames of the clips of this group
        al = model.align(feats, seqs.to(device), None if lens is None else lens.to(device),
                         num_frames=[frames] * feats.shape[0])
        t0s, t1s = al["token_start_times"].cpu(), al["token_end_times"].cpu()
        out = {}
        for r in rows:
            n = seqs.shape[1] - 1 if lens is None else int(lens[r])
            out[r] = "\n".join(f"[{float(t0s[r, k]):.2f} -> {float(t1s[r, k]):.2f}] {int(seqs[r, 1 + k])}" for k in range(n))
        return out

    for items in groups.values():
        wave = torch.from_numpy(np.stack([w for _, w in items])).to(device)
        if args.save_cross_attentions or args.timestamps:
            feats_all = fe(wave)
        if sample:
            out = model.generate(fe(wave), max_length=args.max_length, return_dict_in_generate=True, **sample, **cons, **ts)
            seqs, scores, lens = out["sequences"].cpu(), out["sequences_scores"].cpu(), out["lengths"].cpu()
            lines = stamps(feats_all, seqs, lens, wave.shape[1], range(len(items))) if args.timestamps else {}
            for j, ((name, _), row, sc, n) in enumerate(zip(items, seqs, scores, lens)):
                n_tok += int(n)
                print(json.dumps({"clip": name, "ids": row[:1 + int(n)].tolist(), "n_tokens": int(n), "logprob": float(sc),
                                  **seg(out, j)}), flush=True)
                if lines.get(j):
                    print(lines[j], flush=True)
            for j, ((name, _), row, n) in enumerate(zip(items, seqs, lens)):
                save_cross(name, feats_all[j] if args.save_cross_attentions else None, row[:1 + int(n)].tolist())
            continue
        if not beam:
            out = model.generate(fe(wave), max_length=args.max_length, **cons, **ts)
            ids = (out["sequences"] if ts else out).cpu()
            lines = stamps(feats_all, ids, None, wave.shape[1], range(len(items))) if args.timestamps else {}
            for j, ((name, _), row) in enumerate(zip(items, ids)):
                n_tok += row.numel() - 1
                print(json.dumps({"clip": name, "ids": row.tolist(), "n_tokens": int(row.numel() - 1), **seg(out, j)}),
                      flush=True)
                if lines.get(j):
                    print(lines[j], flush=True)
            for j, ((name, _), row) in enumerate(zip(items, ids)):
                save_cross(name, feats_all[j] if args.save_cross_attentions else None, row.tolist())
            continue
        R = args.num_return_sequences
        out = model.generate(fe(wave), max_length=args.max_length, num_beams=args.num_beams,
                             length_penalty=args.length_penalty, num_return_sequences=R, return_dict_in_generate=True,
                             **cons, **ts)
        seqs, scores, lens = out["sequences"].cpu(), out["sequences_scores"].cpu(), out["lengths"].cpu()
        lines = stamps(feats_all, seqs, lens, wave.shape[1], range(len(seqs))) if args.timestamps else {}
        for i, row in enumerate(seqs):
            n = int(lens[i])
            n_tok += n
            print(json.dumps({"clip": items[i // R][0], "rank": i % R, "ids": row[:1 + n].tolist(), "n_tokens": n,
                              "score": float(scores[i]), **seg(out, i)}), flush=True)
            if lines.get(i):
                print(lines[i], flush=True)
            if i % R == 0:  # (the best hypothesis of the clip)
                save_cross(items[i // R][0], feats_all[i // R] if args.save_cross_attentions else None, row[:1 + n].tolist())
    if args.save_cross_attentions:
        np.savez(args.save_cross_attentions, **{k: (np.asarray(v) if k == "clips" else v) for k, v in saved.items()})
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(json.dumps({"clips": len(clips), "seconds": round(dt, 4), "tokens": n_tok,
                      "tokens_per_s": round(n_tok / dt, 1) if dt > 0 else None}), flush=True)


if __name__ == "__main__":
    main()
