#!/usr/bin/env python3
"""Inference job: frame and clip embeddings from a Wav2Vec2 model (the reference's ``Wav2Vec2Model.call(...,
training=False)``, speech_jobs/wav2vec2_dist.py V:768-825, with the masked mean over time of V:1031-1042).

Loads a checkpoint (``--resume_from``: a ``save_checkpoint`` or ``save_weights`` file; without one the model keeps its
seeded initialisation), pads the ``--wav`` clips (16-bit PCM mono 16 kHz) to the longest of them - or, without one, takes
``--batch_size`` dummy clips of ``--seconds``, every second one cut to 60 % - builds the frame mask
(``wav2vec2.frame_attention_mask``) and runs the masked forward once.  Prints one JSON line with the three output
shapes and the frames per clip, then one timing line; ``--out PREFIX`` writes PREFIX.last_hidden_state.npy and
PREFIX.pooled_output.npy (float32).
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
    parser = argparse.ArgumentParser(description="Wav2Vec2 embeddings of padded clips (masked forward, mean pooling)")
    parser.add_argument("--model_size", default="base", choices=["tiny", "small", "base"])
    parser.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    parser.add_argument("--resume_from", default=None, help="checkpoint to load the weights from")
    parser.add_argument("--wav", action="append", default=[], help="16-bit PCM mono 16 kHz .wav file (repeatable)")
    parser.add_argument("--batch_size", type=int, default=2, help="number of dummy clips when no --wav is given")
    parser.add_argument("--seconds", type=float, default=2.0, help="length of the dummy clips")
    parser.add_argument("--out", default=None, help="prefix of the .npy files to write")
    args = parser.parse_args(argv)

    import numpy as np
    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, wav2vec2, whisper

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    model = wav2vec2.create_full_model("pretraining", args.model_size, device=device, precision=args.precision)
    if args.resume_from:
        train.load_weights(model, args.resume_from)
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
    torch.cuda.synchronize()
    t0 = time.time()
    out = model(audio, attention_mask=mask, pool="mean", training=False)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(json.dumps({"clips": [name for name, _ in clips], "frames": [int(x) for x in mask.sum(1).tolist()],
                      "last_hidden_state": list(out["last_hidden_state"].shape),
                      "extract_features": list(out["extract_features"].shape),
                      "pooled_output": list(out["pooled_output"].shape)}), flush=True)
    if args.out:
        np.save(args.out + ".last_hidden_state.npy", out["last_hidden_state"].float().cpu().numpy())
        np.save(args.out + ".pooled_output.npy", out["pooled_output"].cpu().numpy())
    print(json.dumps({"clips": len(clips), "samples": T_in, "seconds": round(dt, 4)}), flush=True)


if __name__ == "__main__":
    main()
