#!/usr/bin/env python3
"""Dialog / background section mining -- the reference's gendataset-separate.py (--input/--output/--channel) with the model on the
MI355X HIP path.

Reference flow (gendataset-separate.py:82-149): stream the input at 44.1 kHz in chunks of 1024 samples, run the separator on the chosen
channel, form per chunk 10 ln mean(dialog^2 / background^2) and 10 ln mean(chunk^2), and let a run-length state machine open and close
`dialog-{i}.wav` / `background-{i}.wav` files that receive the MIXTURE's chunks; `i` is the sample counter at the moment the writer opens,
(first_hop + 1) * 1024.  Here the whole file is separated in segments (`BSRNN.separate_long_ragged`), the per-hop figures come from one
kernel launch and the state machine is the library's (`speechseparation_amd.mining`).  The estimate and the mixture are compared aligned;
the reference compares its delayed stream output with the current chunk (include/bsrnn_hip.h).  A chunk whose estimate is all zero counts
as -inf dB instead of raising.  Extra flags: --input may repeat (several files are mined in one batch; each then writes into a
sub-directory of --output named after the file), --weights / --synthetic-weights SEED, --segment-frames, --device.
"""
import argparse
import os

import torch

from speechseparation_amd import audio, mining
from speechseparation_amd.bsrnn import BSRNN

MODEL_RATE = 44100                                  # add_basic_audio_stream(sample_rate=44100), gendataset-separate.py:83


def main(argv=None):
    ap = argparse.ArgumentParser(description="Mine dialog and background sections with the BSRNN model")
    ap.add_argument("--input", type=str, action="append", required=True, help="Input file (may repeat)")
    ap.add_argument("--output", type=str, required=True, help="Output dir")
    ap.add_argument("--channel", type=str, default="0", help="Channel to use")
    ap.add_argument("--weights", type=str, default="model.pth")
    ap.add_argument("--synthetic-weights", type=int, default=None, metavar="SEED")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--segment-frames", type=int, default=256, metavar="N",
                    help="separate N STFT frames at a time (bounded device memory); default 256")
    args = ap.parse_args(argv)
    channel = int(args.channel)

    model = BSRNN().eval()
    audio.load_model_weights(model, args.weights, args.synthetic_weights)
    model = model.to(args.device)

    clips = []
    for path in args.input:
        waveform, sr = audio.load_wav(path)
        if not 0 <= channel < waveform.shape[0]:
            raise SystemExit("%s has %d channels, --channel %d" % (path, waveform.shape[0], channel))
        clips.append(audio.resample(waveform[channel:channel + 1], sr, MODEL_RATE)[0].contiguous())

    with torch.no_grad(), torch.cuda.device(args.device):
        mined = mining.mine(model, clips, segment_frames=args.segment_frames)

    for path, clip, m in zip(args.input, clips, mined):
        outdir = args.output if len(args.input) == 1 else os.path.join(args.output, os.path.splitext(os.path.basename(path))[0])
        os.makedirs(outdir, exist_ok=True)
        for s in m.sections[0]:
            a, b = s.samples
            audio.save_wav(os.path.join(outdir, "%s-%d.wav" % (s.name, (s.first_hop + 1) * mining.HOP)), clip[a:b].unsqueeze(0), MODEL_RATE)
        print("%s: %d hops, %d dialog and %d background sections" % (
            path, m.activity.shape[1], sum(s.kind == mining.DIALOG for s in m.sections[0]),
            sum(s.kind == mining.BACKGROUND for s in m.sections[0])))


if __name__ == "__main__":
    main()
