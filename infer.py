#!/usr/bin/env python3
"""Offline separation entry point -- same command line and outputs as the reference's infer.py
(--input/--output; writes the separated file, prints "Separation dB", writes the five re-mix
files mix_{100,90,50,20,-100}.wav), with the model on the MI355X HIP path.

Reference flow (infer.py:17-79): load model-always.pth -> load audio, mono duplicated to two
rows (:26-27) -> STFT (:29-33) -> BSRNN.forward (:34) -> iSTFT (:35-37) -> save -> report.
Here STFT -> forward -> iSTFT is one fused device call (`BSRNN.separate`), numerically the same
sandwich.  Extra flags: --weights (checkpoint or flat file), --synthetic-weights SEED (no
trained weights ship with the reference), --device, --outdir for the re-mix files, --segment-frames N
(long files: the waveform stays on the host and is separated N frames at a time in bounded device
memory, `BSRNN.separate_long`; everything after the separation is unchanged), --model-rate HZ (a file at another rate is
converted to HZ on the device, separated and converted back, `BSRNN.separate_at_rate`; off by default: the reference runs
the model at whatever rate the file has).
"""
import argparse
import os

import numpy as np
import torch

from speechseparation_amd import audio
from speechseparation_amd.bsrnn import BSRNN

# (file suffix, gain of the non-dialog residue mixed back in; None = residue only)   infer.py:49-79
REMIXES = (("100", 0.0), ("90", 0.3), ("50", 0.5), ("20", 0.8), ("-100", None))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Infer the BSRNN model")
    ap.add_argument("--input", type=str, required=True, help="Input file")
    ap.add_argument("--output", type=str, required=True, help="Output file")
    ap.add_argument("--weights", type=str, default="model-always.pth")
    ap.add_argument("--synthetic-weights", type=int, default=None, metavar="SEED")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--outdir", type=str, default=".")
    ap.add_argument("--segment-frames", type=int, default=None, metavar="N",
                    help="separate N STFT frames at a time (bounded device memory, for long files); default: the whole file in one call")
    ap.add_argument("--model-rate", type=int, default=0, metavar="HZ",
                    help="the rate the model was trained at (44100): a file at another rate is resampled to it on the device, separated "
                         "and resampled back; default 0: run the model at the file's rate, as the reference does")
    args = ap.parse_args(argv)

    torch.set_grad_enabled(False)
    model = BSRNN().eval()
    audio.load_model_weights(model, args.weights, args.synthetic_weights)
    model = model.to(args.device)

    waveform, sr = audio.load_wav(args.input)
    if waveform.shape[0] == 1:                      # mono -> two identical rows
        waveform = torch.cat((waveform, waveform), 0)
    orig_peak = waveform.max().item()

    if args.model_rate and args.model_rate != sr:
        dialog = model.separate_at_rate(waveform.to(args.device), sr, args.model_rate, args.segment_frames).cpu()
    elif args.segment_frames is None:
        dialog = model.separate(waveform.to(args.device)).cpu()
    else:
        with torch.cuda.device(args.device):
            dialog = model.separate_long(waveform, args.segment_frames)
    waveform = waveform[:, :dialog.shape[1]]
    audio.save_wav(args.output, dialog, sr)

    signal_power = np.sum(np.square(waveform.numpy()))
    remaining_power = np.sum(np.square((waveform - dialog).numpy()))
    print("Separation dB", 10 * np.log(signal_power / remaining_power))     # natural log, as the reference prints it

    residue = waveform - dialog
    for tag, gain in REMIXES:
        mix = residue if gain is None else dialog + gain * residue
        mix = mix * orig_peak / mix.max()
        audio.save_wav(os.path.join(args.outdir, "mix_%s.wav" % tag), mix, sr)


if __name__ == "__main__":
    main()
