#!/usr/bin/env python3
"""Streaming separation entry point -- same command line as the reference's
infer-streaming.py (--input/--output/--name), with the whole per-chunk loop
(infer-streaming.py:104-147: slide buffer, rfft, forward_recurrent, irfft, 2-slot overlap-add)
resident on the MI355X: one `StreamingSeparator.step` per 1024-sample chunk at 44.1 kHz, or with
`--block N` one `StreamingSeparator.process` per N chunks (same output to rounding, far fewer launches).  A file at another rate is brought to
44.1 kHz on the host (`audio.resample`, the default) or, with `--device-resample`, on the device through a `Resampler`.

The reference also dumps the traced model for its LADSPA plugin (hello.onnx, :74); the
counterpart here is the flat weight file `hello.bsrnnw` that speech_separator_ladspa.so loads
(the model name is recorded next to it in hello.name).  ONNX export itself is out of scope
for this round.
"""
import argparse
import time

import torch

from speechseparation_amd import audio
from speechseparation_amd.bsrnn import BSRNN, Resampler, StreamingSeparator

STREAM_RATE = 44100      # infer-streaming.py:78
CHUNK = 1024


def main(argv=None):
    ap = argparse.ArgumentParser(description="Infer the BSRNN model")
    ap.add_argument("--input", type=str, required=True, help="Input file")
    ap.add_argument("--output", type=str, required=True, help="Output file")
    ap.add_argument("--name", type=str, default="bsrnn", help="Model name")
    ap.add_argument("--weights", type=str, default="model-always.pth")
    ap.add_argument("--synthetic-weights", type=int, default=None, metavar="SEED")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--export", type=str, default="hello.bsrnnw")
    ap.add_argument("--block", type=int, default=1, metavar="N",
                    help="hops per library call: 1 = one step per 1024-sample chunk (the reference's loop), N > 1 = N hops per "
                         "StreamingSeparator.process call")
    ap.add_argument("--device-resample", action="store_true",
                    help="convert a file at another rate to 44.1 kHz on the device (Resampler) instead of on the host (audio.resample)")
    args = ap.parse_args(argv)

    torch.set_grad_enabled(False)
    model = BSRNN().eval()
    audio.load_model_weights(model, args.weights, args.synthetic_weights)
    model = model.to(args.device)
    if args.export:
        model.save_flat(args.export)
        with open(args.export.rsplit(".", 1)[0] + ".name", "w") as f:
            f.write("model=%s\n" % args.name)
        print("Flat weight file dumped")

    waveform, sr = audio.load_wav(args.input)
    if not args.device_resample:
        waveform = audio.resample(waveform, sr, STREAM_RATE)
    if waveform.shape[0] == 1:
        waveform = torch.cat((waveform, waveform), 0)
    waveform = waveform[:2].to(args.device)
    if args.device_resample and sr != STREAM_RATE:
        # the file as one block through the streaming resampler, then what the block's end still owes
        with torch.cuda.device(args.device):
            rs = Resampler(model, 2, sr, STREAM_RATE)
            waveform = torch.cat((rs.process(waveform.contiguous()), rs.flush()), 1)

    sep = StreamingSeparator(model, channels=2, device=args.device)
    n_chunks = waveform.shape[1] // CHUNK                 # a short tail chunk ends the stream (:108)
    outs = []
    t = time.time()
    if args.block < 1:
        ap.error("--block must be at least 1")
    if args.block == 1:
        for i in range(n_chunks):
            outs.append(sep.step(waveform[:, i * CHUNK:(i + 1) * CHUNK].contiguous()))
    else:
        sep.reserve(min(args.block, max(n_chunks, 1)))
        for i in range(0, n_chunks, args.block):
            outs.append(sep.process(waveform[:, i * CHUNK:min(i + args.block, n_chunks) * CHUNK]))
    torch.cuda.synchronize()
    elapsed = time.time() - t
    out = torch.cat(outs, 1) if outs else torch.zeros((2, 0))
    audio.save_wav(args.output, out, STREAM_RATE)
    print(f"Elapsed {elapsed}")


if __name__ == "__main__":
    main()
