#!/usr/bin/env python3
"""Validation pass over (mixture, clean speech) file pairs -- the `with torch.no_grad()` block of the reference's
train.py:132-150 without the training around it: `train_infer(model, None, sample, l1loss)` per pair, then the averages
the reference prints ("Validation Loss", "Validation SDR") plus the SI-SDR it logs.  Separation, both STFTs and every
reduction run on the MI355X: one bsrnn_evaluate call per pair, or with --batch-rows N the pairs batched by length into a few
bsrnn_evaluate_ragged calls of at most N rows (the same per-pair numbers to rounding, then the same averages).  With
--segment-frames S the pairs go through bsrnn_evaluate_long_ragged instead, in segments of S frames: recordings of any and of very
different lengths in bounded device memory, at most --batch-rows (64 when that is 0) rows per call.

    validate.py --pairs mix1.wav speech1.wav [mix2.wav speech2.wav ...] [--weights model-always.pth] [--batch-rows 64] [--segment-frames 256]
"""
import argparse

import torch

from speechseparation_amd import audio, metrics
from speechseparation_amd.bsrnn import BSRNN


def main(argv=None):
    ap = argparse.ArgumentParser(description="Validate the BSRNN model on (mixture, speech) pairs")
    ap.add_argument("--pairs", type=str, nargs="+", required=True, metavar="WAV", help="mixture and clean file, alternating")
    ap.add_argument("--weights", type=str, default="model-always.pth")
    ap.add_argument("--synthetic-weights", type=int, default=None, metavar="SEED")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--batch-rows", type=int, default=0, metavar="N",
                    help="0: one call per pair; N > 0: pairs of similar length batched into calls of at most N rows")
    ap.add_argument("--segment-frames", type=int, default=0, metavar="S",
                    help="0: whole clips; S > 0: long-form evaluation in segments of S frames, --batch-rows (64 when 0) rows per call")
    args = ap.parse_args(argv)
    if len(args.pairs) % 2:
        ap.error("--pairs needs an even number of files")
    if args.segment_frames < 0:
        ap.error("--segment-frames must not be negative")
    batched = args.batch_rows > 0 or args.segment_frames > 0

    torch.set_grad_enabled(False)
    model = BSRNN().eval()
    audio.load_model_weights(model, args.weights, args.synthetic_weights)
    model = model.to(args.device)
    l1loss = torch.nn.L1Loss(reduction="mean")

    val_loss = val_sdr = val_sdr2 = val_sisdr = 0.0
    n_pairs = len(args.pairs) // 2
    loaded = []
    for mix_path, speech_path in zip(args.pairs[0::2], args.pairs[1::2]):
        mix, _ = audio.load_wav(mix_path)
        speech, _ = audio.load_wav(speech_path)
        if mix.shape[0] == 1:                                       # mono -> two identical rows, as infer.py:26-27
            mix, speech = torch.cat((mix, mix), 0), torch.cat((speech, speech), 0)
        n = min(mix.shape[1], speech.shape[1])
        if batched:
            loaded.append((mix[:, :n], speech[:, :n]))
            continue
        sample = (mix[None, :, :n].to(args.device), speech[None, :, :n].to(args.device))
        loss, sdr, sdr2, sisdr = metrics.train_infer(model, None, sample, l1loss)
        val_loss += loss.item(); val_sdr += sdr.item(); val_sdr2 += sdr2.item(); val_sisdr += sisdr.item()
    if batched:
        with torch.cuda.device(args.device):
            if args.segment_frames > 0:
                results = metrics.evaluate_many_long(model, loaded, segment_frames=args.segment_frames, max_rows=args.batch_rows or 64)
            else:
                results = metrics.evaluate_many(model, loaded, max_rows=args.batch_rows)
            for m in results:
                val_loss += m["loss"]; val_sdr += m["sdr"]; val_sdr2 += m["input_sdr"]; val_sisdr += m["sisdr"]
    print("Validation Loss", val_loss / n_pairs, "Validation SDR", val_sdr / n_pairs)
    print("Validation input SDR", val_sdr2 / n_pairs, "Validation SI-SDR", val_sisdr / n_pairs)


if __name__ == "__main__":
    main()
