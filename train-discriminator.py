#!/usr/bin/env python3
"""Critic training entry point -- the loop of the reference's train-discriminator.py (:23-126) on the MI355X kernels
(speechseparation_amd/discriminator.py: every Conv1d layer forward and backward through bsrnn_critic_conv_*).

Reference flow per epoch: for every training clip a random scale in [0.02, 1], the spectra of the mixture and of the clean speech as
`cat(real, imag)`, `loss = score_speech + (1 - score_orig)`, `loss.backward()`, an optimizer step every `batch_size` clips (and one at the
end of the epoch); `Adam(lr=1e-4)` - here the project's AdamW(lr=1e-4, weight_decay=0), which is Adam's arithmetic - under
ReduceLROnPlateau('min', patience=8, factor=0.8) stepped with the epoch's mean loss; then a validation pass without gradients summing
`score_speech - score_orig`, and `discriminator.pth` whenever that sum exceeds the best so far (the first validation always saves: the
reference starts its best at 0 and so never saves a critic whose sums stay negative).  Same flags:
--datapath --mini --batch_size --resume --loss_sdr; as in the reference the last two are accepted and do nothing.

--n_fft chooses the analysis.  4096 is the reference's: `critic_spectrum` (the 4096-point transform, hop 1024, 4098 channels) and the
default `Discriminator()`, so a `discriminator.pth` of the reference's script trains on and validates here.  2048, the default, is the
library's `train.stft` (hop 1024, 2050 channels) and `Discriminator(2050)` - the size the reference's own `train_infer` feeds its critic,
and the one `metrics.train_infer` / `train.train_loss` can use.

Data: <datapath>/{train,val}/<clip>/{mixture,speech}.wav as train.py reads them (a `tr/` resp. `cv/` folder is used when those are
missing), or --synthetic N clips of seeded noise.  A clip needs 614 400 samples (601 frames, the critic's shortest input); shorter ones
are skipped with a note.  --epochs N stops after N epochs (default: the reference's endless loop).
"""
import argparse
import os
import random

import torch

from speechseparation_amd import audio, train as hip_train, weights
from speechseparation_amd.discriminator import MIN_FRAMES, Discriminator, critic_spectrum, reference_channel_order

MIN_SAMPLES = (MIN_FRAMES - 1) * 1024


def dataset(datapath, folders):
    """[(mixture path, speech path)] of the first of `folders` that exists under datapath (m_dataset.samples)."""
    for folder in folders:
        base = os.path.join(datapath, folder)
        if not os.path.isdir(base):
            continue
        out = []
        for name in sorted(os.listdir(base)):
            d = os.path.join(base, name)
            if os.path.exists(os.path.join(d, "mixture.wav")) and os.path.exists(os.path.join(d, "speech.wav")):
                out.append((os.path.join(d, "mixture.wav"), os.path.join(d, "speech.wav")))
        return out
    return []


def load_pair(item, device):
    """(mix, speech) [2, n] on the device; a synthetic clip is numbered, mono files are duplicated to two rows."""
    if isinstance(item, int):
        return tuple(torch.from_numpy(weights.synth_waveform(2, MIN_SAMPLES, seed=3000 + 2 * item + k)).to(device) for k in range(2))
    pair = []
    for path in item:
        w, _ = audio.load_wav(path)
        pair.append((torch.cat((w, w), 0) if w.shape[0] == 1 else w[:2]).to(device))
    n = min(pair[0].shape[1], pair[1].shape[1])
    return pair[0][:, :n].contiguous(), pair[1][:, :n].contiguous()


def spectra(item, device, rng, n_fft=2048):
    """The two critic inputs of a clip (train-discriminator.py:59-68), or None for a clip that is too short."""
    mix, speech = load_pair(item, device)
    if mix.shape[1] < MIN_SAMPLES:
        return None
    scale = rng.uniform(0.02, 1.0)
    if n_fft == 4096:
        return tuple(critic_spectrum(w, scale) for w in (mix, speech))
    return tuple(reference_channel_order(hip_train.stft(w * scale)) for w in (mix, speech))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the BSRNN critic")
    ap.add_argument("--datapath", type=str, default=None, help="Path to the dataset")
    ap.add_argument("--mini", action="store_true", help="Use a small dataset")
    ap.add_argument("--batch_size", type=int, default=1, help="Batch size")
    ap.add_argument("--resume", action="store_true", help="Reload model (accepted and unused, as in the reference)")
    ap.add_argument("--loss_sdr", action="store_true", help="Use SDR as loss (accepted and unused, as in the reference)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic training clips (and N // 4 + 1 for validation)")
    ap.add_argument("--epochs", type=int, default=0, metavar="N", help="stop after N epochs (default 0: loop until interrupted, as the reference)")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--outdir", type=str, default=".")
    ap.add_argument("--seed", type=int, default=0, help="seed of the clip order and of the random scales")
    ap.add_argument("--n_fft", type=int, choices=(2048, 4096), default=2048,
                    help="the analysis: 4096 = the reference's transform and its Discriminator() of 4098 channels; 2048 = train.stft and Discriminator(2050)")
    args = ap.parse_args(argv)
    if args.synthetic:
        train_set, val_set = list(range(args.synthetic)), list(range(args.synthetic, args.synthetic + args.synthetic // 4 + 1))
    elif args.datapath:
        train_set, val_set = dataset(args.datapath, ("train", "tr")), dataset(args.datapath, ("val", "cv"))
    else:
        ap.error("give --datapath DIR or --synthetic N")
    if args.mini:
        train_set, val_set = train_set[:10], val_set[:10]
    if not train_set:
        raise SystemExit("no training clips found")
    if not torch.cuda.is_available():
        raise SystemExit("train-discriminator.py needs a GPU: the critic's kernels have no CPU fallback")
    device = torch.device(args.device)
    rng = random.Random(args.seed)
    torch.manual_seed(args.seed)
    if args.n_fft == 4096:
        print("4096-point STFT (hop 1024) of the library: Discriminator() of 4098 channels, the reference's analysis")
        model = Discriminator().to(device)
    else:
        print("2048-point STFT (hop 1024) of the library: Discriminator(2050), not the reference's 4096-point / 4098-channel analysis")
        model = Discriminator(2050).to(device)
    optimizer = hip_train.AdamW(model.parameters(), lr=1e-4, weight_decay=0)
    scheduler = hip_train.ReduceLROnPlateau(optimizer, "min", patience=8, factor=0.8)
    epoch, best = 0, None
    while args.epochs <= 0 or epoch < args.epochs:
        print("Epoch", epoch)
        order = list(train_set)
        rng.shuffle(order)
        batch, epoch_loss = 0, 0.0
        for item in order:
            pair = spectra(item, device, rng, args.n_fft)
            if pair is None:
                print("skipped (shorter than %d samples):" % MIN_SAMPLES, item)
                continue
            x_mix, x_speech = pair
            loss = model(x_speech) + (1 - model(x_mix))          # maximize score_orig, minimize score_speech
            loss.backward()
            epoch_loss += loss.item()
            batch += 1
            if batch % max(1, args.batch_size) == 0:
                optimizer.step()
                optimizer.zero_grad()
        optimizer.step()                                          # (the reference steps once more at the end of the epoch; without gradients a no-op)
        optimizer.zero_grad()
        mean = epoch_loss / max(1, batch)
        print("Epoch", epoch, "Loss", mean, "lr", scheduler.get_last_lr())
        scheduler.step(mean)
        epoch += 1
        with torch.no_grad():
            model.eval()
            val_loss = 0.0
            for item in val_set:
                pair = spectra(item, device, rng, args.n_fft)
                if pair is None:
                    continue
                val_loss += (model(pair[1]) - model(pair[0])).item()
            print("Validation Loss", val_loss / max(1, len(val_set)))
            if best is None or val_loss > best:
                best = val_loss
                torch.save(model.state_dict(), os.path.join(args.outdir, "discriminator.pth"))
        model.train()


if __name__ == "__main__":
    main()
