#!/usr/bin/env python3
"""Training entry point -- the loop of the reference's train.py (:55-176) with every parameterised layer's forward and backward on
the MI355X training kernels (speechseparation_amd/train.py).

Reference flow per epoch: for every training clip `train_infer` (STFT -> BSRNN -> iSTFT, L1 tri-loss, SDR; m_dataset.py:182-226),
`toBackward.backward()` (the loss, or -SDR with --loss_sdr), an optimizer step every `batch_size` clips (AdamW lr 1e-3,
weight_decay 1e-2; :50), then a validation pass without gradients and the checkpoints `model.pth` (best validation loss) /
`model-always.pth` (+ `optimizer*.pth`).  Same flags: --datapath --mini --batch_size --resume --loss_sdr.  --ragged runs the `batch_size` clips of an optimizer
step as one padded batch with one backward pass (speechseparation_amd.train.train_step_many) instead of clip by clip: the same gradients
and the same printed averages, to rounding.

Data: <datapath>/{train,val}/<clip>/{mixture,speech}.wav - the folders the reference trains from (`samples(args.datapath, 'train')` /
`'val'`, train.py:58,74; DnR layout of m_dataset.samples(), :8-19), as 16-bit / float WAV (the reference's .flac needs torchaudio, absent
here); a `tr/` folder (DnR v2's name) is used when there is no `train/`; --train-folder / --val-folder override, or --synthetic N clips of seeded noise (no dataset ships with the reference).
--rir DIR applies the reference's room-impulse-response augmentation (MyDataSet(with_rir=True), m_dataset.py:92-114) on the device: the WAV
files of DIR whose names contain `imp` are resampled from --rir_rate to 44.1 kHz (BSRNN.resample) and loaded into one
speechseparation_amd.augment.FirBank at start; a training clip is reverberated with probability --rir_prob, by the reference's draws on
the clip's index (augment.rir_draw) and with its chained channels (augment.reverb_pairs), all chosen clips of an optimizer step in one
convolution call per stage.  Without --rir nothing changes.
--remix DIR trains on the reference's MixDataSet (m_dataset.py:141-180) instead of on mixture / speech pairs: the dialog and background
WAV files under DIR (mix_samples' naming rules, plus the dialog-*.wav / background-*.wav that gendataset-separate.py writes) are loaded onto
one augment.SourceShelf on the device at start; an epoch is len(dialogs) items; every --batch_size items are drawn as the reference draws
them on the item's index (augment.remix_draw), mixed by ONE launch into the padded buffers of the ragged step (augment.remix_many) and
trained on in one backward pass (train_step_packed).  --remix_seconds / --remix_backgrounds: the reference's 50 and 4.  Validation still
reads --datapath's val split, when there is one.  Refused with --rir or --graph.  Without --remix nothing changes.
--batch_critic PATH [--adversarial] (with --ragged or --remix) adds a frozen Discriminator(2050)'s score to every clip's loss of the
ragged and packed steps - one library call scores all clips of the padded batch, each over its own frames
(speechseparation_amd.train.train_loss_ragged_critic, CommittedCritic.score_ragged / score_fixed_ragged); every clip needs 601 frames.
--critic PATH stays the per-clip step's option and is still refused with --ragged, --remix and --graph.
Not carried over: wandb logging, the discriminator argument (the reference's loop passes None; `speechseparation_amd.train.train_loss`
takes a `Discriminator`, and `train-discriminator.py` trains one), ReduceLROnPlateau (commented out in the reference loop; the rule is
`speechseparation_amd.train.ReduceLROnPlateau`) and its batch-size growth heuristic.  Under `torchrun` (one process per GPU) the clips are split over the ranks
and the gradients averaged before every optimizer step (data-parallel, RCCL).
"""
import argparse
import os
import random

import torch

from speechseparation_amd import audio, augment, train as hip_train, weights
from speechseparation_amd.bsrnn import BSRNN


def dataset(datapath, folder):
    """[(mixture path, speech path)] of m_dataset.samples(datapath, folder)."""
    base = os.path.join(datapath, folder)
    if not os.path.isdir(base):
        return []
    out = []
    for name in sorted(os.listdir(base)):
        d = os.path.join(base, name)
        if os.path.isdir(d) and os.path.exists(os.path.join(d, "mixture.wav")) and os.path.exists(os.path.join(d, "speech.wav")):
            out.append((os.path.join(d, "mixture.wav"), os.path.join(d, "speech.wav")))
    return out


def load_pair(item, device):
    """(mix, speech) [2, n] on the device; mono files are duplicated to two rows (m_dataset.load_waveform, :57-61)."""
    if isinstance(item, int):                                   # synthetic clip number `item`
        n = SYNTH_SAMPLES
        return (torch.from_numpy(weights.synth_waveform(2, n, seed=1000 + 2 * item)).to(device),
                torch.from_numpy(weights.synth_waveform(2, n, seed=1001 + 2 * item)).to(device))
    pair = []
    for path in item:
        w, _ = audio.load_wav(path)
        pair.append((torch.cat((w, w), 0) if w.shape[0] == 1 else w[:2]).to(device))
    n = min(pair[0].shape[1], pair[1].shape[1])
    return pair[0][:, :n].contiguous(), pair[1][:, :n].contiguous()


SYNTH_SAMPLES = 4 * 16000


def load_rirs(model, folder, rate, device):
    """(FirBank, first filter of every response, channels of every response) of the room impulse responses under `folder`: the WAV files
    whose names contain `imp` (m_dataset.py:76; sorted - os.listdir's order is the file system's), every channel resampled from `rate` to
    44.1 kHz on the device (the reference's Resample(16000, 44100), with this library's resampling kernel) as one filter."""
    names = sorted(x for x in os.listdir(folder) if "imp" in x and x.lower().endswith(".wav"))
    if not names:
        raise SystemExit("--rir: no WAV file with `imp` in its name under %s" % folder)
    filters, first, channels = [], [], []
    for name in names:
        w, _ = audio.load_wav(os.path.join(folder, name))
        w = model.resample(w.to(device), rate, 44100).cpu()
        if w.shape[1] > augment.MAX_TAPS:
            raise SystemExit("--rir: %s has %d taps at 44.1 kHz, the limit is %d" % (name, w.shape[1], augment.MAX_TAPS))
        first.append(len(filters))
        channels.append(w.shape[0])
        filters.extend(w[c].contiguous() for c in range(w.shape[0]))
    return augment.FirBank(model, filters), first, channels


def remix_files(base):
    """(dialog paths, background paths, FLAC files skipped) under `base`, recursively, by the rules of the reference's mix_samples
    (m_dataset.py:21-55): a dialog is a .wav whose path contains `lownoise`, or a file whose name starts with `speech.wav` or
    `speech_post_rnnoise.wav`; a background is a file named `sfx*`, `music*` or `vocalnoise*` that ends in .wav (what the reference's
    broken `endswith` evidently means); plus the `dialog-*.wav` / `background-*.wav` files gendataset-separate.py writes here.  Sorted
    (os.listdir's order is the file system's).  FLAC files are counted and skipped: audio.load_wav reads WAV only."""
    dialogs, backgrounds, flac = [], [], 0
    for root, dirs, names in os.walk(base):
        dirs.sort()
        for x in sorted(names):
            p = os.path.join(root, x)
            if x.lower().endswith(".flac"):
                flac += 1
            elif "lownoise" in p and p.endswith(".wav"):
                dialogs.append(p)
            elif x.startswith("speech.wav") or x.startswith("speech_post_rnnoise.wav") or (x.startswith("dialog-") and x.endswith(".wav")):
                dialogs.append(p)
            elif x.startswith(("sfx", "music", "vocalnoise", "background-")) and x.endswith(".wav"):
                backgrounds.append(p)
    return dialogs, backgrounds, flac


def load_shelf(base, length, device):
    """Every dialog and background under `base` on ONE augment.SourceShelf on the device (the shelf holds all of it: it has to fit)."""
    dialogs, backgrounds, flac = remix_files(base)
    if flac:
        print("--remix: %d FLAC files under %s skipped (WAV only)" % (flac, base))
    if not dialogs or not backgrounds:
        raise SystemExit("--remix: found %d dialogs and %d backgrounds under %s, need at least one of each (speech.wav / dialog-*.wav / "
                         "*lownoise*.wav; sfx*.wav / music*.wav / vocalnoise*.wav / background-*.wav)" % (len(dialogs), len(backgrounds), base))
    shelf = augment.SourceShelf(device)
    for paths, add in ((dialogs, shelf.add_dialog), (backgrounds, shelf.add_background)):
        for p in paths:
            w, _ = audio.load_wav(p)
            if w.shape[1] == length:
                raise SystemExit("--remix: %s has exactly the item's %d samples: the reference's random_resize raises there" % (p, length))
            add(w[:2].contiguous())
    return shelf


def build_parser():
    ap = argparse.ArgumentParser(description="Train a BSRNN model")
    ap.add_argument("--datapath", type=str, default=None, help="Path to the dataset")
    ap.add_argument("--mini", action="store_true", help="Use a small dataset")
    ap.add_argument("--batch_size", type=int, default=1, help="Batch size")
    ap.add_argument("--resume", action="store_true", help="Reload model")
    ap.add_argument("--train-folder", type=str, default=None, help="training split under --datapath (default: train, else tr)")
    ap.add_argument("--val-folder", type=str, default="val", help="validation split under --datapath")
    ap.add_argument("--loss_sdr", action="store_true", help="Use SDR as loss")
    ap.add_argument("--epochs", type=int, default=1, help="epochs to run (the reference loops until interrupted)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic training clips (and N // 4 + 1 for validation)")
    ap.add_argument("--seconds", type=float, default=4.0, help="length of the synthetic clips")
    ap.add_argument("--synthetic-weights", type=int, default=None, metavar="SEED", help="initial weights from the seeded generator instead of torch's init")
    ap.add_argument("--graph", action="store_true", help="replay each iteration as one hipGraph (speechseparation_amd.train.GraphedTrainStep): "
                    "single process, --batch_size 1, one graph per clip length (at most 4 lengths, other clips run launch by launch)")
    ap.add_argument("--ragged", action="store_true", help="run the clips of one optimizer step (--batch_size of them, or the epoch's tail) as one "
                    "padded batch with one backward pass (speechseparation_amd.train.train_step_many) instead of clip by clip")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--outdir", type=str, default=".")
    ap.add_argument("--rir", type=str, default=None, metavar="DIR", help="folder of room impulse responses (WAV files with `imp` in their names): "
                    "reverberate training clips on the device as the reference's MyDataSet(with_rir=True) does")
    ap.add_argument("--rir_prob", type=float, default=0.1, metavar="P", help="chance of a training clip being reverberated (the reference's 0.1)")
    ap.add_argument("--rir_rate", type=int, default=16000, metavar="HZ", help="sample rate the responses are taken to be at (the reference's 16000)")
    ap.add_argument("--remix", type=str, default=None, metavar="DIR", help="train on re-mixed items as the reference's MixDataSet makes them: the "
                    "dialog and background WAV files under DIR are held on the device, and every --batch_size items are mixed there in one launch")
    ap.add_argument("--remix_seconds", type=float, default=50.0, metavar="S", help="length of a re-mixed item at 44.1 kHz (the reference's 50)")
    ap.add_argument("--remix_backgrounds", type=int, default=4, metavar="N", help="backgrounds per re-mixed item (the reference's 4)")
    # (absent from the parsed arguments unless given: a run without them sees the arguments it always saw)
    ap.add_argument("--critic", type=str, default=argparse.SUPPRESS, metavar="PATH", help="state dict of a Discriminator(2050) (train-discriminator.py at its "
                    "default --n_fft 2048): committed once, its score of the model's output is added to every clip's loss as a constant "
                    "(clips need 601 frames)")
    ap.add_argument("--adversarial", action="store_true", default=argparse.SUPPRESS, help="with --critic: let the gradient flow through the frozen critic into the model "
                    "(score and dx from one library call, CommittedCritic.score_fixed)")
    ap.add_argument("--batch_critic", type=str, default=argparse.SUPPRESS, metavar="PATH", help="with --ragged or --remix: state dict of a "
                    "Discriminator(2050), committed once; every clip of a step gets its own score added to its loss, all clips in one library "
                    "call (CommittedCritic.score_ragged; with --adversarial score_fixed_ragged).  Clips need 601 frames")
    return ap


CRITIC_REFUSAL = ("--critic does not go with --graph, --ragged or --remix: the critic's term is part of the per-clip step only "
                  "(no graph capture of it, no ragged or packed step with a critic)")
BATCH_CRITIC_REFUSAL = ("--batch_critic goes with --ragged or --remix only, and not with --graph or --critic: it is the critic's term of the "
                        "ragged and packed steps (--critic is the per-clip step's)")
REMIX_REFUSAL = "--remix does not go with --rir or --graph: the reference's MixDataSet has no reverberation, and the items of a step are a ragged batch"


def parse_args(ap, argv=None):
    """The parsed arguments, or the parser's exit for combinations that are refused."""
    args = ap.parse_args(argv)
    if args.remix and (args.rir or args.graph):
        ap.error(REMIX_REFUSAL)
    if args.remix and (int(args.remix_seconds * 44100) <= 1024 or args.remix_backgrounds < 0):
        ap.error("--remix needs --remix_seconds of more than 1024 samples at 44.1 kHz and --remix_backgrounds >= 0")
    critic, adversarial = getattr(args, "critic", None), getattr(args, "adversarial", False)
    if critic and (args.graph or args.ragged or args.remix):
        ap.error(CRITIC_REFUSAL)
    batch_critic = getattr(args, "batch_critic", None)
    if batch_critic and (critic or args.graph or not (args.ragged or args.remix)):
        ap.error(BATCH_CRITIC_REFUSAL)
    if adversarial and not critic and not batch_critic:
        ap.error("--adversarial needs --critic PATH (or --batch_critic PATH with --ragged or --remix)")
    return args


def main(argv=None):
    global SYNTH_SAMPLES
    ap = build_parser()
    args = parse_args(ap, argv)
    SYNTH_SAMPLES = int(args.seconds * 16000)

    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    device = torch.device(args.device or "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)

    shelf = None
    if args.remix:
        remix_length = int(args.remix_seconds * 44100)
        shelf = load_shelf(args.remix, remix_length, device)
        train_set = list(range(shelf.n_dialogs))                 # an epoch is len(dialogs) items (MixDataSet.__len__)
        val_set = dataset(args.datapath, args.val_folder) if args.datapath else []
    elif args.synthetic:
        train_set, val_set = list(range(args.synthetic)), list(range(args.synthetic, args.synthetic + args.synthetic // 4 + 1))
    elif args.datapath:
        # the reference's live path reads `train` and `val` (train.py:58,74); DnR's own split is called `tr`
        tf = args.train_folder or ("train" if os.path.isdir(os.path.join(args.datapath, "train")) else "tr")
        train_set, val_set = dataset(args.datapath, tf), dataset(args.datapath, args.val_folder)
    else:
        ap.error("give --datapath DIR or --synthetic N")
    if args.mini:
        random.Random(0).shuffle(train_set)
        train_set, val_set = train_set[:10], val_set[:10]
    if not train_set:
        raise SystemExit("no training clips found under %s/{train,tr}/*/{mixture,speech}.wav (WAV copies of the reference's .flac; "
                         "--train-folder names another split)" % args.datapath)

    model = BSRNN().train()
    if args.synthetic_weights is not None:
        audio.load_model_weights(model, None, args.synthetic_weights)
    if args.resume:
        model.load_state_dict(torch.load(os.path.join(args.outdir, "model.pth"), weights_only=True))
    model = model.to(device)
    use_graph = args.graph and world == 1 and args.batch_size == 1 and not args.ragged
    if args.graph and not use_graph and rank == 0:
        print("--graph needs a single process and --batch_size 1: running launch by launch")
    optimizer = hip_train.AdamW(model.parameters(), lr=0.001, weight_decay=0.01, capturable=use_graph)
    graphs = {}                                                  # clip shape -> GraphedTrainStep
    if args.resume and os.path.exists(os.path.join(args.outdir, "optimizer.pth")):
        optimizer.load_state_dict(torch.load(os.path.join(args.outdir, "optimizer.pth"), weights_only=True))

    critic, adversarial = None, getattr(args, "adversarial", False)
    critic_path = getattr(args, "critic", None) or getattr(args, "batch_critic", None)      # (never both: parse_args)
    if critic_path:
        from speechseparation_amd.discriminator import Discriminator
        D = Discriminator(2050)
        D.load_state_dict(torch.load(critic_path, weights_only=True), strict=True)
        critic = D.to(device).commit(grad=adversarial)      # a snapshot: the module goes, the object stays for the run
        del D

    reverb = None
    if args.rir:
        bank, rir_first, rir_channels = load_rirs(model, args.rir, args.rir_rate, device)

        def reverb(indices, mixes):
            """the reference's draws for these training clips, applied to their mixtures in place: one convolution call per stage"""
            draws = [augment.rir_draw(idx, len(rir_first), rir_channels.__getitem__, args.rir_prob) for idx in indices]
            augment.reverb_pairs(bank, mixes, [d and (rir_first[d[0]] + d[1], rir_first[d[0]] + d[2]) for d in draws])

    best = 1.0e30
    for epoch in range(args.epochs):
        if rank == 0:
            print("Epoch", epoch)
        order = list(range(len(train_set)))
        random.Random(epoch).shuffle(order)                      # DataLoader(shuffle=True)
        order = order[: len(order) // world * world][rank::world]     # the same number of clips (and collectives) on every rank
        epoch_loss, epoch_sdr, batch_i = 0.0, 0.0, 0
        if shelf is not None:
            # the items of one optimizer step: the reference's draws on the host, one launch that mixes them, one backward pass
            for b0 in range(0, len(order), args.batch_size):
                specs = [augment.remix_draw(train_set[i], shelf, remix_length, args.remix_backgrounds) for i in order[b0:b0 + args.batch_size]]
                mix, speech, lengths, clip_rows = augment.remix_many(shelf, specs, remix_length)
                for loss, sdr in hip_train.train_step_packed_critic(model, optimizer, mix, speech, lengths, clip_rows, critic, adversarial,
                                                                    group=dist.group.WORLD if world > 1 else None, loss_sdr=args.loss_sdr):
                    batch_i += 1
                    epoch_loss += loss
                    epoch_sdr += sdr
            order = []
        elif args.ragged:
            # the clips of one optimizer step in one backward pass; the tail of the epoch is a smaller step (train.py:122-123)
            for b0 in range(0, len(order), args.batch_size):
                pairs = [load_pair(train_set[idx], device) for idx in order[b0:b0 + args.batch_size]]
                if reverb:
                    reverb(order[b0:b0 + args.batch_size], [mix for mix, _ in pairs])
                for loss, sdr in hip_train.train_step_many(model, optimizer, pairs, group=dist.group.WORLD if world > 1 else None,
                                                           loss_sdr=args.loss_sdr, discriminator=critic, adversarial=adversarial):
                    batch_i += 1
                    epoch_loss += loss
                    epoch_sdr += sdr
            order = []
        for idx in order:
            mix, speech = load_pair(train_set[idx], device)
            if reverb:
                reverb([idx], [mix])
            if use_graph and (tuple(mix.shape) in graphs or len(graphs) < 4):
                if tuple(mix.shape) not in graphs:
                    graphs[tuple(mix.shape)] = hip_train.GraphedTrainStep(model, optimizer, mix.shape[0], mix.shape[1], loss_sdr=args.loss_sdr)
                step = graphs[tuple(mix.shape)]
                loss = step(mix, speech)                         # loss, backward, optimizer step, zero_grad: one graph launch
                batch_i += 1
                epoch_loss += float(loss)
                epoch_sdr += float(step.last_sdr)
                continue
            loss, x_time = hip_train.train_loss(model, mix, speech, discriminator=critic, adversarial=adversarial)
            sdr = hip_train.sdr(x_time, speech[:, :x_time.shape[1]])
            (-sdr if args.loss_sdr else loss).backward()
            batch_i += 1
            epoch_loss += float(loss.detach())
            epoch_sdr += float(sdr.detach())
            if batch_i % args.batch_size == 0:
                if world > 1:
                    from speechseparation_amd.dist import all_reduce_gradients
                    all_reduce_gradients(model.parameters())
                optimizer.step()
                optimizer.zero_grad()
        if world > 1 and not args.ragged and shelf is None:
            from speechseparation_amd.dist import all_reduce_gradients
            all_reduce_gradients(model.parameters())
        optimizer.step()                                         # train.py:122-123: the tail of the epoch (--ragged: already stepped, no gradient is left)
        optimizer.zero_grad()
        if rank == 0:
            print("Epoch", epoch, "Loss", epoch_loss / max(1, batch_i), "sdr", epoch_sdr / max(1, batch_i))

        # validation without gradients: the inference path (bsrnn_evaluate = infer + train_infer's arithmetic on the device)
        model.eval()
        val_loss = val_sdr = 0.0
        with torch.no_grad():
            for item in val_set:
                mix, speech = load_pair(item, device)
                mtr = model.evaluate(mix, speech)
                val_loss += mtr["loss"]
                val_sdr += mtr["sdr"]
        model.train()
        if rank == 0:
            if val_set:
                print("Validation Loss", val_loss / len(val_set), "Validation SDR", val_sdr / len(val_set))
            state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
            if val_set and val_loss < best:
                print("...Saving")
                best = val_loss
                torch.save(state, os.path.join(args.outdir, "model.pth"))
                torch.save(optimizer.state_dict(), os.path.join(args.outdir, "optimizer.pth"))
            torch.save(state, os.path.join(args.outdir, "model-always.pth"))
            torch.save(optimizer.state_dict(), os.path.join(args.outdir, "optimizer-always.pth"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
