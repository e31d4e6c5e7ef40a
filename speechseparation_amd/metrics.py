"""Host mirror of the reference's validation helpers (m_dataset.py:182-226), over the HIP path.

`train_infer(model, discriminator, sample)` keeps the reference's call shape and return tuple
`(loss, sdr, sdr2, sdr3)` so that a validation loop written against m_dataset.py (train.py:137-150) runs
unchanged; the arithmetic itself is one C-ABI call (`bsrnn_evaluate`): separation, the clean signal's STFT
and every reduction stay on the device, only the eight numbers come back.  With a `Discriminator`
(speechseparation_amd/discriminator.py) its score of the model's output is added to the loss, as m_dataset.py:205-213 does.
The backward pass lives in speechseparation_amd/train.py.
"""
import torch


def evaluate(model, mix, speech, return_estimate=False):
    """mix, speech: [R, n] (or the DataLoader's [1, R, n]) -> dict of the metrics (BSRNN.evaluate)."""
    if mix.dim() == 3 and mix.shape[0] == 1:
        mix, speech = mix.squeeze(0), speech.squeeze(0)        # m_dataset.py:184-185
    return model.evaluate(mix, speech, return_estimate=return_estimate)


def evaluate_many(model, pairs, max_rows=64, max_padding=0.25):
    """pairs: a list of (mix, speech), each [n] or [ch, n], of different lengths -> the per-pair metric dicts in input order, from a few
    batched calls (BSRNN.evaluate_many -> bsrnn_evaluate_ragged): each pair is a clip, evaluated as `evaluate` evaluates it alone."""
    return model.evaluate_many(pairs, max_rows=max_rows, max_padding=max_padding)


def evaluate_many_long(model, pairs, segment_frames=256, max_rows=64):
    """evaluate_many for pairs that are long and of very different lengths -> the per-pair metric dicts in input order, from one
    bsrnn_evaluate_long_ragged call per bucket of at most max_rows rows (BSRNN.evaluate_many_long): bounded memory, rows retire."""
    return model.evaluate_many_long(pairs, segment_frames=segment_frames, max_rows=max_rows)


def train_infer(model, discriminator, sample, lossfn=None, verbose=False):
    """m_dataset.py:202-226.  sample = (waveform, waveform_speech), each [1, R, n].  lossfn must be the reference's
    L1Loss(reduction='mean') (train.py:54) or None.  Returns 0-dim tensors like the reference (its validation loop calls
    `.item()` on them, train.py:140-144); they carry no graph: inference only.  discriminator: None, a Discriminator(2050) or its CommittedCritic (Discriminator.commit()) whose
    score of the model's output (under no_grad) is added to the loss; the clip then needs 601 frames (614 400 samples).  sdr, sdr2 and
    sdr3 do not depend on it.  (The reference's loss then has shape [1]; `.item()` serves both.)"""
    if discriminator is not None:
        from .discriminator import CommittedCritic, Discriminator
        if not isinstance(discriminator, (Discriminator, CommittedCritic)):
            raise NotImplementedError("the discriminator must be a speechseparation_amd Discriminator (or None), got %s" % type(discriminator).__name__)
    if lossfn is not None and not (isinstance(lossfn, torch.nn.L1Loss) and lossfn.reduction == "mean"):
        raise ValueError("only the reference's L1Loss(reduction='mean') is implemented on the device")
    m = evaluate(model, sample[0], sample[1])
    if verbose:
        print(" ".join("%s=%.4f" % kv for kv in m.items()))
    out = tuple(torch.tensor(m[k], dtype=torch.float64) for k in ("loss", "sdr", "input_sdr", "sisdr"))
    if discriminator is None:
        return out
    mix = sample[0].squeeze(0) if sample[0].dim() == 3 and sample[0].shape[0] == 1 else sample[0]
    if isinstance(discriminator, CommittedCritic):             # one library call on the interleaved spectrum, no reorder copy
        dev = model._device_for(mix)
        with torch.no_grad():
            score = discriminator.score(model.forward(model.stft(mix.to(dev))), interleaved=True)
        return (out[0] + score.to(torch.float64).cpu().reshape(()),) + out[1:]
    with torch.no_grad():                                      # m_dataset.py:205-208
        score = discriminator(critic_input(model, mix))
    return (out[0] + score.detach().to(torch.float64).cpu().reshape(()),) + out[1:]


def critic_input(model, mix):
    """`x_freq2` of m_dataset.py:205 for the mixture `mix` [R, n]: the model's output spectrum in the reference's channel order (all real
    parts, then all imaginary parts) - a permutation of the library's interleaved [R, 2050, T], on the device."""
    from .discriminator import reference_channel_order
    dev = model._device_for(mix)
    return reference_channel_order(model.forward(model.stft(mix.to(dev))))
