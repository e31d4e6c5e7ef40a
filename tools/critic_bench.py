#!/usr/bin/env python3
"""Times the critic's kernels (speechseparation_amd/discriminator.py) beside stock torch on the same device: every layer's forward,
dW / db and dx, and the whole critic step (two forwards, the loop's loss, backward), at 8 s and 60 s clips (44.1 kHz, hop 1024) for
in_channels 2050 and 4098.  Medians of `--reps` runs after `--warmup`, device events around each run, nothing else on the GPU.  Beside
every figure the two floors it sits between: the kernel's FLOP count over the 155 TF f32 matrix rate and, for the first layer, its weight
bytes over HBM bandwidth (about 6.3 TB/s).

    python tools/critic_bench.py > profiles/critic_bench.txt

`--score` times the committed critic instead (Discriminator.commit(), bsrnn_critic_score) at the same four shapes, beside the exact
first-layer forward alone (bsrnn_critic_conv_forward) and the module's no_grad __call__: `--rounds` medians of `--reps` runs each, the
median of the medians and their spread (lowest .. highest).  The score is timed as the library call it is - all four layers, the tail and,
under the default range policy, the wait for the guard word - and once more under the deferred policy (asynchronous).  Its rate counts
the first layer's FLOPs over the whole call, against the 833 TF the f16 matrix pipe offers a three-term product.

    python tools/critic_bench.py --score > profiles/critic_score_bench.txt

`--grad` times the committed critic's score with its gradient (Discriminator.commit(grad=True), bsrnn_critic_score_grad: one call) at the
same four shapes, beside the adversarial path it replaces, run in the same session: reference_channel_order of the interleaved spectrum,
Discriminator.score_fixed, backward to x (the exact kernels through autograd, the first layer's dW formed and dropped).  Also the first
layer's dx alone on both paths (bsrnn_critic_layer1_dx; bsrnn_critic_conv_backward with and without dx, the difference).  Same method as
`--score`.  The last line of every shape says whether score_grad is faster than the path it replaces by more than both spreads together.

    python tools/critic_bench.py --grad > profiles/critic_grad_bench.txt

`--ragged` times the committed critic on a padded batch (bsrnn_critic_score_grad_ragged / _score_ragged: one call for all clips) at 2050
channels, interleaved order, 32 stereo clips with lengths spread evenly over 601 .. 793 frames and the same batch at 2154 frames (50 s
items, all equal), beside the only route without it, run in the same session: per clip a contiguous copy of the clip's rows and
score_grad / score, looped.  Same method as `--score`.  The last line of every shape says whether the one-call form is slower than the
loop by more than both spreads together.  Then the step time of train_step_packed on the first batch with and without the adversarial
term.

    python tools/critic_bench.py --ragged > profiles/critic_ragged_bench.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechseparation_amd import _native, train as hip_train                      # noqa: E402
from speechseparation_amd.discriminator import WIDTHS, Discriminator, conv_layout, frames_out     # noqa: E402

F32_MATRIX_TF, HBM_TBS = 155.0, 6.3
F16X3_TF = 833.0                          # 2.5 PF of dense f16 over three terms


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def rounds_of(fn, warmup, reps, rounds):
    """Median of `rounds` medians and their lowest and highest."""
    m = sorted(timed(fn, warmup, reps) for _ in range(rounds))
    return statistics.median(m), m[0], m[-1]


def score_bench(args, dev, lib, ctx, p):
    from speechseparation_amd.discriminator import score_layout
    print("critic_bench --score: %s; %d medians of %d runs after %d warm-up runs each: median of the medians (lowest .. highest), ms" % (
        torch.cuda.get_device_name(0), args.rounds, args.reps, args.warmup))
    for ch in args.channels:
        D = Discriminator(ch).to(dev)
        cc = D.commit()
        w, b = D.layers[0].weight.detach(), D.layers[0].bias.detach()
        for sec in args.seconds:
            T = max(601, 1 + int(sec * 44100) // 1024)
            To = frames_out(T)
            x = torch.randn(2, ch, T, device=dev)
            y = torch.empty(2, WIDTHS[0], To, device=dev)
            flop = 2.0 * 2 * To * WIDTHS[0] * ch * 16
            lay = score_layout(ch, 2, T)
            print("\nin_channels %d, T = %d frames, C = 2: first layer %.1f GFLOP, %d K slabs of %d channels; image %.0f MB + snapshot %.0f MB" % (
                ch, T, flop * 1e-9, lay["slabs"], lay["ch_per_slab"], lay["image_bytes"] * 1e-6, lay["snapshot_bytes"] * 1e-6))

            def module():
                with torch.no_grad():
                    D(x)
            rows = [("bsrnn_critic_score (policy exact)", lambda: cc.score(x), native_policy(lib, ctx, _native.RANGE_EXACT)),
                    ("bsrnn_critic_score (policy deferred)", lambda: cc.score(x), native_policy(lib, ctx, _native.RANGE_DEFERRED)),
                    ("bsrnn_critic_score, interleaved x", lambda: cc.score(x, interleaved=True), native_policy(lib, ctx, _native.RANGE_DEFERRED)),
                    ("exact first-layer forward alone", lambda: _native.check(lib.bsrnn_critic_conv_forward(ctx, p(x), p(w), p(b), p(y), 2, ch, T, WIDTHS[0], 1, None)), None),
                    ("no_grad Discriminator.__call__", module, None)]
            for name, fn, policy in rows:
                if policy is not None:
                    policy()
                med, lo, hi = rounds_of(fn, args.warmup, args.reps, args.rounds)
                native_policy(lib, ctx, _native.RANGE_EXACT)()
                rate = flop / med * 1e-9
                print("  %-38s %8.3f (%.3f .. %.3f)   first layer's FLOPs over it: %6.1f TF = %4.1f %% of %.0f, %5.1f %% of %.0f" % (
                    name, med, lo, hi, rate, 100 * rate / F16X3_TF, F16X3_TF, 100 * rate / F32_MATRIX_TF, F32_MATRIX_TF))
            del x, y
        cc.close()
        del D, w, b
        torch.cuda.empty_cache()


def grad_bench(args, dev, lib, ctx, p):
    from speechseparation_amd.discriminator import grad_layout, layer1_dx, reference_channel_order
    print("critic_bench --grad: %s; %d medians of %d runs after %d warm-up runs each: median of the medians (lowest .. highest), ms" % (
        torch.cuda.get_device_name(0), args.rounds, args.reps, args.warmup))
    for ch in args.channels:
        D = Discriminator(ch).to(dev)
        cc = D.commit(grad=True)
        w = D.layers[0].weight.detach()
        for sec in args.seconds:
            T = max(601, 1 + int(sec * 44100) // 1024)
            To = frames_out(T)
            y = torch.randn(2, ch, T, device=dev)                       # the separator's interleaved spectrum
            dp = torch.randn(2, WIDTHS[0], To, device=dev) * 1e-6
            dx, dw, db = torch.empty_like(y), torch.empty_like(w), torch.empty(WIDTHS[0], device=dev)
            flop = 2.0 * 2 * To * WIDTHS[0] * ch * 16
            lay = grad_layout(ch, 2, T)
            print("\nin_channels %d, T = %d frames, C = 2: %.1f GFLOP per first-layer product; %d x %d x 2 workgroups; dx image %.0f MB" % (
                ch, T, flop * 1e-9, lay["i_tiles"], lay["s_tiles"], lay["image_bytes"] * 1e-6))

            def parent():
                ya = y.detach().requires_grad_(True)
                D.score_fixed(reference_channel_order(ya)).sum().backward()
                return ya.grad

            def exact_bwd(want_dx):
                return lambda: _native.check(lib.bsrnn_critic_conv_backward(ctx, p(y), p(w), None, p(dp), p(dx) if want_dx else None, p(dw), p(db),
                                                                            2, ch, T, WIDTHS[0], 0, None))
            rows = [("score_grad, interleaved (policy exact)", lambda: cc.score_grad(y, interleaved=True), _native.RANGE_EXACT),
                    ("score_grad, interleaved (deferred)", lambda: cc.score_grad(y, interleaved=True), _native.RANGE_DEFERRED),
                    ("score_grad, planar (deferred)", lambda: cc.score_grad(y), _native.RANGE_DEFERRED),
                    ("score alone (deferred)", lambda: cc.score(y, interleaved=True), _native.RANGE_DEFERRED),
                    ("reorder + score_fixed + backward to x", parent, _native.RANGE_EXACT),
                    ("layer1_dx, fp16x2 (deferred)", lambda: layer1_dx(cc, dp, T, interleaved=True), _native.RANGE_DEFERRED),
                    ("exact first layer dW + db", exact_bwd(False), _native.RANGE_EXACT),
                    ("exact first layer dW + db + dx", exact_bwd(True), _native.RANGE_EXACT)]
            got = {}
            for name, fn, policy in rows:
                native_policy(lib, ctx, policy)()
                got[name] = rounds_of(fn, args.warmup, args.reps, args.rounds)
                native_policy(lib, ctx, _native.RANGE_EXACT)()
                print("  %-40s %8.3f (%.3f .. %.3f)" % ((name,) + got[name]))
            med = got["layer1_dx, fp16x2 (deferred)"][0]
            print("  first-layer dx: fp16x2 %.3f ms = %.1f TF (%.1f %% of %.0f); exact %.3f ms (dW + db + dx minus dW + db)" % (
                med, flop / med * 1e-9, 100 * flop / med * 1e-9 / F16X3_TF, F16X3_TF,
                got["exact first layer dW + db + dx"][0] - got["exact first layer dW + db"][0]))
            new, old = got["score_grad, interleaved (policy exact)"], got["reorder + score_fixed + backward to x"]
            spreads = (new[2] - new[1]) + (old[2] - old[1])
            print("  score_grad %.3f ms against %.3f ms: %.2fx; the difference %.3f ms %s both spreads together (%.3f ms)" % (
                new[0], old[0], old[0] / new[0], old[0] - new[0], "exceeds" if old[0] - new[0] > spreads else "DOES NOT exceed", spreads))
            del y, dp, dx, dw, db
        cc.close()
        del D, w
        torch.cuda.empty_cache()


def ragged_bench(args, dev, lib, ctx, p):
    from speechseparation_amd.bsrnn import BSRNN
    from speechseparation_amd.discriminator import ragged_layout
    print("critic_bench --ragged: %s; %d medians of %d runs after %d warm-up runs each: median of the medians (lowest .. highest), ms" % (
        torch.cuda.get_device_name(0), args.rounds, args.reps, args.warmup))
    ch, clips = 2050, 32
    D = Discriminator(ch).to(dev)
    cc = D.commit(grad=True)
    spread = [601 + (793 - 601) * c // (clips - 1) for c in range(clips)]
    for name, frames in (("32 stereo clips, 601 .. 793 frames", spread), ("32 stereo clips, 2154 frames each", [2154] * clips)):
        rows, Tmax, R = [2] * clips, max(frames), 2 * clips
        y = torch.randn(R, ch, Tmax, device=dev)                        # the separator's interleaved spectrum
        for c, t in enumerate(frames):
            y[2 * c:2 * c + 2, :, t:] = 0
        lay = ragged_layout(ch, R, Tmax, frames, rows)
        print("\n%s: R = %d, Tmax = %d; first layer %d K slabs, live frame tiles %d of %d, live position tiles %d of %d; workspace %.0f MB" % (
            name, R, Tmax, lay["slabs"], lay["live_t_tiles"], R * lay["t_tiles"], lay["live_s_tiles"], R * lay["s_tiles"], lay["ws_floats"] * 4e-6))

        def loop_grad():
            for c, t in enumerate(frames):
                cc.score_grad(y[2 * c:2 * c + 2, :, :t].contiguous(), interleaved=True)

        def loop_score():
            for c, t in enumerate(frames):
                cc.score(y[2 * c:2 * c + 2, :, :t].contiguous(), interleaved=True)
        table = [("score_grad_ragged (policy exact)", lambda: cc.score_grad_ragged(y, frames, rows, interleaved=True), _native.RANGE_EXACT),
                 ("score_grad_ragged (deferred)", lambda: cc.score_grad_ragged(y, frames, rows, interleaved=True), _native.RANGE_DEFERRED),
                 ("score_ragged (deferred)", lambda: cc.score_ragged(y, frames, rows, interleaved=True), _native.RANGE_DEFERRED),
                 ("per clip: copy + score_grad (exact)", loop_grad, _native.RANGE_EXACT),
                 ("per clip: copy + score_grad (deferred)", loop_grad, _native.RANGE_DEFERRED),
                 ("per clip: copy + score (deferred)", loop_score, _native.RANGE_DEFERRED)]
        got = {}
        for label, fn, policy in table:
            native_policy(lib, ctx, policy)()
            got[label] = rounds_of(fn, args.warmup, args.reps, args.rounds)
            native_policy(lib, ctx, _native.RANGE_EXACT)()
            print("  %-40s %8.3f (%.3f .. %.3f)" % ((label,) + got[label]))
        for new, old in (("score_grad_ragged (policy exact)", "per clip: copy + score_grad (exact)"),
                         ("score_grad_ragged (deferred)", "per clip: copy + score_grad (deferred)"),
                         ("score_ragged (deferred)", "per clip: copy + score (deferred)")):
            a, b = got[new], got[old]
            spreads = (a[2] - a[1]) + (b[2] - b[1])
            print("  %s %.3f ms against the loop's %.3f ms: %.2fx; one call is %s than the loop by more than both spreads together (%.3f ms)" % (
                new, a[0], b[0], b[0] / a[0], "SLOWER" if a[0] - b[0] > spreads else "not slower", spreads))
        del y
        torch.cuda.empty_cache()
    # the packed training step on the first batch, with and without the adversarial term
    model = BSRNN().to(dev).train()
    opt = hip_train.AdamW(model.parameters(), lr=0.001, weight_decay=0.01)
    lens = [(t - 1) * 1024 for t in spread]
    mix, speech = torch.randn(2 * clips, max(lens), device=dev) * 0.1, torch.randn(2 * clips, max(lens), device=dev) * 0.1
    print("\ntrain_step_packed, 32 stereo clips of 601 .. 793 frames (one optimizer step, the per-clip read-back included)")
    for label, kw in (("without a critic", {}), ("with the critic's score as a constant", dict(discriminator=cc)),
                      ("with the adversarial term", dict(discriminator=cc, adversarial=True))):
        got = rounds_of(lambda: hip_train.train_step_packed_critic(model, opt, mix, speech, lens, [2] * clips, kw.get("discriminator"),
                                                                 kw.get("adversarial", False)), args.warmup, args.reps, args.rounds)
        print("  %-40s %8.3f (%.3f .. %.3f)" % ((label,) + got))
    cc.close()


def native_policy(lib, ctx, policy):
    return lambda: _native.check(lib.bsrnn_set_range_policy(ctx, policy))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--score", action="store_true", help="time the committed critic (bsrnn_critic_score) instead of the layers")
    ap.add_argument("--grad", action="store_true", help="time the committed critic's score with its gradient (bsrnn_critic_score_grad) beside "
                    "the adversarial path through Discriminator.score_fixed")
    ap.add_argument("--ragged", action="store_true", help="time the committed critic on a padded batch (bsrnn_critic_score_grad_ragged) beside "
                    "the per-clip loop it replaces, and train_step_packed with and without the adversarial term")
    ap.add_argument("--rounds", type=int, default=5, help="--score, --grad, --ragged: medians per figure")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seconds", type=float, nargs="*", default=[8.0, 60.0])
    ap.add_argument("--channels", type=int, nargs="*", default=[2050, 4098])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib, ctx = _native.lib, hip_train._context(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()       # noqa: E731
    if args.score:
        return score_bench(args, dev, lib, ctx, p)
    if args.grad:
        return grad_bench(args, dev, lib, ctx, p)
    if args.ragged:
        return ragged_bench(args, dev, lib, ctx, p)
    print("critic_bench: %s, medians of %d after %d warm-up runs; ms (TF of the product) | floor at %.0f TF" % (
        torch.cuda.get_device_name(0), args.reps, args.warmup, F32_MATRIX_TF))
    for ch in args.channels:
        for sec in args.seconds:
            T = 1 + int(sec * 44100) // 1024
            if T < 601:
                T = 601
                note = " (raised to the critic's shortest input, 601 frames)"
            else:
                note = ""
            print("\nin_channels %d, %.0f s clip: T = %d frames%s, C = 2" % (ch, sec, T, note))
            dims, Tl = (ch,) + WIDTHS, T
            for l in range(4):
                I, O, To = dims[l], dims[l + 1], frames_out(Tl)
                x, w, b = torch.randn(2, I, Tl, device=dev), torch.randn(O, I, 16, device=dev) * 0.01, torch.randn(O, device=dev)
                y, dy = torch.empty(2, O, To, device=dev), torch.randn(2, O, To, device=dev)
                dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
                leaky = int(l < 3)
                flop = 2.0 * 2 * To * O * I * 16
                g = conv_layout(2, I, Tl, O)
                ours = {
                    "forward": lambda: _native.check(lib.bsrnn_critic_conv_forward(ctx, p(x), p(w), p(b), p(y), 2, I, Tl, O, leaky, None)),
                    "dW+db": lambda: _native.check(lib.bsrnn_critic_conv_backward(ctx, p(x), p(w), p(y), p(dy), None, p(dw), p(db), 2, I, Tl, O, leaky, None)),
                    "dW+db+dx": lambda: _native.check(lib.bsrnn_critic_conv_backward(ctx, p(x), p(w), p(y), p(dy), p(dx), p(dw), p(db), 2, I, Tl, O, leaky, None)),
                }
                xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

                def stock_bwd(inputs):
                    out = F.leaky_relu(F.conv1d(xs, ws, b, stride=3), 0.01) if leaky else F.conv1d(xs, ws, b, stride=3)
                    torch.autograd.grad(out, inputs, dy)
                stock = {
                    "forward": lambda: F.conv1d(x, w, b, stride=3),
                    "dW+db": lambda: stock_bwd([ws]),              # (forward included: autograd needs its graph)
                    "dW+db+dx": lambda: stock_bwd([ws, xs]),
                }
                t = {k: (timed(ours[k], args.warmup, args.reps), timed(stock[k], args.warmup, args.reps)) for k in ours}
                t_dx = t["dW+db+dx"][0] - t["dW+db"][0]
                floor = flop / (F32_MATRIX_TF * 1e12) * 1e3
                print("  layer %d  %4d -> %4d, T %4d -> %4d  (%.1f GFLOP per product; %d K slabs of %d channels, %d dW chunks)" % (
                    l, I, O, Tl, To, flop * 1e-9, g["slabs"], g["ch_per_slab"], g["dw_chunks"]))
                print("    forward    %8.3f ms (%5.1f TF) | floor %.3f ms | stock conv1d %8.3f ms" % (t["forward"][0], flop / t["forward"][0] * 1e-9, floor, t["forward"][1]))
                print("    dW + db    %8.3f ms (%5.1f TF) | floor %.3f ms | stock forward + autograd (dW) %8.3f ms" % (
                    t["dW+db"][0], flop / t["dW+db"][0] * 1e-9, floor, t["dW+db"][1]))
                print("    dx         %8.3f ms (%5.1f TF) | floor %.3f ms | stock forward + autograd (dW, dx) %8.3f ms (ours dW + db + dx: %.3f ms)" % (
                    t_dx, flop / max(t_dx, 1e-6) * 1e-9, floor, t["dW+db+dx"][1], t["dW+db+dx"][0]))
                if l == 0:
                    print("    weights    %.0f MB: %.3f ms at %.1f TB/s (read once by forward and by dx, written once by dW)" % (
                        w.numel() * 4e-6, w.numel() * 4 / (HBM_TBS * 1e12) * 1e3, HBM_TBS))
                del x, w, y, dy, dx, dw, xs, ws
                Tl = To
            # the whole critic step of train-discriminator.py: two clips, the loop's loss, backward
            D = Discriminator(ch).to(dev)
            a, c = torch.randn(2, ch, T, device=dev), torch.randn(2, ch, T, device=dev)

            def step():
                for q in D.parameters():
                    q.grad = None
                (D(a) + (1 - D(c))).sum().backward()

            def stock_step():
                for q in D.parameters():
                    q.grad = None
                f = lambda v: D.layers2(D.layers(v).mean(dim=2).mean(dim=0))        # noqa: E731
                (f(a) + (1 - f(c))).sum().backward()
            print("  critic step (2 forwards + backward, dx of the first layer not needed): %.3f ms | stock torch modules %.3f ms" % (
                timed(step, args.warmup, args.reps), timed(stock_step, args.warmup, args.reps)))
            del D, a, c
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
