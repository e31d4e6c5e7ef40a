"""Float64 restatement of the critic (speechseparation_amd/csrc/critic_host.h, "THE DEFINITION"; speechseparation_amd/discriminator.py)
on stock torch, CPU: one Conv1d(kernel 16, stride 3) layer with its backward, the error bounds of a length-n fp32 dot product, and the
whole module from nn.Conv1d / nn.Linear.  Written from the definition; the tests compare the library against it."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

KERNEL, STRIDE = 16, 3
WIDTHS = (1024, 128, 64, 32)
U = 2.0 ** -24                                     # unit roundoff of fp32


def t_out(T):
    return (T - KERNEL) // STRIDE + 1


def leaky32(pre):
    """LeakyReLU(0.01) as the library applies it to an fp32 pre-activation: v >= 0 ? v : fl32(0.01f * v), returned as float64."""
    v = pre.to(torch.float32)
    return torch.where(v >= 0, v, torch.tensor(0.01, dtype=torch.float32) * v).to(torch.float64)


def layer(x, w, b, dy, leaky, want_dx=True):
    """Everything one layer computes, in float64: dict(pre, y, dp, db, dw, dx) and, for the bounds, the same sums over absolute values
    (S_y, S_db, S_dw, S_dx) and the number of products of every element (n_y, n_db, n_dw scalars; n_dx per position s).
    `y` follows the library's conventions: fp32 LeakyReLU of the float64 pre-activation rounded to fp32; dp reads y > 0."""
    x, w, b, dy = (t.detach().to(torch.float64).cpu() for t in (x, w, b, dy))
    C, I, T = x.shape
    O = w.shape[0]
    To = t_out(T)
    pre = F.conv1d(x, w, b, stride=STRIDE)
    y = leaky32(pre) if leaky else pre
    dp = torch.where(y > 0, dy, float(np.float32(0.01)) * dy) if leaky else dy      # (the library's constant is 0.01f)
    out = dict(pre=pre, y=y, dp=dp)
    out["db"] = dp.sum(dim=(0, 2))
    xw = x.unfold(2, KERNEL, STRIDE)                                   # [C, I, To, 16]: x[c, i, 3 t + k]
    out["dw"] = torch.einsum("cot,citk->oik", dp, xw)
    out["S_y"] = F.conv1d(x.abs(), w.abs(), b.abs(), stride=STRIDE)
    out["S_db"] = dp.abs().sum(dim=(0, 2))
    out["S_dw"] = torch.einsum("cot,citk->oik", dp.abs(), xw.abs())
    out["n_y"], out["n_db"], out["n_dw"] = I * KERNEL, C * To, C * To
    if want_dx:
        dx = F.conv_transpose1d(dp, w, stride=STRIDE)                  # length 3 (To - 1) + 16 <= T
        S_dx = F.conv_transpose1d(dp.abs(), w.abs(), stride=STRIDE)
        pad = T - dx.shape[2]
        out["dx"], out["S_dx"] = F.pad(dx, (0, pad)), F.pad(S_dx, (0, pad))
        taps = F.conv_transpose1d(torch.ones(1, 1, To, dtype=torch.float64), torch.ones(1, 1, KERNEL, dtype=torch.float64), stride=STRIDE)
        out["n_dx"] = F.pad(taps, (0, pad)).reshape(1, 1, T) * O       # taps that reach position s, times the output channels
    return out


def bound(n, S):
    """First-order bound of a length-n fp32 dot product summed in any order: (n + 2) u S (n products, n - 1 additions, the bias, the
    rounding of the result)."""
    return (n + 2) * U * S


class CriticF64(nn.Module):
    """The critic from stock modules, float64 by default: the same state_dict keys and shapes as the library's Discriminator."""

    def __init__(self, in_channels=4098, dtype=torch.float64):
        super().__init__()
        dims = (in_channels,) + WIDTHS
        mods = []
        for l in range(4):
            mods.append(nn.Conv1d(dims[l], dims[l + 1], KERNEL, stride=STRIDE, dtype=dtype))
            if l < 3:
                mods.append(nn.LeakyReLU(0.01))
        self.layers = nn.Sequential(*mods)
        self.layers2 = nn.Sequential(nn.Linear(32, 1, dtype=dtype), nn.Sigmoid())

    def forward(self, x):
        return self.layers2(self.layers(x).mean(dim=2).mean(dim=0))


def synth_critic_state(in_channels, seed):
    """Weights of a fixed seed with torch's default scale (uniform in +-1/sqrt(fan_in)), float32 numpy -> dict of tensors."""
    rng = np.random.default_rng(seed)
    dims = (in_channels,) + WIDTHS
    sd = {}
    for l in range(4):
        k = 1.0 / np.sqrt(dims[l] * KERNEL)
        sd["layers.%d.weight" % (2 * l)] = torch.from_numpy(rng.uniform(-k, k, (dims[l + 1], dims[l], KERNEL)).astype(np.float32))
        sd["layers.%d.bias" % (2 * l)] = torch.from_numpy(rng.uniform(-k, k, (dims[l + 1],)).astype(np.float32))
    k = 1.0 / np.sqrt(32.0)
    sd["layers2.0.weight"] = torch.from_numpy(rng.uniform(-k, k, (1, 32)).astype(np.float32))
    sd["layers2.0.bias"] = torch.from_numpy(rng.uniform(-k, k, (1,)).astype(np.float32))
    return sd
