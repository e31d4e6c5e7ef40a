"""CPU checks of the critic's host side: the index arithmetic of speechseparation_amd/csrc/critic_host.h (output lengths, the four-layer
chain, the K slabs, the reduction chunks, the scratch sizes) through the small program tests/cpp/critic_check.cpp, the state_dict
inventory of the Discriminator, the channel permutation and the plateau rule of the learning rate.  No GPU."""
import json
import os
import subprocess

import pytest
import torch

from conftest import GOLDEN, REPO

CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("critic") / "critic_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "critic_check.cpp"), "-o", exe], check=True)

    def run(*args):
        return json.loads(subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True, text=True).stdout)
    return run


def test_t_out(ask):
    assert [ask("tout", T)["T_out"] for T in (15, 16, 17, 18, 19, 601)] == [0, 1, 1, 1, 2, 196]


def test_chain(ask):
    assert ask("chain", 600) == {"ok": 0, "lengths": [195, 60, 15, 0], "min": 601, "widths": [1024, 128, 64, 32]}
    assert ask("chain", 601)["ok"] == 1 and ask("chain", 601)["lengths"] == [196, 61, 16, 1]
    assert ask("chain", 684)["lengths"] == [223, 70, 19, 2]
    assert ask("chain", 15) == {"ok": 0, "lengths": [0, 0, 0, 0], "min": 601, "widths": [1024, 128, 64, 32]}


SHAPES = [(2, I, T, O) for I in (1, 66, 1024, 4098) for T, O in ((16, 1), (19, 1024), (211, 72), (601, 40), (601, 1024), (2813, 1024))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_slabs_and_chunks_cover_exactly_once(ask, shape):
    C, I, T, O = shape
    g = ask("layout", *shape)
    assert g["why"] == 0 and g["T_out"] == (T - 16) // 3 + 1
    # K slabs: [0, I) exactly once, in order, whole stages of four channels except the end
    rs = g["slab_ranges"]
    assert len(rs) == g["slabs"] >= 1 and rs[0][0] == 0 and rs[-1][1] == I
    assert all(a[1] == b[0] for a, b in zip(rs, rs[1:])) and all(lo < hi for lo, hi in rs)
    assert g["ch_per_slab"] % 4 == 0 and all(hi - lo == g["ch_per_slab"] for lo, hi in rs[:-1])
    assert g["slabs"] == 1 or g["ch_per_slab"] >= 8
    # reduction chunks: [0, T_out) exactly once, in order, whole stages of 32 frames except the end
    cs = g["chunk_ranges"]
    assert len(cs) == g["dw_chunks"] >= 1 and cs[0][0] == 0 and cs[-1][1] == g["T_out"]
    assert all(a[1] == b[0] for a, b in zip(cs, cs[1:])) and all(lo < hi for lo, hi in cs)
    assert g["dw_frames"] % 32 == 0 and all(hi - lo == g["dw_frames"] for lo, hi in cs[:-1])
    # tiles
    assert g["t_tiles"] == -(-g["T_out"] // 64) and g["o_tiles"] == -(-O // 64) and g["i_tiles"] == -(-I // 4)
    assert g["dx_tile"] == 177 and g["dx_halo"] == 5 and g["s_tiles"] == -(-T // 177)
    # a dx tile's 64 frames [59 n - 5, 59 n + 59) hold every frame (s - k) / 3 its positions [177 n, 177 n + 177) can name
    for n in (0, g["s_tiles"] - 1):
        lo, hi = 59 * n - 5, 59 * n + 59
        for s in (177 * n, 177 * n + 176):
            fr = [(s - k) // 3 for k in range(16) if (s - k) % 3 == 0]
            assert lo <= min(fr) and max(fr) < hi
    # scratch
    n_out = C * O * g["T_out"]
    assert g["record"] == O * I * 16 + O
    assert g["fwd_scratch"] == g["slabs"] * n_out
    rec = g["dw_chunks"] * g["record"] if g["dw_chunks"] > 1 else 0
    assert g["bwd_scratch"] == rec and g["bwd_scratch_leaky"] == rec + -(-n_out // 4) * 4
    # a function of the shape only
    assert ask("layout", *shape) == g


def test_first_layer_fills_the_chip_at_the_shortest_clip(ask):
    g = ask("layout", 2, 4098, 601, 1024)
    assert 2 * g["t_tiles"] * g["o_tiles"] * g["slabs"] >= 1024 and g["slabs"] >= 8
    assert g["dw_chunks"] == 1                                   # 16 x 1025 output tiles: no partial records of 268 MB each


def test_refusals(ask):
    assert ask("layout", 2, 3, 15, 5) == {"why": 2}
    assert ask("layout", 0, 3, 16, 5) == {"why": 1} and ask("layout", 2, 0, 16, 5) == {"why": 1} and ask("layout", 2, 3, 16, 0) == {"why": 1}
    assert ask("layout", 2, 1 << 20, 1 << 20, 5) == {"why": 3}
    assert ask("layout", 2, 1 << 22, 16, 1 << 6) == {"why": 3}  # W alone: 2^32 elements
    assert ask("layout", 2, 4098, 2813, 1024)["why"] == 0        # a 60 s clip


def test_state_dict_inventory():
    from speechseparation_amd.bsrnn import Discriminator
    import speechseparation_amd
    assert speechseparation_amd.Discriminator is Discriminator
    want = json.load(open(os.path.join(GOLDEN, "critic_state_dict.json")))["keys"]
    for ch in (4098, 2050, 66):
        D = Discriminator() if ch == 4098 else Discriminator(ch)
        got = [[k, list(v.shape)] for k, v in D.state_dict().items()]
        assert got == [[k, [ch if d == "IN" else d for d in shape]] for k, shape in want]
        assert all(v.dtype == torch.float32 for v in D.state_dict().values())
    with pytest.raises(ValueError, match="cuda"):
        Discriminator(66)(torch.zeros(2, 66, 601))              # no CPU fallback
    with pytest.raises(ValueError, match="601"):
        Discriminator(66)(torch.zeros(2, 66, 600))


def test_channel_permutation():
    from speechseparation_amd.discriminator import reference_channel_order
    z = torch.complex(torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3), -torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3) - 0.5)
    inter = torch.stack((z.real, z.imag), dim=2).reshape(2, 10, 3)           # the library's layout (m_dataset.py:189-190)
    assert torch.equal(reference_channel_order(inter), torch.cat((z.real, z.imag), 1))


def test_plateau_rule_follows_torch():
    from speechseparation_amd import train

    class Opt:
        lr = 1e-4

        def set_lr(self, v):
            self.lr = float(v)
    mine = Opt()
    sched = train.ReduceLROnPlateau(mine, "min", patience=8, factor=0.8)
    p = torch.nn.Parameter(torch.zeros(1))
    ref_opt = torch.optim.SGD([p], lr=1e-4)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(ref_opt, "min", patience=8, factor=0.8)
    # improves, stalls for ten epochs (one reduction), improves by less than the threshold for ten more (a second one), then improves
    losses = [1.0, 0.9, 0.8] + [0.8] * 10 + [0.8 * (1 - 5e-5)] * 10 + [0.5, 0.5]
    lrs = []
    for v in losses:
        sched.step(v)
        ref.step(v)
        assert mine.lr == ref_opt.param_groups[0]["lr"] and sched.get_last_lr() == ref.get_last_lr()
        lrs.append(mine.lr)
    assert len(set(lrs)) == 3 and lrs[-1] == pytest.approx(1e-4 * 0.8 * 0.8)
