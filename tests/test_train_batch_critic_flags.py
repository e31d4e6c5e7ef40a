"""CPU: train.py --batch_critic PATH [--adversarial]: the critic's term of the ragged and packed steps - how it parses, what it refuses,
and that --critic with --ragged or --remix is still refused as before."""
import importlib.util
import os

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def entry():
    spec_ = importlib.util.spec_from_file_location("train_entry_batch_critic", os.path.join(REPO, "train.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


def test_batch_critic_parses_with_the_two_batch_modes(entry):
    ap = entry.build_parser()
    plain = vars(entry.parse_args(ap, ["--synthetic", "2", "--ragged"]))
    assert "batch_critic" not in plain and "critic" not in plain and "adversarial" not in plain      # absent unless given
    args = entry.parse_args(ap, ["--synthetic", "2", "--ragged", "--batch_critic", "d.pth"])
    assert args.batch_critic == "d.pth" and not getattr(args, "adversarial", False) and not hasattr(args, "critic")
    args = entry.parse_args(ap, ["--remix", "dir", "--batch_critic", "d.pth", "--adversarial", "--batch_size", "4"])
    assert args.batch_critic == "d.pth" and args.adversarial is True and args.remix == "dir"
    args = entry.parse_args(ap, ["--synthetic", "2", "--ragged", "--batch_critic", "d.pth", "--adversarial"])
    assert args.adversarial is True


@pytest.mark.parametrize("extra", [[], ["--graph"], ["--ragged", "--graph"], ["--ragged", "--critic", "c.pth"], ["--critic", "c.pth"]],
                         ids=lambda e: "+".join(e) or "neither-mode")
def test_batch_critic_refusals(entry, capsys, extra):
    with pytest.raises(SystemExit) as e:
        entry.main(["--synthetic", "2", "--batch_critic", "d.pth"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    # (--critic beside --ragged meets its own, older refusal first)
    assert "--batch_critic goes with --ragged or --remix only" in err or ("--critic" in extra and "--ragged" in extra and entry.CRITIC_REFUSAL in err)


def test_batch_critic_beside_remix_and_graph_is_refused(entry, capsys):
    with pytest.raises(SystemExit) as e:
        entry.main(["--remix", "dir", "--graph", "--batch_critic", "d.pth"])
    assert e.value.code == 2 and "--remix does not go with --rir or --graph" in capsys.readouterr().err


def test_critic_with_ragged_or_remix_is_still_refused(entry, capsys):
    for extra in (["--ragged"], ["--remix", "dir"]):
        with pytest.raises(SystemExit) as e:
            entry.main(["--synthetic", "2", "--critic", "d.pth"] + extra)
        assert e.value.code == 2
        assert entry.CRITIC_REFUSAL in capsys.readouterr().err


def test_adversarial_alone_still_needs_a_critic(entry, capsys):
    with pytest.raises(SystemExit) as e:
        entry.main(["--synthetic", "2", "--ragged", "--adversarial"])
    assert e.value.code == 2 and "--adversarial needs --critic" in capsys.readouterr().err
