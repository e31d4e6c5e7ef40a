"""CPU: train.py --critic PATH [--adversarial]: the flags, what they refuse, and that a run without them parses to what it always did."""
import importlib.util
import os

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def entry():
    spec_ = importlib.util.spec_from_file_location("train_entry_critic", os.path.join(REPO, "train.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


def test_critic_flags(entry, capsys):
    ap = entry.build_parser()
    plain = vars(entry.parse_args(ap, ["--synthetic", "2"]))
    assert "critic" not in plain and "adversarial" not in plain                   # absent unless given
    args = entry.parse_args(ap, ["--synthetic", "2", "--critic", "discriminator.pth"])
    assert args.critic == "discriminator.pth" and not getattr(args, "adversarial", False)
    args = entry.parse_args(ap, ["--synthetic", "2", "--critic", "d.pth", "--adversarial", "--batch_size", "4"])
    assert args.critic == "d.pth" and args.adversarial is True
    for extra in (["--graph"], ["--ragged"], ["--remix", "dir"]):
        with pytest.raises(SystemExit) as e:
            entry.main(["--synthetic", "2", "--critic", "d.pth"] + extra)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--critic does not go with --graph, --ragged or --remix" in err
    with pytest.raises(SystemExit) as e:
        entry.main(["--synthetic", "2", "--adversarial"])
    assert e.value.code == 2 and "--adversarial needs --critic" in capsys.readouterr().err
