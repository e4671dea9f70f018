"""CPU: the --flow / --flow_tile flags of infer_script_local.py (linking under a tile-wise displacement field; DESIGN.md
§6v) — the parser reports range errors and the missing --cells / --drift before a model is loaded."""
import pytest

BASE = ["-i", "x", "-m", "y"]
ON = BASE + ["--cells", "--drift"]


def _parser():
    import infer_script_local as script
    return script.build_parser()


def test_flow_values():
    parser = _parser()
    assert parser.parse_args(BASE).flow is None and parser.parse_args(ON).flow is None
    assert parser.parse_args(ON).flow_tile == 64
    assert parser.parse_args(ON + ["--flow"]).flow == 8                             # the bare flag
    assert parser.parse_args(ON + ["--flow", "0"]).flow == 0
    assert parser.parse_args(ON + ["--flow", "32"]).flow == 32
    assert parser.parse_args(BASE + ["--flow", "5", "--drift", "16", "--cells"]).flow == 5
    for tile in (64, 128, 256):
        assert parser.parse_args(ON + ["--flow", "--flow_tile", str(tile)]).flow_tile == tile
    for flag in ("--flow", "--flow_tile"):
        action, = [a for a in parser._actions if flag in a.option_strings]
        assert action.help.startswith("[extension]") and action.type is int
    action, = [a for a in parser._actions if "--flow" in a.option_strings]
    assert action.nargs == "?" and action.const == 8


@pytest.mark.parametrize("extra", [["--flow"], ["--cells", "--flow"], ["--drift", "--flow"], ["--cells", "--drift", "--flow", "33"],
                                   ["--cells", "--drift", "--flow", "-1"], ["--cells", "--drift", "--flow", "1.5"]])
def test_flow_is_refused_with_a_message(extra, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + extra)
    assert exit_.value.code == 2 and "--flow" in capsys.readouterr().err


@pytest.mark.parametrize("tile", ["100", "32", "0", "64.0"])
def test_flow_tile_is_refused_with_a_message(tile, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(ON + ["--flow", "--flow_tile", tile])
    assert exit_.value.code == 2 and "--flow_tile" in capsys.readouterr().err
