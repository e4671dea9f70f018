"""CPU: the --gap flag of infer_script_local.py (gap closing in cell tracks) — the parser reports range errors
and the missing --cells before a model is loaded."""
import pytest

BASE = ["-i", "x", "-m", "y"]
ON = BASE + ["--cells"]


def _parser():
    import infer_script_local as script
    return script.build_parser()


def test_gap_values():
    parser = _parser()
    assert parser.parse_args(BASE).gap is None and parser.parse_args(ON).gap is None
    assert parser.parse_args(ON + ["--gap"]).gap == 1                               # the bare flag
    for g in (1, 2, 3, 4):
        assert parser.parse_args(ON + ["--gap", str(g)]).gap == g
    args = parser.parse_args(BASE + ["--gap", "2", "--drift", "16", "--flow", "--cells"])
    assert (args.gap, args.drift, args.flow) == (2, 16, 8)
    action, = [a for a in parser._actions if "--gap" in a.option_strings]
    assert action.help.startswith("[extension]") and action.type is int
    assert action.nargs == "?" and action.const == 1 and action.default is None


@pytest.mark.parametrize("extra", [["--gap"], ["--gap", "2"], ["--drift", "--gap"], ["--hull", "--gap", "4"]])
def test_gap_without_cells_is_refused_with_the_scripts_message(extra, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + extra)
    assert exit_.value.code == 2 and "--gap needs --cells" in capsys.readouterr().err


@pytest.mark.parametrize("value", ["0", "5", "-1", "17"])
def test_gap_out_of_range_is_refused_with_the_scripts_message(value, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(ON + ["--gap", value])
    err = capsys.readouterr().err
    assert exit_.value.code == 2 and "--gap: 1 .. 4 missed frames expected" in err and f"got {value}" in err


def test_gap_that_is_no_whole_number_is_refused(capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(ON + ["--gap", "1.5"])
    err = capsys.readouterr().err
    assert exit_.value.code == 2 and "argument --gap: invalid int value: '1.5'" in err


def test_help_still_says_what_linking_is():
    text = " ".join(_parser().format_help().split())
    assert "no motion model" in text and "no gap closing" in text and "--gap" in text
