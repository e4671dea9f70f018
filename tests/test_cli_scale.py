"""CPU: the --scale flag of infer_script_local.py (inference at a chosen resolution) — the parser reports
range errors and the combinations the worker refuses, before a model is loaded."""
import pytest

BASE = ["-i", "x", "-m", "y"]


def _parser():
    import infer_script_local as script
    return script.build_parser()


def test_scale_is_accepted_and_defaults_to_one():
    parser = _parser()
    args = parser.parse_args(BASE)
    assert args.scale == 1.0 and isinstance(args.scale, float)
    assert parser.parse_args(BASE + ["--scale", "0.5"]).scale == 0.5
    assert parser.parse_args(BASE + ["--scale", "4"]).scale == 4.0
    assert parser.parse_args(BASE + ["--scale", "0.25"]).scale == 0.25
    action, = [a for a in parser._actions if "--scale" in a.option_strings]
    assert action.help.startswith("[extension]") and "--scale" in parser.format_help()


@pytest.mark.parametrize("value", ["0.2", "4.5", "0", "-1", "nan", "inf", "half"])
def test_out_of_range_values_are_rejected(value, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + ["--scale", value])
    assert exit_.value.code == 2 and "--scale" in capsys.readouterr().err


@pytest.mark.parametrize("extra", [["--tta", "4"], ["--sliding_window"]])
def test_combinations_are_rejected(extra, capsys):
    parser = _parser()
    with pytest.raises(SystemExit) as exit_:
        parser.parse_args(BASE + ["--scale", "0.5"] + extra)
    assert exit_.value.code == 2 and "--scale" in capsys.readouterr().err
    assert parser.parse_args(BASE + ["--scale", "1"] + extra).scale == 1.0          # scale = 1 is off: nothing to refuse
