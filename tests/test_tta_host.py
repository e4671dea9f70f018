"""CPU: the host side of test-time augmentation (--tta) — the numpy restatement tests/tta_ref.py against
numpy's own flips / rotations and against the code numbering of mseg_aug_flip, the member sets, the shape classes, the
chunking arithmetic, the C ABI table and the command-line flag."""
import pathlib
import re

import numpy as np
import pytest

import augment_kernels_ref
import tta_ref

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEW = {"mseg_tta_expand": 12, "mseg_tta_merge": 12}

NUMPY = {0: lambda a: a, 1: np.fliplr, 2: np.flipud, 3: np.rot90, 4: lambda a: np.rot90(a, 2), 5: lambda a: np.rot90(a, 3),
         6: lambda a: np.rot90(np.fliplr(a)), 7: lambda a: np.rot90(np.flipud(a))}


@pytest.mark.parametrize("shape", [(5, 7), (1, 4), (6, 6)])
def test_restatement_equals_numpy_compositions_and_inverts(shape):
    a = np.arange(shape[0] * shape[1], dtype=np.float32).reshape(shape)
    for code in range(8):
        got = tta_ref.transform(a, code)
        assert np.array_equal(got, NUMPY[code](a)), code
        assert got.shape == (shape[::-1] if code in (3, 5, 6, 7) else shape)
        assert np.array_equal(tta_ref.transform(got, tta_ref.inverse(code)), a), code
    assert np.array_equal(tta_ref.transform(a, 6), a.T)
    stack = np.stack([a, 2 * a])                              # leading axes pass through
    assert np.array_equal(tta_ref.transform(stack, 5)[1], NUMPY[5](2 * a))


def test_code_numbering_is_that_of_the_training_flip_kernel():
    a = np.random.Generator(np.random.PCG64(3)).normal(size=(9, 9)).astype(np.float32)
    for code in range(8):
        assert np.array_equal(tta_ref.transform(a, code), augment_kernels_ref.flip(a, code)), code


def test_member_sets_inverse_codes_and_errors():
    from microbeseg_amd.inference import tta
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.tta == 1
    assert tta.member_codes(1) == (0,) and tta.member_codes(2) == (0, 1)
    assert tta.member_codes(4) == (0, 1, 2, 4) and tta.member_codes(8) == tuple(range(8))
    for bad in (3, 0, 16, -1, True, "4"):
        with pytest.raises(ValueError):
            tta.member_codes(bad)
    for c in range(8):
        assert tta.inverse_code(c) == tta_ref.inverse(c)
        assert tta.inverse_code(tta.inverse_code(c)) == c
    assert (tta.inverse_code(3), tta.inverse_code(5)) == (5, 3)
    with pytest.raises(ValueError):
        tta.inverse_code(8)


def test_shape_classes():
    from microbeseg_amd.inference import tta
    from microbeseg_amd.utils.utils import pad_amounts
    assert tta.shape_classes((0, 1, 2, 4), 100, 130) == [((0, 1, 2, 4), (100, 130), pad_amounts((100, 130)))]
    rect = tta.shape_classes(tuple(range(8)), 100, 130)
    assert rect == [((0, 1, 2, 4), (100, 130), pad_amounts((100, 130))), ((3, 5, 6, 7), (130, 100), pad_amounts((130, 100)))]
    assert rect[0][2] == rect[1][2][::-1] and rect[0][2][0] > 0 and rect[0][2][1] > 0
    square = tta.shape_classes(tuple(range(8)), 64, 64)         # two classes (two expand calls) of one shape
    assert square == [((0, 1, 2, 4), (64, 64), [0, 0]), ((3, 5, 6, 7), (64, 64), [0, 0])]
    assert tta.shape_classes((0,), 5, 7)[0][:2] == ((0,), (5, 7))
    with pytest.raises(Exception, match="too big"):
        tta.shape_classes((0, 1), 9000, 64)
    # the reference's member of a class has the class's shape and padding
    f = np.arange(100 * 130, dtype=np.uint16).reshape(100, 130)
    for cs, shape, pads in rect:
        for c in cs:
            x, p = tta_ref.member_input(f, c)
            assert list(p) == pads and x.shape == (shape[0] + pads[0], shape[1] + pads[1]) and x.dtype == np.float32


@pytest.mark.parametrize("hp,wp,fb,K,want", [(2048, 2048, 1, 8, (1, 1)), (2048, 2048, 0, 8, (1, 1)), (256, 256, 1, 8, (8, 1)),
                                             (256, 256, 0, 8, (64, 8)), (256, 256, 4, 4, (16, 4)), (256, 256, 64, 2, (64, 32)),
                                             (128, 192, 3, 8, (24, 3)), (1024, 1024, 1, 8, (4, 1)), (512, 512, 2, 2, (4, 2))])
def test_chunk_members(hp, wp, fb, K, want):
    from microbeseg_amd.inference import tta
    assert tta.chunk_members(hp, wp, fb, K) == want


def test_chunk_members_follows_the_pixel_budget(monkeypatch):
    from microbeseg_amd.inference import infer, tta
    monkeypatch.setattr(infer, "FRAME_BATCH_PIXELS", 3 * 128 * 128)
    assert tta.chunk_members(128, 128, 1, 4) == (3, 1)


def test_header_ctypes_table_and_build_script_carry_the_entry_points():
    import ctypes as C
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/mseg_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    assert "tta.hip" in build and (ROOT / "microbeseg_amd" / "csrc" / "tta.hip").is_file()
    # the descriptor: a pointer, four 64-bit strides, the code (+ padding) = 48 bytes, as the header declares it
    assert C.sizeof(_lib.MsegTtaMember) == 48
    decl = re.search(r"typedef struct MsegTtaMember \{(.*?)\} MsegTtaMember;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", decl)
    assert names == [f[0] for f in _lib.MsegTtaMember._fields_], names


def test_command_line_flag():
    import infer_script_local as script
    parser = script.build_parser()
    assert parser.parse_args(["-i", "x", "-m", "y"]).tta == 1
    assert parser.parse_args(["-i", "x", "-m", "y", "--tta", "8"]).tta == 8
    with pytest.raises(SystemExit):
        parser.parse_args(["-i", "x", "-m", "y", "--tta", "3"])
    assert "--tta" in parser.format_help()


def test_merge_restatement_is_an_ordered_fp32_sum():
    """three values whose fp32 sum depends on the order: the restatement adds left to right, then scales once"""
    vals = [np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24), np.float32(-1.0)]
    members = [np.full((2, 3), v, np.float32) for v in vals]
    got = tta_ref.merge(members, [0, 0, 0, 0], 4)
    want = np.float32(np.float32(np.float32(np.float32(vals[0] + vals[1]) + vals[2]) + vals[3]) * np.float32(0.25))
    assert want == 0.0 and np.all(got == want)                 # ((1 + e) + e) - 1 = 0 in fp32; e + e first would give 2e
    # mapping back: a member that is T_c of a plane merges to the plane
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    codes = list(range(8))
    assert np.array_equal(tta_ref.merge([tta_ref.transform(a, c) for c in codes], codes, 8), a)
