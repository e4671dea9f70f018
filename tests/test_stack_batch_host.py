"""CPU: the host side of batched stack inference (--frame_batch) — the C ABI declares the group entry points and the
ctypes table carries them (test_host_contract.py then checks that the built library exports them), the group size rule,
and the command-line flag."""
import pathlib
import re
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEW = {"mseg_frames_minmax": 6, "mseg_frames_normalize": 10, "mseg_postproc_batch_workspace_bytes": 3,
       "mseg_distance_postprocess_batch": 16}


def test_header_and_ctypes_table_carry_the_group_entry_points():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    for name, nargs in NEW.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/mseg_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


@pytest.mark.parametrize("hp,wp,requested,want", [(256, 256, 0, 64), (512, 512, 0, 16), (2048, 2048, 0, 1),
                                                  (4096, 4096, 8, 1), (256, 256, 8, 8), (64, 64, 0, 64)])
def test_frame_batch_for(hp, wp, requested, want):
    from microbeseg_amd.inference.infer import frame_batch_for
    assert frame_batch_for(hp, wp, requested) == want


def test_frame_batch_defaults_to_the_frame_by_frame_path():
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.frame_batch == 1


def test_infer_script_lists_frame_batch():
    r = subprocess.run([sys.executable, str(ROOT / "infer_script_local.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--frame_batch" in r.stdout
    assert re.search(r"--frame_batch.*?\[extension\]", r.stdout, re.S)


class _FakeNet:
    """stands in for the network: 'runs out of memory' above `limit` samples, records the batch sizes it was asked for"""

    def __init__(self, limit, message="HIP out of memory. Tried to allocate 1.00 GiB"):
        self.limit, self.message, self.asked = limit, message, []

    def __call__(self, x):
        self.asked.append(int(x.shape[0]))
        if x.shape[0] > self.limit:
            raise RuntimeError(self.message)
        return x * 2


def _host_worker(net):
    from microbeseg_amd.inference.infer import InferWorker
    worker = InferWorker(device="cpu")
    worker.net = net
    return worker


def test_forward_group_halves_on_out_of_memory():
    import torch
    x = torch.arange(8, dtype=torch.float32).reshape(8, 1, 1, 1)
    net = _FakeNet(limit=2)
    chunks, size = _host_worker(net)._forward_group(x)
    assert net.asked == [8, 4, 2, 2, 2, 2] and size == 2
    assert [(i, m) for i, m, _ in chunks] == [(0, 2), (2, 2), (4, 2), (6, 2)]
    assert torch.equal(torch.cat([p for _, _, p in chunks]), x * 2)
    net = _FakeNet(limit=3)                          # 7 frames: 7, 3, 3, and the last one alone
    chunks, size = _host_worker(net)._forward_group(x[:7])
    assert net.asked == [7, 3, 3, 1] and size == 3
    assert [(i, m) for i, m, _ in chunks] == [(0, 3), (3, 3), (6, 1)]
    net = _FakeNet(limit=8)                          # fits: one call, the group size stays
    chunks, size = _host_worker(net)._forward_group(x)
    assert net.asked == [8] and size == 8 and len(chunks) == 1


def test_forward_group_gives_the_zero_mask_rule_to_single_frames():
    import torch
    x = torch.zeros(4, 1, 1, 1)
    net = _FakeNet(limit=0)
    worker = _host_worker(net)
    said = []
    worker.text_output.connect(said.append)
    chunks, size = worker._forward_group(x)
    assert net.asked == [4, 2, 1, 1, 1, 1] and size == 1
    assert [(i, m, p) for i, m, p in chunks] == [(0, 1, None), (1, 1, None), (2, 1, None), (3, 1, None)]
    assert len(said) == 4 and all("RuntimeError during inference" in s for s in said)


def test_forward_group_passes_other_errors_on():
    import torch
    worker = _host_worker(_FakeNet(limit=0, message="invalid device function"))
    with pytest.raises(RuntimeError, match="invalid device function"):
        worker._forward_group(torch.zeros(4, 1, 1, 1))
