"""CPU: the host side of the device-resident training set (``TrainWorker.resident``) — the C ABI declares the gather and
the ctypes table binds it, the budget rule, the host stage against the files, the generator parity of the resident
iterable with a DataLoader iterator, and the fallback to the loader route on a CPU device."""
import pathlib
import random
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import unet_ref

ROOT = pathlib.Path(__file__).resolve().parents[1]
GIB = 1 << 30


def test_header_and_ctypes_table_carry_the_gather():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    m = re.search(r"\bint\s+mseg_set_gather\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, "mseg_set_gather is not declared in include/mseg_hip.h"
    assert len(m.group(1).split(",")) == 11
    assert "mseg_set_gather" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mseg_set_gather"][1]) == 11
    for name in ("MSEG_GATHER_RAW", "MSEG_GATHER_F32", "MSEG_GATHER_NORM", "MSEG_GATHER_I64"):
        value = int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))
        assert getattr(_lib, name[5:]) == value
    assert "resident.hip" in (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()


@pytest.mark.parametrize("need,limit,free,want", [
    (8 * GIB, 8 * GIB, 288 * GIB, True),            # exactly at the limit
    (8 * GIB + 1, 8 * GIB, 288 * GIB, False),       # one byte over
    (4 * GIB, 8 * GIB, 16 * GIB, True),             # exactly a quarter of the free memory
    (4 * GIB + 1, 8 * GIB, 16 * GIB, False),        # the quarter rule binds before the 8 GiB one
    (1, 8 * GIB, 3, False),
    (0, 0, 0, True),
])
def test_budget_rule(need, limit, free, want):
    from microbeseg_amd.training.resident_set import resident_fits
    assert resident_fits(need, limit, free) is want


def test_budget_default_and_worker_attributes():
    from microbeseg_amd.training import resident_set as R
    from microbeseg_amd.training.train import TrainWorker
    assert R.DEFAULT_MAX_BYTES == 8 * GIB and R.MAX_THREADS == 16
    assert TrainWorker.resident is False and TrainWorker.resident_max_bytes == 8 * GIB


@pytest.mark.parametrize("label_type", ["distance", "boundary"])
def test_host_stage_equals_the_files(tmp_path, label_type):
    from microbeseg_amd.training import resident_set as R
    from microbeseg_amd.utils import synth, tiffio
    data = synth.write_training_set(tmp_path / "set", 6, 4, size=64, seed=5)
    host = R.load_host(data, label_type, threads=64)           # more than 16 threads asked for: capped, still right
    want = {"distance": {"img": ("img", np.uint16), "border_label": ("neighbor_dist", np.float32),
                         "cell_label": ("cell_dist", np.float32)},
            "boundary": {"img": ("img", np.uint16), "label": ("boundary", np.uint8)}}[label_type]
    total = 0
    for split, n in (("train", 6), ("val", 4)):
        assert list(host[split]) == list(want)
        for name, (prefix, dtype) in want.items():
            a = host[split][name]
            assert a.dtype == dtype and a.shape == (n, 64, 64) and a.flags.c_contiguous
            for i in range(n):
                assert np.array_equal(a[i], tiffio.imread(str(data / split / f"{prefix}_{i:03d}.tif")).astype(dtype))
            total += a.nbytes
    assert R.host_bytes(host) == total


@pytest.mark.parametrize("label_type", ["distance", "boundary"])
def test_host_stage_refuses_mixed_shapes(tmp_path, label_type):
    from microbeseg_amd.training import resident_set as R
    from microbeseg_amd.utils import synth, tiffio
    data = synth.write_training_set(tmp_path / "set", 6, 4, size=64, seed=5)
    rng = np.random.Generator(np.random.PCG64(1))
    other = synth.synth_crop(rng, 48)
    for prefix, key in (("img", "img"), ("cell_dist", "cell_dist"), ("neighbor_dist", "neighbor_dist"),
                        ("boundary", "boundary")):
        tiffio.imwrite(data / "train" / f"{prefix}_003.tif", other[key])
    with pytest.raises(R.MixedCropShapes):
        R.load_host(data, label_type)
    assert issubclass(R.MixedCropShapes, R.ResidentUnavailable)


class _StubSet:
    """in place of the gather: a batch is its index list"""

    def batch(self, split, indices, training):
        return (split, list(indices), training)


@pytest.mark.parametrize("n_train,n_val,batch", [(10, 4, 4), (7, 3, 8)])
def test_resident_iterable_consumes_the_generator_like_a_dataloader(n_train, n_val, batch):
    from microbeseg_amd.training.resident_set import ResidentBatches
    from microbeseg_amd.training.train import ShardPlan

    def run(make_loader, as_indices):
        torch.manual_seed(11)
        plans = {"train": ShardPlan(n_train, batch, 1, 0, shuffle=True), "val": ShardPlan(n_val, batch, 1, 0, shuffle=False)}
        loaders = {x: make_loader(x, plans[x]) for x in plans}
        trace = []
        for epoch in range(3):
            plans["train"].start_epoch(epoch)
            for phase in ("train", "val"):
                it = iter(loaders[phase])
                trace.append(("iter", phase, torch.get_rng_state().clone()))
                got = [as_indices(b) for b in it]
                assert got == [b for b in plans[phase].steps if b]
                trace.append(("done", phase, got, torch.get_rng_state().clone()))
        return trace

    sizes = {"train": n_train, "val": n_val}
    loader_trace = run(lambda x, plan: torch.utils.data.DataLoader(list(range(sizes[x])), batch_sampler=plan, num_workers=0),
                       lambda b: b.tolist())
    random.seed(5)
    np.random.seed(5)
    py_state, np_state = random.getstate(), np.random.get_state()
    stub = _StubSet()
    resident_trace = run(lambda x, plan: ResidentBatches(stub, x, plan, training=(x == "train")), lambda b: b[1])
    assert random.getstate() == py_state
    after = np.random.get_state()
    assert after[0] == np_state[0] and np.array_equal(after[1], np_state[1]) and after[2:] == np_state[2:]
    assert len(loader_trace) == len(resident_trace) == 12
    for a, b in zip(loader_trace, resident_trace):
        assert a[:2] == b[:2]
        assert torch.equal(a[-1], b[-1]), a[:2]
        if a[0] == "done":
            assert a[2] == b[2]
    shuffled = [t[2] for t in resident_trace if t[0] == "done" and t[1] == "train"]
    assert shuffled[0] != shuffled[1] or shuffled[1] != shuffled[2]          # the epochs do differ


def test_resident_iterable_passes_split_and_phase():
    from microbeseg_amd.training.resident_set import ResidentBatches
    from microbeseg_amd.training.train import ShardPlan
    plan = ShardPlan(5, 2, 1, 0, shuffle=False)
    assert list(ResidentBatches(_StubSet(), "val", plan, training=False)) == [("val", [0, 1], False), ("val", [2, 3], False),
                                                                              ("val", [4], False)]
    assert len(ResidentBatches(_StubSet(), "val", plan, training=False)) == 3


def test_batch_checks_indices_on_the_host_before_any_launch(tmp_path):
    from microbeseg_amd.training import resident_set as R
    from microbeseg_amd.utils import synth
    data = synth.write_training_set(tmp_path / "set", 3, 2, size=16, seed=2, label_types=("boundary",))
    calls = []
    rset = R.ResidentSet(R.load_host(data, "boundary"), "boundary", "cpu", 0, 65535, raw_train=True,
                         gather=lambda *a: calls.append(a))
    for bad in ([0, 3], [-1], [1, 2, 7]):
        with pytest.raises(IndexError):
            rset.batch("train", bad, True)
    with pytest.raises(IndexError):
        rset.batch("val", [2], False)
    assert calls == []


class OracleNet(nn.Module):
    """CPU stand-in with the product's parameter tree; forward = oracle/unet_ref.py (the harness of test_train_worker.py)."""

    def __init__(self, holder, ut, act, norm, filters):
        super().__init__()
        self.holder, self.cfg = holder, (ut, act, norm, filters)

    def forward(self, x):
        sd = dict(self.holder.named_parameters())
        sd.update(dict(self.holder.named_buffers()))
        ut, act, norm, filters = self.cfg
        return unet_ref.unet_forward(sd, x, ut, act, norm, filters, training=self.training,
                                     update_running_stats=self.training)

    def state_dict(self, *a, **k):
        return self.holder.state_dict(*a, **k)

    def load_state_dict(self, sd, *a, **k):
        return self.holder.load_state_dict(sd, *a, **k)


def test_resident_on_the_cpu_falls_back_to_the_loader(tmp_path, monkeypatch):
    import json
    from microbeseg_amd.training import train as T
    from microbeseg_amd.utils import synth
    from microbeseg_amd.utils.unets import build_unet as real_build
    data = synth.write_training_set(tmp_path / "set", 6, 4, size=64, seed=5)

    def fake_build(unet_type, act_fun, pool_method, normalization, device, num_gpus, ch_in=1, ch_out=1,
                   filters=(64, 1024)):
        holder = real_build(unet_type, act_fun, pool_method, normalization, "cpu", 1, ch_in, ch_out, tuple(filters))
        return OracleNet(holder, unet_type, act_fun, normalization, tuple(filters))

    monkeypatch.setattr(T, "build_unet", fake_build)
    monkeypatch.setattr(T, "get_loss", lambda loss_function, label_type: {"border": unet_ref.regression_loss,
                                                                          "cell": unet_ref.regression_loss})
    monkeypatch.setitem(T.OPTIMIZER_RECIPES["adam"], "make",
                        lambda ps, lr: torch.optim.Adam(ps, lr=lr, betas=(0.9, 0.999), eps=1e-8, amsgrad=True))
    w = T.TrainWorker()
    w.augment = False
    w.resident = True
    msgs, prog = [], []
    w.text_output.connect(msgs.append)
    w.progress.connect(prog.append)
    models = tmp_path / "models"
    models.mkdir()
    w.start_training(data, models, "distance", 2, "adam", 2, torch.device("cpu"), 1, False, filters=[8, 16], max_epochs=2)
    fallback = [m for m in msgs if m.startswith("Resident training set not used")]
    assert len(fallback) == 1 and "not a GPU" in fallback[0]                 # said once for both iterations
    assert w._resident_state is None                                          # released at the end
    for k in (1, 2):
        assert (models / f"distance_model_{k:02d}.pth").exists()
        cfg = json.load(open(models / f"distance_model_{k:02d}.json"))
        assert cfg["trained_epochs"] == 2 and "data_route" not in cfg
        assert len((models / f"distance_model_{k:02d}_loss.txt").read_text().splitlines()) == 3
    assert any("--> save" in m for m in msgs) and prog[-1] == 100
