"""CPU: `python bench.py --gpus 2` starts two ranks itself (torch.distributed.run, 127.0.0.1 rendezvous) and rank 0
prints ONE JSON line with n_gpus == 2 — the launcher / barrier / max-over-ranks path of the driver contract, rehearsed
with gloo and no kernels (`--rehearse`); and what `--dump-outputs` writes."""
import json
import os
import pathlib
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True, env=env,
                       timeout=300)
    return r


def test_gpus_2_starts_two_ranks_and_reports_them():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--rehearse"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 64
    assert out["steps"] == 3 and out["scaling"] == "weak" and out["rehearsal"] is True
    assert out["ms_per_step"] >= 2.0          # max over ranks: rank 1 sleeps 2 ms per step, rank 0 only 1 ms


def test_gpus_flag_must_match_the_launcher():
    r = _run(["--gpus", "2", "--rehearse"], {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 2" in (r.stderr + r.stdout)


def test_pmc_profile_is_selected_by_workload_and_kernel_sources(monkeypatch):
    """roofline.traffic comes from a committed counter profile of the SAME workload taken on the SAME kernel sources
    (tools/pmc_traffic.sh records bench.csrc_digest()); anything else is reported as stale / none, never as current."""
    import glob
    sys.path.insert(0, str(ROOT))
    import bench
    import argparse
    a = argparse.Namespace(batch=32, size=256, arch="DU", act="relu", norm="bn", filters=[64, 1024], optimizer="adam",
                           precision="fp32")
    monkeypatch.setattr(bench, "csrc_digest", lambda: "not-a-tree")
    got = bench.pmc_traffic("wgrad_halo9_kernel<3, 1>", a)
    assert got["traffic"] is None and got["traffic_source"] == "stale" and got["traffic_stale_profile"].startswith("profiles/")
    # a profile that records its source digest is used when (and only when) the digest matches
    for f in sorted(glob.glob(str(ROOT / "profiles" / "*_hbm_traffic_pmc.json")), reverse=True):
        tab = json.load(open(f))
        cfg = dict(tab.get("__config__") or {})
        sha = cfg.pop("csrc_sha", None)
        if sha is None:
            continue
        a2 = argparse.Namespace(**{**vars(a), **{k: cfg[k] for k in ("batch", "size", "precision") if k in cfg}})
        if bench.workload_key(a2) != cfg:
            continue
        kernel = next(k for k in tab if k != "__config__")
        monkeypatch.setattr(bench, "csrc_digest", lambda sha=sha: sha)
        got = bench.pmc_traffic(kernel, a2)
        assert got["traffic"] == int(tab[kernel]["hbm_bytes_per_launch"]) and got["traffic_source"].startswith("profiles/")
        break
    a.size = 512                               # no profile of that workload: say so instead of borrowing another one's
    assert bench.pmc_traffic("igemm_halo_bf16w4_kernel<0, true>", a) == {"traffic": None, "traffic_source": "none"}


def test_dump_outputs_writes_seeded_samples(tmp_path):
    """--dump-outputs: float32 / float64 arrays, the large ones cut to the same seeded sample in every run, 64 MB at most"""
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import bench
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4))
    preds = [torch.rand(3 << 20), torch.rand(2, 1, 8, 8)]   # one prediction above the sample size, one below
    loss = net(torch.rand(2, 1, 8, 8)).square().mean()
    loss.backward()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), net, loss.detach(), preds)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert set(got) == {"loss", "border", "cell", "state_sample", "grad_sample"}
    assert got["loss"].dtype == np.float64 and got["loss"] == np.float64(loss.item())
    assert all(a.dtype == np.float32 for k, a in got.items() if k != "loss")
    assert got["border"].shape == (bench.DUMP_SAMPLE,) and np.isin(got["border"], preds[0].numpy()).all()
    assert np.array_equal(got["cell"], preds[1].numpy().ravel())
    n_state = sum(v.numel() for v in net.state_dict().values() if v.is_floating_point())
    assert got["state_sample"].shape == (n_state,) and got["grad_sample"].shape == (sum(p.numel() for p in net.parameters()),)
    assert np.array_equal(got["grad_sample"], torch.cat([p.grad.ravel() for p in net.parameters()]).numpy())
    for k, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{k}.npy"))


@pytest.mark.gpu
def test_dump_outputs_come_from_the_last_timed_step(tmp_path):
    """Same arguments -> the same outputs; one more timed step (--steps) -> a later step's outputs"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    small = ["--batch", "2", "--size", "64", "--filters", "16", "64", "--warmup", "1", "--no-cpu-baseline",
             "--no-inference", "--no-kernel-timing"]
    dumps = {}
    for tag, steps in (("a", 2), ("b", 2), ("c", 3)):
        r = _run(["--gpus", "1", "--steps", str(steps), "--dump-outputs", str(tmp_path / tag)] + small)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == steps
        dumps[tag] = {p.stem: np.load(p) for p in (tmp_path / tag).iterdir()}
    a, b, c = dumps["a"], dumps["b"], dumps["c"]
    assert set(a) == {"loss", "border", "cell", "state_sample", "grad_sample"}
    assert a["border"].shape == a["cell"].shape == (2 * 64 * 64,)
    assert all(np.isfinite(v).all() for v in a.values())
    np.testing.assert_allclose(b["loss"], a["loss"], rtol=1e-5)
    for k in ("border", "cell"):
        np.testing.assert_allclose(b[k], a[k], rtol=1e-4, atol=1e-5)
    assert abs(float(c["loss"]) - float(a["loss"])) > 1e-4 * abs(float(a["loss"]))


def test_full_is_off_by_default(monkeypatch):
    """A plain run (--gpus / --steps / --warmup) measures the headline alone; whatever else the benchmark measures needs
    --full"""
    sys.path.insert(0, str(ROOT))
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--full"])
    assert bench.parse().full is True


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_rest():
    """A plain run prints the headline of its own timed steps and nothing that takes runs of its own; --full adds the
    bracketed kernel-timing pass and the CPU baseline (the inference block, also --full, is left out here for time)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    small = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64", "--filters", "16", "64"]
    extra = ("roofline", "kernel_families", "kernel_timing", "bf16_320", "secondary", "cpu_baseline", "inference")
    lines = {}
    for tag, more in (("plain", []), ("full", ["--full", "--no-inference"])):
        r = _run(small + more)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(got) == 1, r.stdout
        lines[tag] = json.loads(got[0])
    for out in lines.values():
        assert out["metric"] == "training crops/sec (64px)" and out["unit"] == "crops/s" and out["dtype"] == "f32"
        assert out["higher_is_better"] is True and out["steps"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert not any(k in lines["plain"] for k in extra), sorted(lines["plain"])
    assert "kernel_timing" in lines["full"] and "cpu_baseline" in lines["full"] and "inference" not in lines["full"]
