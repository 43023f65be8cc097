"""bench.py's plain run and ``--dump-outputs``.

On the CPU: ``dump_outputs`` writes float32 / float64 ``.npy`` files, whole while they fit the byte
budget and as one fixed, seeded sample of rows beyond it.  On the GPU: ``bench.py --gpus 1 --steps K
--warmup W --dump-outputs DIR`` times exactly K steps in one window, runs no other leg, and the
arrays it writes are those of the drop-in API on the same seeded batch.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _outputs(B):
    import torch
    g = torch.Generator().manual_seed(3)
    return {"tokens": torch.randint(0, 256, (B, 140), generator=g, dtype=torch.int64),
            "params": torch.randn((B, 140), generator=g, dtype=torch.float32),
            "positions": torch.randn((B, 50, 14), generator=g, dtype=torch.float32)}


def test_dump_outputs_whole(tmp_path):
    import bench
    outs = _outputs(37)
    info = bench.dump_outputs(str(tmp_path / "d"), outs)
    assert sorted(os.listdir(tmp_path / "d")) == ["params.npy", "positions.npy", "tokens.npy"]
    assert info["rows_sampled"] is False
    for name, dtype in (("tokens", np.float64), ("params", np.float32), ("positions", np.float32)):
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == dtype and info["arrays"][name] == list(a.shape)
        assert np.array_equal(a, outs[name].numpy())


def test_dump_outputs_samples_rows_beyond_the_budget(tmp_path, monkeypatch):
    import bench
    outs = _outputs(501)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 200 * 1000)
    info = bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    assert info["rows_sampled"] is True and info["bytes"] <= 200 * 1000
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < 501
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 501
    # the budget is used: one more row of every array would not fit
    row_bytes = 140 * 8 + 140 * 4 + 50 * 14 * 4 + 8
    assert (len(rows) + 1) * row_bytes > 200 * 1000
    idx = rows.astype(np.int64)
    total = 0
    for name in ("tokens", "params", "positions", "sample_rows"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b), "the sample differs between two runs"
        total += a.nbytes
        if name != "sample_rows":
            assert np.array_equal(a, outs[name].numpy()[idx])
    assert total == info["bytes"]


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_outputs(gpu_device, tmp_path):
    import torch
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BEAST_BENCH_ONE_DEVICE"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], env=env, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    # the headline: exactly --steps timed steps in one window, ms_per_step is that window's
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["full"] is False
    walls = line["timing"]["window_wall_s"]
    assert line["timing"]["windows"] == 1 and len(walls) == 1
    assert line["ms_per_step"] == pytest.approx(walls[0] / 7 * 1e3, rel=1e-12)
    assert line["value"] == pytest.approx(4096 * 7 / walls[0], rel=1e-12)
    assert line["unit"] == "trajectories/s" and line["higher_is_better"] is True and line["dtype"].startswith("f32")
    # ... and nothing that belongs to --full
    for leg in ("fit", "bpe", "cpu_baseline", "token_parity", "roofline", "mfma"):
        assert line[leg] is None, leg
    assert line["timing"]["window_gpu_event_ms"] is None and "host_issue_us_per_step" not in line["timing"]
    # the arrays: what encode -> reconstruct_traj return on the bench's seeded batch
    assert sorted(os.listdir(out)) == ["params.npy", "positions.npy", "tokens.npy"]
    got = {n: np.load(out / f"{n}.npy") for n in ("tokens", "params", "positions")}
    assert got["tokens"].dtype == np.float64 and got["tokens"].shape == (4096, 140)
    assert got["params"].dtype == np.float32 and got["params"].shape == (4096, 140)
    assert got["positions"].dtype == np.float32 and got["positions"].shape == (4096, 50, 14)
    assert sum(a.nbytes for a in got.values()) == line["outputs"]["bytes"] <= 64 * 1000 * 1000
    from beast_tokenizer_amd import BEASTBsplineTokenizer
    from beast_tokenizer_amd.synthetic import synth_trajectories
    tok = BEASTBsplineTokenizer(num_dof=14, num_basis=10, seq_len=50, vocab_size=256, device=str(gpu_device))
    tok.fit_parameters([{"actions": torch.from_numpy(synth_trajectories(4096, 50, 14, seed=1, start=4096 * i))}
                        for i in range(2)], verbose=False)
    x = torch.from_numpy(synth_trajectories(4096, 50, 14, seed=100)).to(gpu_device)
    tokens, pd = tok.encode(x)
    pos = tok.reconstruct_traj(tokens)
    assert np.array_equal(got["tokens"], tokens.cpu().numpy().astype(np.float64))
    assert np.array_equal(got["params"], pd["params"].cpu().numpy())
    assert np.array_equal(got["positions"], pos.cpu().numpy())
