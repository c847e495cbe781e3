"""bench.py's ``--dump-outputs`` writer and the ``--full`` switch, on host tensors: the files hold
float32 arrays, a buffer above the per-array cap is sampled at the same positions on every call (so two
builds' dumps line up element for element), a small buffer is written whole, and a plain command line
leaves the extra measurements off."""
import importlib
import sys
import types

import numpy as np
import pytest
import torch


@pytest.fixture()
def bench(monkeypatch):
    # importing the benchmark installs the shipped MIOpen database and sets a runtime default in the
    # environment: keep both out of this process' later tests
    monkeypatch.setenv("PSD_NO_MIOPEN_DB", "1")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return importlib.import_module("bench")


def _plane(n, async_plane):
    g = torch.Generator().manual_seed(5)
    ps = types.SimpleNamespace(params_flat=torch.randn(n, generator=g).to(torch.bfloat16), refreshed=0)
    if async_plane:  # parallel/async_ps.py: the workers' weights are one pull behind until refreshed

        def refresh_weights():
            ps.refreshed += 1

        ps.refresh_weights = refresh_weights
    return ps


@pytest.mark.parametrize("async_plane", [False, True])
def test_small_buffers_are_written_whole(bench, tmp_path, async_plane):
    ps = _plane(1000, async_plane)
    loss = torch.tensor(6.25, dtype=torch.bfloat16)
    shapes = bench.dump_outputs(str(tmp_path / "d"), ps, loss)
    assert shapes == {"loss": 1, "weights": 1000}
    assert ps.refreshed == (1 if async_plane else 0)
    for name, t in {"loss": loss.reshape(1), "weights": ps.params_flat}.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, t.float().numpy())


def test_large_buffer_sample_is_fixed_and_bounded(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 4096)
    n = 3 * 4096 + 17
    ps = _plane(n, False)
    loss = torch.tensor(1.0)
    bench.dump_outputs(str(tmp_path / "a"), ps, loss)
    a = np.load(tmp_path / "a" / "weights.npy")
    assert a.dtype == np.float32 and a.shape == (4096,)
    # the positions depend only on the length: marking each element with its index reads them back
    marks = types.SimpleNamespace(params_flat=torch.arange(n, dtype=torch.float32))
    bench.dump_outputs(str(tmp_path / "b"), marks, loss)
    idx = np.load(tmp_path / "b" / "weights.npy").astype(np.int64)
    assert (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() < n
    assert len(np.unique(idx)) > 3000 and idx.max() - idx.min() > n // 2  # spread over the buffer
    np.testing.assert_array_equal(a, ps.params_flat.float().numpy()[idx])
    bench.dump_outputs(str(tmp_path / "c"), ps, loss)  # a second call: the same positions
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "weights.npy"), a)
    assert np.load(tmp_path / "a" / "loss.npy").shape == (1,)


def test_dump_stays_below_64_mb(bench):
    assert (bench.DUMP_MAX_ELEMS + 1) * 4 + 2 * 128 <= 64 * 10**6  # weights + loss + the .npy headers


def test_plain_command_line_leaves_the_extras_off(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "somewhere"
