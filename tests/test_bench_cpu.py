"""bench.py on the CPU: the arrays --dump-outputs writes (what the timed path hands its caller, float32, within the size
budget, the same sample from run to run) and the argument checks that run before anything touches a GPU."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("_sgic_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SGIC_BENCH_SHAPES")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=120)


def test_dump_compress_streams(tmp_path):
    """one (B, longest) float32 array per byte-string field, byte values in order, -1 past the end of a shorter stream"""
    b = _bench()
    res = [(bytes([1, 2, 3]), bytes([250, 0]), b"\x07"), (bytes([4, 5, 6]), bytes([9, 8, 7, 255]), b"")]
    b.dump_outputs(str(tmp_path), res)
    assert sorted(os.listdir(tmp_path)) == ["clip_stream.npy", "h_bit_stream.npy", "z_bit_stream.npy"]
    z, h, c = (np.load(tmp_path / f"{n}.npy") for n in ("z_bit_stream", "h_bit_stream", "clip_stream"))
    assert z.dtype == h.dtype == c.dtype == np.float32
    assert np.array_equal(z, [[1, 2, 3], [4, 5, 6]])
    assert np.array_equal(h, [[250, 0, -1, -1], [9, 8, 7, 255]])
    assert np.array_equal(c, [[7], [-1]])


def test_dump_decompress_images_whole_when_small(tmp_path):
    b = _bench()
    x = torch.rand(2, 3, 8, 8)
    b.dump_outputs(str(tmp_path), x)
    got = np.load(tmp_path / "x_hat.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    assert not (tmp_path / "x_hat_index.npy").exists()


def test_dump_samples_an_output_over_the_budget(tmp_path):
    """an output larger than the budget: a seeded sample of its elements plus their positions, the same in every run, and the
    files stay within the budget"""
    b = _bench()
    x = torch.arange(4 * 3 * 64 * 64, dtype=torch.float32).reshape(4, 3, 64, 64)
    budget = 20_000
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), x, budget=budget)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= budget
    val, idx = np.load(tmp_path / "a" / "x_hat.npy"), np.load(tmp_path / "a" / "x_hat_index.npy")
    assert val.dtype == np.float32 and idx.dtype == np.float64 and len(val) == len(idx) > 1000
    assert np.array_equal(val, x.numpy().reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(val, np.load(tmp_path / "b" / "x_hat.npy"))
    assert np.array_equal(idx, np.load(tmp_path / "b" / "x_hat_index.npy"))


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_full_and_dump_outputs_are_options():
    r = _run(["--help"])
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_shape_list_needs_full():
    """SGIC_BENCH_SHAPES lists the launches of the --full profile window: refused without --full, before any GPU work"""
    r = _run(["--steps", "1"], env_extra={"SGIC_BENCH_SHAPES": os.devnull})
    assert r.returncode == 2 and "--full" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
