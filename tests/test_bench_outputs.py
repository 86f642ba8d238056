"""bench.py --dump-outputs and --full (CPU part): what dump_outputs writes for
a small and for a sampled output, that it is the same from call to call, and
that a plain command line asks for none of the --full measurements."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_output_is_dumped_whole(bench, tmp_path):
    import torch
    out = torch.arange(3 * 2048, dtype=torch.int64).to(torch.uint8)
    names = bench.dump_outputs(torch, str(tmp_path / "d"), 0, out, 2048)
    assert names == ["decoded.npy"]
    a = np.load(tmp_path / "d" / "decoded.npy")
    assert a.dtype == np.float32 and np.array_equal(a, out.numpy().astype(np.float32))


def test_large_output_is_sampled_and_summed(bench, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    monkeypatch.setattr(bench, "DUMP_SUMS", 4)
    stripe, nst = 2048, 9                        # 9 stripes in groups of 3
    g = torch.Generator().manual_seed(5)
    out = torch.randint(0, 256, (nst * stripe,), dtype=torch.uint8, generator=g)
    dirs = [str(tmp_path / d) for d in ("a", "b")]
    for d in dirs:
        names = bench.dump_outputs(torch, d, 1, out, stripe)
        assert sorted(names) == ["decoded_sample_rank1.npy", "decoded_stripe_sums_rank1.npy"]
    s = np.load(os.path.join(dirs[0], "decoded_sample_rank1.npy"))
    t = np.load(os.path.join(dirs[0], "decoded_stripe_sums_rank1.npy"))
    assert s.dtype == np.float32 and s.shape == (1000,)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, out.numel(), 1000))
    assert np.array_equal(s, out.numpy()[idx].astype(np.float32))
    want = out.numpy().astype(np.int64).reshape(3, 3 * stripe).sum(axis=1)
    assert t.dtype == np.float64 and np.array_equal(t, want.astype(np.float64))
    for name in ("decoded_sample_rank1.npy", "decoded_stripe_sums_rank1.npy"):
        assert np.array_equal(np.load(os.path.join(dirs[0], name)),
                              np.load(os.path.join(dirs[1], name)))


def test_dump_of_the_flagship_size_stays_under_64_mb(bench):
    nst = (1 << 30) // 2048
    assert bench.DUMP_SAMPLE * 4 + min(nst, bench.DUMP_SUMS) * 8 <= 64 * 10**6


def test_plain_command_line_is_lean(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "x"
