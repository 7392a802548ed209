"""bench.py --dump-outputs (CPU): the arrays written for the timed path's outputs.  dump_outputs runs on CPU tensors
here, with the outputs as strided views of one stripes tensor, as the benchmark passes them."""
import os
import types

import numpy as np
import torch

import bench

S, N, K, B = 37, 14, 10, 4099


def _dump(tmp_path, name, cap):
    torch.manual_seed(5)
    stripes = torch.randint(0, 256, (S, N, B), dtype=torch.uint8)
    old = bench.DUMP_MAX_BYTES
    bench.DUMP_MAX_BYTES = cap
    try:
        bench.dump_outputs(str(tmp_path / name), types.SimpleNamespace(rank=0),
                           {"parity": stripes[:, K:], "rebuilt": stripes[:, :1]})
    finally:
        bench.DUMP_MAX_BYTES = old
    files = sorted(os.listdir(tmp_path / name))
    assert files == ["parity.npy", "rebuilt.npy"]
    size = sum(os.path.getsize(tmp_path / name / f) for f in files)
    return stripes.numpy(), {f[:-4]: np.load(tmp_path / name / f) for f in files}, size


def test_dump_whole_outputs_when_they_fit(tmp_path):
    stripes, got, size = _dump(tmp_path, "whole", 32 << 20)
    assert size <= 32 << 20
    assert got["parity"].dtype == np.float32 and got["rebuilt"].dtype == np.float32
    assert np.array_equal(got["parity"], stripes[:, K:].astype(np.float32))
    assert np.array_equal(got["rebuilt"], stripes[:, :1].astype(np.float32))


def test_dump_samples_every_block_the_same_way_on_every_run(tmp_path):
    cap = 256 << 10
    stripes, a, size = _dump(tmp_path, "a", cap)
    _, b, _ = _dump(tmp_path, "b", cap)
    assert size <= cap
    for name, full in (("parity", stripes[:, K:]), ("rebuilt", stripes[:, :1])):
        assert a[name].dtype == np.float32
        assert np.array_equal(a[name], b[name])  # same positions, same bytes
        rows, blocks, c = a[name].shape
        assert (rows, blocks) == full.shape[:2] and 2 <= c < B
        assert np.array_equal(a[name][:, :, 0], full[:, :, 0]) and np.array_equal(a[name][:, :, -1], full[:, :, -1])
        # every sampled value is a byte of its own block
        for s, j in ((0, 0), (S - 1, blocks - 1)):
            assert set(a[name][s, j].astype(np.uint8)) <= set(full[s, j])
