"""`bench.py --full` / `--dump-outputs DIR` (CPU tests).

A plain run times the headline alone (--full is off by default), and
dump_outputs writes the last step's outputs exactly, as float32 / float64
.npy files, cutting an output over its byte budget to the same seeded rows
every time.  The pipeline here is a stand-in holding host tensors.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from hyperdrive_amd.verify import Verifier  # noqa: E402


class StubPipe:
    def __init__(self, B, seed=7):
        g = np.random.default_rng(seed)
        self.B = B
        self.verdict = g.integers(0, 8, B).astype(np.uint8)
        self.recovered = g.integers(0, 256, (B, 32)).astype(np.uint8)
        self.bitmap = g.integers(0, 1 << 32, B // 32, dtype=np.uint64).astype(np.uint32)
        t, a = Verifier._tally_struct(B)
        t.n_counts, t.n_hr = 5, 3
        for k in a:
            a[k][...] = g.integers(0, 200, a[k].shape).astype(a[k].dtype)
        self.last_tally = (t, a)

    def last(self, steps):
        return (torch.from_numpy(self.verdict), torch.from_numpy(self.recovered),
                torch.from_numpy(self.bitmap.view(np.int32)))


def test_full_is_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_exact(tmp_path):
    p = StubPipe(256)
    bench.dump_outputs(str(tmp_path), p, 4, 0, 1)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["bitmap", "recovered", "tally_counts", "tally_dup", "tally_hr", "verdict"]
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert np.array_equal(got["verdict"], p.verdict) and got["verdict"].dtype == np.float32
    assert np.array_equal(got["recovered"], p.recovered) and got["recovered"].shape == (256, 32)
    assert np.array_equal(got["bitmap"].astype(np.uint32), p.bitmap) and got["bitmap"].dtype == np.float64
    t, a = p.last_tally
    assert np.array_equal(got["tally_dup"], a["dup"][:256])
    assert got["tally_counts"].shape == (5, 5) and got["tally_hr"].shape == (3, 6)
    assert np.array_equal(got["tally_counts"][:, 0], a["count_height"][:5])


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setitem(bench.DUMP_BUDGET, "recovered", 64 * 128)      # 64 rows of 32 float32
    p = StubPipe(256)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), p, 4, 0, 1)
    ra, rb = np.load(tmp_path / "a" / "recovered.npy"), np.load(tmp_path / "b" / "recovered.npy")
    assert ra.shape == (64, 32) and np.array_equal(ra, rb)
    # the sample is rows of the output, in order
    rows = [int(np.flatnonzero((p.recovered == r).all(1))[0]) for r in ra]
    assert rows == sorted(rows) and len(set(rows)) == 64
    # ranks of a larger world share the budget and name their files
    bench.dump_outputs(str(tmp_path / "w"), p, 4, 1, 2)
    assert np.load(tmp_path / "w" / "recovered_rank1.npy").shape == (32, 32)
    # a rank of N > 1 holds its tally as packed rows (shard.pack_tally), without the dup column
    p.last_tally = {"counts": np.arange(10, dtype=np.int64).reshape(2, 5), "hr": np.zeros((0, 6), np.int64)}
    bench.dump_outputs(str(tmp_path / "r"), p, 4, 0, 2)
    assert sorted(os.listdir(tmp_path / "r")) == [f"{n}_rank0.npy" for n in
                                                  ("bitmap", "recovered", "tally_counts", "tally_hr", "verdict")]
    assert np.array_equal(np.load(tmp_path / "r" / "tally_counts_rank0.npy"), p.last_tally["counts"])
    assert np.load(tmp_path / "r" / "tally_hr_rank0.npy").shape == (0, 6)
    assert sum(bench.DUMP_BUDGET.values()) <= 64 << 20
