"""bench.py --dump-outputs without a GPU: the files it writes for a whole merged index and for one rank's slice, their types and
sizes, and that a large result is sampled the same way every time."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeHip:
    """hipMemcpy on host memory: the fake index's 'device' pointer points into a numpy array."""

    class _Fn:
        argtypes = None

        def __call__(self, dst, src, count, kind):
            assert kind == 2
            ctypes.memmove(dst, src, count)
            return 0

    def __init__(self, *a, **k):
        self.hipMemcpy = self._Fn()


class FakeIndex:
    def __init__(self, stream, blocks):
        self.stream = stream
        self.nbytes = self.total_nbytes = stream.size
        self.bases, self.sequences, self.blocks = 10 * stream.size, stream.size // 7, blocks
        self.C = np.arange(7, dtype=np.uint64) * 1000

    def device_data(self):
        return self.stream.ctypes.data, self.stream.size

    def samples(self):
        be = np.arange(self.blocks, dtype=np.uint64) * 3
        cum = np.arange(6 * (self.blocks + 1), dtype=np.uint64).reshape(6, self.blocks + 1)
        return be, cum


class FakeSlice:
    def __init__(self, stream, first, total):
        self.stream, self.byte_first, self.nbytes, self.total_nbytes = stream, first, stream.size, total

    def data(self):
        return self.stream.copy()


@pytest.fixture
def fake_hip(monkeypatch):
    monkeypatch.setattr(ctypes, "CDLL", FakeHip)


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_small_index_is_dumped_whole(tmp_path, fake_hip):
    stream = np.random.default_rng(1).integers(0, 256, 100_000).astype(np.uint8)
    rec = bench.dump_outputs(np, FakeIndex(stream, 1563), str(tmp_path), 0, 1)
    got = load(str(tmp_path))
    assert rec["sampled"] is None and set(got) == {"stream", "stream_offsets", "C", "header", "sample_blocks", "sample_block_ends", "sample_counts"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["stream"], stream.astype(np.float32)) and got["stream"].dtype == np.float32
    assert np.array_equal(got["sample_counts"], np.arange(6 * 1564).reshape(6, 1564)[:, :1563])
    assert got["header"].tolist() == [10 * stream.size, stream.size // 7, stream.size, stream.size, 0]


def test_large_index_is_sampled_within_the_budget_and_reproducibly(tmp_path, fake_hip):
    stream = np.random.default_rng(2).integers(0, 256, 3 * bench.DUMP_BUDGET_BYTES // 4, dtype=np.uint8)
    blocks = stream.size // 64
    res = FakeIndex(stream, blocks)
    rec = bench.dump_outputs(np, res, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(np, res, str(tmp_path / "b"), 0, 1)
    a, b = load(str(tmp_path / "a")), load(str(tmp_path / "b"))
    assert rec["sampled"] and sum(x.nbytes for x in a.values()) == rec["bytes"] <= bench.DUMP_BUDGET_BYTES
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    offs = a["stream_offsets"].astype(np.int64)
    assert offs[0] == 0 and offs[-1] == stream.size - bench.DUMP_WINDOW and a["stream"].shape == (offs.size, bench.DUMP_WINDOW)
    for i in (0, offs.size // 2, offs.size - 1):
        assert np.array_equal(a["stream"][i], stream[offs[i]: offs[i] + bench.DUMP_WINDOW])
    pick = a["sample_blocks"].astype(np.int64)
    assert pick[0] == 0 and pick[-1] == blocks - 1 and np.array_equal(a["sample_block_ends"], 3.0 * pick)


def test_slices_of_a_sharded_result_carry_the_rank(tmp_path):
    stream = np.arange(5000, dtype=np.uint64).astype(np.uint8)
    rec = bench.dump_outputs(np, FakeSlice(stream, 12345, 99999), str(tmp_path), 1, 2)
    got = load(str(tmp_path))
    assert set(got) == {"stream_rank1", "stream_offsets_rank1", "header_rank1"} and set(rec["files"]) == set(got)
    assert np.array_equal(got["stream_rank1"], stream.astype(np.float32)) and got["header_rank1"].tolist() == [99999, 5000, 12345]
