"""CPU: bench.py's --dump-outputs writers and the --full switch. The arrays
are float64 and exact (64-bit words as their low and high halves), an array
past its share of the byte budget is sampled at the same seeded positions in
every run, and a batch of Orswot records is written as every record's size
plus the words of a fixed sample of records, gaps left out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _args(d):
    return argparse.Namespace(dump_outputs=str(d))


def _argv(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_by_default_and_gates_the_cpu_baseline(monkeypatch):
    a = _argv(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "2")
    assert not a.full and not a.cpu_baseline and a.dump_outputs is None and a.steps == 3 and a.warmup == 2
    assert _argv(monkeypatch, "--full").cpu_baseline
    assert not _argv(monkeypatch, "--full", "--no-cpu-baseline").cpu_baseline
    assert _argv(monkeypatch, "--dump-outputs", "x").dump_outputs == "x"


def test_no_dir_no_files(tmp_path):
    bench.dump_arrays(argparse.Namespace(dump_outputs=None), 0, [("a", np.arange(4))])
    assert not list(tmp_path.iterdir())


def test_arrays_are_exact_float64(tmp_path):
    u = np.array([0, 1, (1 << 64) - 1, (1 << 53) + 1, 0xDEADBEEF12345678], np.uint64)
    t = torch.tensor([-1, 5, 1 << 40], dtype=torch.int64)
    bench.dump_arrays(_args(tmp_path), 0, [("u", u), ("t", t), ("i", np.array([[1, -2], [3, 4]], np.int32)),
                                           ("none", None)])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["i.npy", "t.npy", "u.npy"]
    gu, gt, gi = (np.load(tmp_path / f"{k}.npy") for k in "uti")
    assert gu.dtype == gt.dtype == gi.dtype == np.float64
    assert gu.shape == (5, 2) and gi.shape == (2, 2)
    back = gu[:, 0].astype(np.uint64) | (gu[:, 1].astype(np.uint64) << np.uint64(32))
    assert (back == u).all()
    tb = gt[:, 0].astype(np.uint64) | (gt[:, 1].astype(np.uint64) << np.uint64(32))
    assert (tb.view(np.int64) == t.numpy()).all()
    assert (gi == [[1, -2], [3, 4]]).all()


def test_large_array_is_a_fixed_sample_within_budget(tmp_path):
    x = np.arange(100_000, dtype=np.int32) * 3
    for d in ("a", "b"):
        bench.dump_arrays(_args(tmp_path / d), 0, [("x", x)], budget=16_000)
    idx, val = np.load(tmp_path / "a" / "x_index.npy"), np.load(tmp_path / "a" / "x.npy")
    assert idx.nbytes + val.nbytes <= 16_000 and idx.size == val.size == 1000
    assert (np.diff(idx) >= 0).all() and (val == x[idx.astype(np.int64)]).all()
    assert (idx == np.load(tmp_path / "b" / "x_index.npy")).all() and (val == np.load(tmp_path / "b" / "x.npy")).all()


def test_rank_folders(tmp_path):
    bench.dump_arrays(_args(tmp_path), 2, [("x", np.arange(3))])
    assert (tmp_path / "rank2" / "x.npy").exists()


class _Batch:
    def __init__(self, base, off):
        self.base, self.off = base, off


def _batch(sizes, gap=8, seed=1):
    """Records of the given byte sizes (multiples of 4; first word = size),
    `gap` bytes of other data between them."""
    rng = np.random.default_rng(seed)
    parts, off, pos = [], [], 0
    for s in sizes:
        rec = rng.integers(0, 1 << 32, s // 4, dtype=np.uint64).astype(np.uint32)
        rec[0] = s
        off.append(pos)
        parts += [rec, np.full(gap // 4, 0xFFFFFFFF, np.uint32)]
        pos += s + gap
    base = np.concatenate(parts).view(np.uint8)
    return _Batch(torch.from_numpy(base.copy()), torch.tensor(off, dtype=torch.int64)), np.concatenate(parts)


def test_orswot_batch_small_is_whole(tmp_path):
    sizes = [16, 40, 24, 160, 8]
    B, words = _batch(sizes)
    bench.dump_orswot_batch(_args(tmp_path), 0, "out", B)
    rec = np.load(tmp_path / "out_records.npy")
    assert rec.dtype == np.float64 and rec.size == sum(sizes) // 4
    assert (np.load(tmp_path / "out_record_objects.npy") == np.arange(5)).all()
    assert (np.load(tmp_path / "out_record_sizes.npy") == sizes).all()
    exp = np.concatenate([words[o // 4:o // 4 + s // 4] for o, s in zip(B.off.tolist(), sizes)])
    assert (rec == exp).all() and not (rec == 0xFFFFFFFF).any()  # no gap word


def test_orswot_batch_sample_is_seeded_and_sorted(tmp_path):
    sizes = [16 + 8 * (i % 5) for i in range(300)]
    B, words = _batch(sizes)
    for d in ("a", "b"):
        bench.dump_orswot_batch(_args(tmp_path / d), 0, "out", B, n_sample=64)
    ids = np.load(tmp_path / "a" / "out_record_objects.npy").astype(np.int64)
    assert ids.size == 64 and (np.diff(ids) > 0).all()
    assert (ids == np.load(tmp_path / "b" / "out_record_objects.npy")).all()
    rec = np.load(tmp_path / "a" / "out_records.npy")
    off = B.off.numpy()
    exp = np.concatenate([words[off[i] // 4:off[i] // 4 + sizes[i] // 4] for i in ids])
    assert (rec == exp).all()
    assert np.load(tmp_path / "a" / "out_record_sizes.npy").size == 300
