"""The state containers of the packed formats: ClockBatch (sparse CSR clocks,
crdt_clock_csr) and OrswotBatch (canonical Orswot records, crdt_orswot_batch).
Device memory comes from torch (plumbing only)."""
from __future__ import annotations

import numpy as np

from ._lib import SPARSE_CLOCK, Batch, ClockCsr, ClockCsrOut
from ._util import _torch


class ClockBatch:
    """A batch of sparse (CSR) clocks (include/crdts_hip.h crdt_clock_csr):
    object i's clock is entries [off[i], off[i] + len[i]) of (act, ctr) —
    actors strictly increasing, counters > 0. Tensors: off int64, len int32,
    act int32, ctr int64 (u64 bits); host numpy or device torch."""

    def __init__(self, off, len_, act, ctr, n_entries=None):
        self.off, self.len, self.act, self.ctr = off, len_, act, ctr
        self.n_obj = int(off.shape[0])
        self.n_entries = int(act.shape[0]) if n_entries is None else int(n_entries)

    @classmethod
    def from_host(cls, off, len_, act, ctr, device=0):
        torch = _torch()
        dev = f"cuda:{device}"

        def t(x, dt, ndt):
            x = np.ascontiguousarray(x, dtype=ndt)
            return torch.from_numpy(x.view(dt) if x.size else np.zeros(1, dt)).to(dev)

        return cls(t(off, np.int64, np.uint64)[: len(off)], t(len_, np.int32, np.uint32)[: len(len_)],
                   t(act, np.int32, np.uint32), t(ctr, np.int64, np.uint64), n_entries=len(act))

    @classmethod
    def from_lists(cls, clocks, device=0):
        """clocks: list of {actor: counter} dicts (or sorted (actor, counter) lists)."""
        runs = [sorted(dict(c).items()) for c in clocks]
        lens = np.array([len(r) for r in runs], np.uint32)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(runs) else np.zeros(0, np.uint64)
        act = np.array([a for r in runs for a, _ in r], np.uint32)
        ctr = np.array([c for r in runs for _, c in r], np.uint64)
        return cls.from_host(off, lens, act, ctr, device)

    def cstruct(self):
        return ClockCsr(self.off.data_ptr(), self.len.data_ptr(), self.act.data_ptr(), self.ctr.data_ptr(),
                        self.n_obj, self.n_entries)

    def cout(self):
        """crdt_clock_csr_out over this batch's arrays: a call writes n_entries entries at the most."""
        return ClockCsrOut(self.off.data_ptr(), self.len.data_ptr(), self.act.data_ptr(), self.ctr.data_ptr(),
                           self.n_entries)

    def to_host(self):
        return (self.off.cpu().numpy().view(np.uint64), self.len.cpu().numpy().view(np.uint32),
                self.act[: self.n_entries].cpu().numpy().view(np.uint32),
                self.ctr[: self.n_entries].cpu().numpy().view(np.uint64))

    def clocks(self):
        """Host list of sorted (actor, counter) lists, one per object."""
        off, ln, act, ctr = self.to_host()
        return [list(zip(act[o:o + n].tolist(), ctr[o:o + n].tolist())) for o, n in zip(off.tolist(), ln.tolist())]


class OrswotBatch:
    """A batch of canonical Orswot records resident on one GPU.

    base: torch.uint8 device tensor; off: torch.int64 device tensor (u64 offsets).
    flags: 0 (dense top clocks, n_actors slots) or SPARSE_CLOCK (CSR top clocks
    over an actor universe of n_actors ids).
    """

    def __init__(self, base, off, n_actors, nbytes=None, flags=0):
        self.base = base
        self.off = off
        self.flags = int(flags)
        self.n_actors = int(n_actors)
        self.n_obj = int(off.numel())
        self.bytes = int(nbytes if nbytes is not None else base.numel())

    def cbatch(self):
        return Batch(self.base.data_ptr(), self.off.data_ptr(), self.n_obj, self.bytes)

    @classmethod
    def from_host(cls, base, off, n_actors, device=0, flags=0):
        """device: a GPU index, or None / "cpu" for host tensors (the CPU tests' gloo path)."""
        torch = _torch()
        dev = "cpu" if device is None or device == "cpu" else (device if isinstance(device, str) else f"cuda:{device}")
        base = np.ascontiguousarray(base, dtype=np.uint8)
        nb = max(16, (base.nbytes + 15) // 16 * 16)
        b = torch.zeros(nb, dtype=torch.uint8, device=dev)
        if base.nbytes:
            b[: base.nbytes].copy_(torch.from_numpy(base))
        o = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).to(dev)
        return cls(b, o, n_actors, nb, flags)

    @classmethod
    def from_records(cls, records, n_actors, device=0, flags=0):
        offs, pos = [], 0
        for r in records:
            offs.append(pos)
            pos += (len(r) + 15) // 16 * 16
        base = np.zeros(max(pos, 16), dtype=np.uint8)
        for o, r in zip(offs, records):
            base[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
        return cls.from_host(base, np.array(offs, dtype=np.uint64), n_actors, device, flags)

    def to_host(self):
        base = self.base.cpu().numpy()
        off = self.off.cpu().numpy().view(np.uint64)
        return base, off

    def compact_bytes(self):
        """Σ over the records of SURVEY.md §8(d)'s compact algorithmic bytes
        (record.compact_bytes), from the headers gathered on the device."""
        torch = _torch()
        w = self.base[: self.base.numel() // 4 * 4].view(torch.int32)
        h = w[(self.off // 4)[:, None] + torch.arange(8, device=self.off.device)[None, :]].to(torch.int64)
        sp = (h[:, 7] & SPARSE_CLOCK) != 0
        top = torch.where(sp, 4 + 12 * h[:, 1], 8 * h[:, 1])
        return int((top + 8 + 12 * h[:, 2] + 12 * h[:, 3] + 8 * h[:, 4] + 12 * h[:, 5] + 8 * h[:, 6]).sum().item())

    def records(self):
        base, off = self.to_host()
        out = []
        for o in off.tolist():
            size = int(base[o:o + 4].view(np.uint32)[0])
            out.append(base[o:o + size].tobytes())
        return out
