"""bincode codec of VClock / GCounter / PNCounter and of their ops: the Engine
methods over crdt_clock_*_bincode* (include/crdts_hip.h "bincode of the
clocks, the counters and their ops").

    VClock<A>     u64 n | n x (A actor | u64 counter), actors ascending
    GCounter<A>   the same bytes; PNCounter<A>: VClock p | VClock n
    Dot<A>        A actor | u64 counter; PNCounter Op: Dot | u32 Dir

Blobs are uint8 device tensors; offsets, lengths and sizes int64 tensors
holding u64 values."""
from __future__ import annotations

import ctypes as C

from ._lib import CrdtError, check, lib
from ._util import _torch, on_stream, ptr as _p
from .batches import ClockBatch

KINDS = {"vclock": 1, "gcounter": 1, "pncounter": 2}
WIDTHS = (1, 2, 4, 8)


def n_clocks(kind):
    """Clocks per object of a kind: 1, or 2 for PNCounter (p then n)."""
    try:
        return KINDS[kind]
    except KeyError:
        raise CrdtError(-1, f"kind {kind!r} is not one of {sorted(KINDS)}") from None


def _width(actor_bytes):
    if actor_bytes not in WIDTHS:
        raise CrdtError(-1, f"actor_bytes {actor_bytes!r} is not one of {WIDTHS}")
    return int(actor_bytes)


def op_blob_bytes(actor_bytes, with_dir=False):
    """Size of a Dot (actor_bytes + 8) or of a PNCounter Op (+ 4)."""
    return _width(actor_bytes) + 8 + (4 if with_dir else 0)


def clock_blob_bytes(entries, actor_bytes, kind="vclock"):
    """Size of a state blob with `entries` (actor, counter) pairs in all."""
    return 8 * n_clocks(kind) + int(entries) * (_width(actor_bytes) + 8)


def place(lens, gap=0):
    """Exclusive scan of per-object counts (int tensor) with `gap` unused
    units after each -> (offsets int64, total)."""
    torch = _torch()
    step = lens.to(torch.int64) + int(gap)
    ends = torch.cumsum(step, 0)
    total = int(ends[-1].item()) if lens.numel() else 0
    return ends - step, total


def ops_extent(n_ops, stride, size):
    """Bytes a buffer of n_ops fixed-size blobs at `stride` must hold."""
    if stride < size:
        raise CrdtError(-1, f"stride {stride} below the op size {size}")
    return (n_ops - 1) * stride + size if n_ops else 0


def _csr_in(B):
    return None if B is None else B.cstruct()


class ClockBincodeEngine:
    """Engine's clock codec methods (mixed into crdts_hip.Engine)."""

    # ------------------------------------------------------------ dense rows
    def clock_from_bincode(self, blobs, blob_off, blob_len, n_actors, actor_bytes, kind="vclock", out=None,
                           stream=None, check_status=True):
        """`to_binary` blobs -> dense rows int64 [n, n_actors] (pncounter: [n,
        2 * n_actors], [P|N]); every slot is written, a bad blob's row is zero
        (CRDT_ENONCANON)."""
        torch = _torch()
        nc, n = n_clocks(kind), int(blob_off.numel())
        if blob_len.numel() != n:
            raise CrdtError(-1, "blob_off / blob_len lengths differ")
        if out is None:
            out = torch.empty((n, nc * n_actors), dtype=torch.int64, device=blobs.device)
        elif out.numel() != n * nc * n_actors:
            raise CrdtError(-1, "dense rows shape mismatch")
        self._done(lib.crdt_clock_dense_from_bincode(self.ctx, _p(blobs), int(blobs.numel()), _p(blob_off),
                                                     _p(blob_len), n, _width(actor_bytes), n_actors, nc, _p(out),
                                                     self._stream(stream)),
                   "clock_from_bincode", stream, check_status)
        return out

    def clock_to_bincode(self, rows, n_actors, actor_bytes, kind="vclock", stream=None, check_status=True):
        """Dense rows -> (blobs uint8, blob_off int64, blob_len int64), packed
        back to back (sizes, exclusive scan, write). A nonzero slot whose actor
        id does not fit actor_bytes latches CRDT_ENONCANON (size 0)."""
        nc, ab = n_clocks(kind), _width(actor_bytes)
        if rows.numel() % (nc * n_actors):
            raise CrdtError(-1, "dense rows shape mismatch")
        n = rows.numel() // (nc * n_actors)
        return self._egest("clock_dense", (_p(rows), n, n_actors, nc, ab), n, rows.device, stream, check_status)

    # -------------------------------------------------------------- CSR runs
    def clock_csr_from_bincode(self, blobs, blob_off, blob_len, actor_bytes, kind="vclock", gap=0, stream=None,
                               check_status=True):
        """`to_binary` blobs -> ClockBatch (a (P, N) pair for pncounter): entry
        counts from the framing, an exclusive scan (with `gap` unused entries
        after each run), then the runs. A bad blob has len 0."""
        torch = _torch()
        nc, ab, n = n_clocks(kind), _width(actor_bytes), int(blob_off.numel())
        if blob_len.numel() != n:
            raise CrdtError(-1, "blob_off / blob_len lengths differ")
        dev, st = blobs.device, self._stream(stream)
        lens = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(nc)]
        args = (self.ctx, _p(blobs), int(blobs.numel()), _p(blob_off), _p(blob_len), n, ab, nc)
        check(lib.crdt_clock_csr_bincode_lens(*args, _p(lens[0]), _p(lens[1]) if nc == 2 else None, st),
              "clock_csr_bincode_lens")
        outs = []
        with on_stream(stream):
            for ln in lens:
                off, total = place(ln, gap)
                cap = max(1, total)
                outs.append(ClockBatch(off, ln, torch.empty(cap, dtype=torch.int32, device=dev),
                                       torch.empty(cap, dtype=torch.int64, device=dev), n_entries=cap))
        w = [B.cout() for B in outs]
        self._done(lib.crdt_clock_csr_from_bincode(*args, C.byref(w[0]), C.byref(w[1]) if nc == 2 else None, st),
                   "clock_csr_from_bincode", stream, check_status)
        return outs[0] if nc == 1 else tuple(outs)

    def clock_csr_to_bincode(self, S, actor_bytes, stream=None, check_status=True):
        """ClockBatch (or a (P, N) pair: PNCounter) -> (blobs uint8, blob_off
        int64, blob_len int64), packed back to back."""
        P, N = S if isinstance(S, (tuple, list)) else (S, None)
        if N is not None and N.n_obj != P.n_obj:
            raise CrdtError(-1, "P and N batches differ in n_obj")
        p, n = _csr_in(P), _csr_in(N)
        lead = (C.byref(p), None if n is None else C.byref(n), _width(actor_bytes))
        return self._egest("clock_csr", lead, P.n_obj, P.off.device, stream, check_status)

    # ------------------------------------------------------------------- ops
    def clock_ops_from_bincode(self, blobs, n_ops, actor_bytes, with_dir=False, stride=None, stream=None,
                               check_status=True):
        """Fixed-size op blobs at blobs[j * stride] -> (actor int32, counter
        int64, dir int32 or None) device tensors of n_ops; a bad op becomes the
        skip sentinel (actor 0xFFFFFFFF, counter 0, dir 0)."""
        torch = _torch()
        size = op_blob_bytes(actor_bytes, with_dir)
        stride = size if stride is None else int(stride)
        if blobs.numel() < ops_extent(n_ops, stride, size):
            raise CrdtError(-1, "blob buffer too small")
        dev = blobs.device
        actor = torch.empty(n_ops, dtype=torch.int32, device=dev)
        counter = torch.empty(n_ops, dtype=torch.int64, device=dev)
        dir_ = torch.empty(n_ops, dtype=torch.int32, device=dev) if with_dir else None
        self._done(lib.crdt_clock_ops_from_bincode(self.ctx, _p(blobs), stride, n_ops, actor_bytes,
                                                   int(bool(with_dir)), _p(actor), _p(counter), _p(dir_),
                                                   self._stream(stream)),
                   "clock_ops_from_bincode", stream, check_status)
        return actor, counter, dir_

    def clock_ops_to_bincode(self, actor, counter, dir_, actor_bytes, stride=None, out=None, stream=None,
                             check_status=True):
        """(actor, counter, dir or None) -> uint8 device tensor, op j at [j *
        stride] (`out` is reused when given; bytes between blobs are not
        touched)."""
        torch = _torch()
        with_dir = dir_ is not None
        size = op_blob_bytes(actor_bytes, with_dir)
        stride = size if stride is None else int(stride)
        n_ops = int(actor.numel())
        need = ops_extent(n_ops, stride, size)
        if out is None:
            out = torch.zeros(need, dtype=torch.uint8, device=actor.device)
        elif out.numel() < need:
            raise CrdtError(-4, "blob buffer too small")
        self._done(lib.crdt_clock_ops_to_bincode(self.ctx, _p(actor), _p(counter), _p(dir_), n_ops, actor_bytes,
                                                 int(with_dir), _p(out), stride, self._stream(stream)),
                   "clock_ops_to_bincode", stream, check_status)
        return out
