"""LWWReg<u64, M> (src/lwwreg.rs): the host mirror, the device batch and op
containers, and the Engine methods over crdt_lwwreg_* (include/crdts_hip.h
"LWWReg<u64, M>, batched").

A marker is an int (marker_words = 1) or a 2-tuple of ints (marker_words = 2,
compared like a Rust tuple: word 0 first); a value is the caller's interned
u64 key."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CrdtError, LWWOpsC, LWWViewC, check, lib
from ._util import _torch, ptr as _p

# crdt_lwwreg_apply: lists of at least this many ops take the wave-per-register
# form, shorter ones the lane-per-register loop (CRDT_LWWREG_WAVE_MIN_OPS)
LWWREG_WAVE_MIN_OPS = 16
LWWREG_MAX_REPS = 32  # CRDT_LWWREG_MAX_REPS

class ConflictingMarker(Exception):
    """Error::ConflictingMarker: an equal marker with a different value."""


def _words(marker):
    return tuple(marker) if isinstance(marker, (tuple, list)) else (marker,)


class LWWReg:
    """Host mirror of LWWReg<V, M> (src/lwwreg.rs:27-32)."""

    def __init__(self, val=0, marker=0):
        self.val = val
        self.marker = tuple(marker) if isinstance(marker, list) else marker

    def update(self, val, marker):  # src/lwwreg.rs:104-118
        marker = tuple(marker) if isinstance(marker, list) else marker
        if self.marker < marker:
            self.val, self.marker = val, marker
        elif self.marker == marker and val != self.val:
            raise ConflictingMarker(f"marker {marker!r}: {val!r} != {self.val!r}")

    def merge(self, other: "LWWReg"):  # src/lwwreg.rs:56-66
        self.update(other.val, other.marker)

    def apply(self, op: "LWWReg"):  # src/lwwreg.rs:74-76
        self.merge(op)

    def clone(self):
        return LWWReg(self.val, self.marker)

    def __eq__(self, other):
        return isinstance(other, LWWReg) and (self.val, self.marker) == (other.val, other.marker)

    def __repr__(self):
        return f"LWWReg(val={self.val!r}, marker={self.marker!r})"


def _pack(regs, marker_words):
    """[(val, marker), ...] -> (val u64 [n], marker u64 [n, marker_words])."""
    val = np.zeros(len(regs), np.uint64)
    mk = np.zeros((len(regs), marker_words), np.uint64)
    for i, r in enumerate(regs):
        v, m = (r.val, r.marker) if isinstance(r, LWWReg) else r
        w = _words(m)
        if len(w) != marker_words:
            raise CrdtError(-1, f"marker {m!r} is not {marker_words} word(s)")
        val[i] = v
        mk[i] = np.array(w, dtype=np.uint64)
    return val, mk


def _dev(x, device):
    t = _torch().from_numpy(np.ascontiguousarray(x).view(np.int64))
    return t if device is None else t.to(f"cuda:{device}")


class LWWBatch:
    """A batch of registers in the ABI's layout: val int64 [n] and marker int64
    [n, marker_words] tensors holding u64 bits (device, or host with
    device=None)."""

    def __init__(self, val, marker):
        if marker.dim() != 2 or marker.shape[0] != val.numel() or marker.shape[1] not in (1, 2):
            raise CrdtError(-1, "LWWBatch: marker must be [n, 1] or [n, 2]")
        self.val, self.marker = val.contiguous(), marker.contiguous()
        self.n = int(val.numel())
        self.marker_words = int(marker.shape[1])

    @classmethod
    def from_arrays(cls, val, marker, device=0):
        marker = np.asarray(marker, np.uint64)
        marker = marker.reshape(-1, 1) if marker.ndim == 1 else marker
        return cls(_dev(np.asarray(val, np.uint64), device), _dev(marker, device))

    @classmethod
    def from_lists(cls, regs, marker_words=1, device=0):
        """regs[i] = (val, marker) or a host LWWReg."""
        return cls.from_arrays(*_pack(regs, marker_words), device=device)

    def clone(self):
        return LWWBatch(self.val.clone(), self.marker.clone())

    def to_host(self):
        return self.val.cpu().numpy().view(np.uint64), self.marker.cpu().numpy().view(np.uint64)

    def to_lists(self):
        """[(val, marker), ...]: marker an int (one word) or a 2-tuple."""
        v, m = self.to_host()
        if self.marker_words == 1:
            return list(zip(v.tolist(), m[:, 0].tolist()))
        return [(a, tuple(b)) for a, b in zip(v.tolist(), m.tolist())]

    def view(self):
        return LWWViewC(self.val.data_ptr() or None, self.marker.data_ptr() or None)


class LWWOps:
    """Op lists grouped per register (crdt_lwwreg_ops): obj_end int64 [n_obj],
    val int64 [n_ops], marker int64 [n_ops, marker_words]."""

    def __init__(self, obj_end, val, marker, host=None):
        self.obj_end, self.val, self.marker = obj_end, val, marker
        self.n_obj = int(obj_end.numel())
        self.n_ops = int(val.numel())
        self.marker_words = int(marker.shape[1])
        self.host = host

    @classmethod
    def from_arrays(cls, obj_end, val, marker, device=0):
        obj_end = np.ascontiguousarray(np.asarray(obj_end, np.uint64))
        val = np.ascontiguousarray(np.asarray(val, np.uint64))
        marker = np.ascontiguousarray(np.asarray(marker, np.uint64))
        marker = marker.reshape(-1, 1) if marker.ndim == 1 else marker
        return cls(_dev(obj_end, device), _dev(val, device), _dev(marker, device), host=(obj_end, val, marker))

    @staticmethod
    def arrays_from_lists(per_obj, marker_words=1):
        """per_obj[i] = [(val, marker), ...] -> (obj_end u64 [n_obj], val u64
        [n_ops], marker u64 [n_ops, marker_words])."""
        ends, flat = [], []
        for ops in per_obj:
            flat.extend(ops)
            ends.append(len(flat))
        val, mk = _pack(flat, marker_words)
        return np.asarray(ends, np.uint64), val, mk

    @classmethod
    def from_lists(cls, per_obj, marker_words=1, device=0):
        return cls.from_arrays(*cls.arrays_from_lists(per_obj, marker_words), device=device)

    def cops(self):
        p = [C.c_void_p(t.data_ptr()) if t.numel() else None for t in (self.obj_end, self.val, self.marker)]
        return LWWOpsC(*p, self.n_ops)


def blob_bytes(val_bytes, marker_bytes):
    return int(val_bytes) + sum(int(b) for b in _words(marker_bytes))


class LWWEngine:
    """Engine's LWWReg methods (mixed into crdts_hip.Engine)."""

    def lwwreg_merge(self, S: LWWBatch, O: LWWBatch, want_bitmap=True, want_count=True, bitmap=None, count=None,
                     stream=None):
        """In place: S[i].merge(O[i]) (src/lwwreg.rs:56-66). Returns (bitmap,
        count): the conflict bitmap (int64 [(n + 63) // 64] holding u64 words,
        bit i % 64 of word i // 64 = register i's merge returned Err) and the
        number of conflicts (int64 [1]), each None when not wanted (`bitmap`
        / `count`: tensors to reuse). Conflicts are results: the context's
        status is not touched."""
        torch = _torch()
        if S.n != O.n or S.marker_words != O.marker_words:
            raise CrdtError(-1, "LWWBatch shapes differ")
        dev = S.val.device
        if bitmap is None and want_bitmap:
            bitmap = torch.zeros((S.n + 63) // 64, dtype=torch.int64, device=dev)
        if count is None and want_count:
            count = torch.zeros(1, dtype=torch.int64, device=dev)
        if bitmap is not None and bitmap.numel() < (S.n + 63) // 64:
            raise CrdtError(-4, "conflict bitmap too small")
        check(lib.crdt_lwwreg_merge(self.ctx, _p(S.val), _p(S.marker), _p(O.val), _p(O.marker), S.n, S.marker_words,
                                    _p(bitmap), _p(count), self._stream(stream)), "lwwreg_merge")
        return bitmap, count

    def lwwreg_apply(self, S: LWWBatch, ops: LWWOps, want_op_err=False, n_err=None, stream=None, check_status=True):
        """In place: register i applies its op list in order (src/lwwreg.rs
        :69-77). Returns n_err (int32 [n]: register i's erring ops), or (n_err,
        op_err) with want_op_err (uint8 [n_ops]: op j's Result, 1 = Err)."""
        torch = _torch()
        if ops.n_obj != S.n or ops.marker_words != S.marker_words:
            raise CrdtError(-1, "LWWOps does not match the batch")
        dev = S.val.device
        if n_err is None:  # (`n_err`: an int32 [n] tensor to reuse; every entry is written)
            n_err = torch.empty(S.n, dtype=torch.int32, device=dev)
        op_err = torch.zeros(ops.n_ops, dtype=torch.uint8, device=dev) if want_op_err else None
        c = ops.cops()
        self._done(lib.crdt_lwwreg_apply(self.ctx, _p(S.val), _p(S.marker), C.byref(c), S.n, S.marker_words,
                                         _p(n_err), _p(op_err), self._stream(stream)),
                   "lwwreg_apply", stream, check_status)
        return (n_err, op_err) if want_op_err else n_err

    def lwwreg_fold(self, reps, out: LWWBatch | None = None, want_n_err=True, n_err=None, stream=None):
        """out[i] = reps[0][i].merge(reps[1][i]).merge(reps[2][i])... in rank
        order, one pass. Returns (out, n_err): n_err int32 [n] counts register
        i's erring merges (None when not wanted). `out` may be reps[0]."""
        torch = _torch()
        R0 = reps[0]
        if any(B.n != R0.n or B.marker_words != R0.marker_words for B in reps):
            raise CrdtError(-1, "LWWBatch shapes differ")
        if out is None:
            out = LWWBatch(torch.empty_like(R0.val), torch.empty_like(R0.marker))
        if n_err is None and want_n_err:  # (`n_err`: an int32 [n] tensor to reuse)
            n_err = torch.empty(R0.n, dtype=torch.int32, device=R0.val.device)
        views = (LWWViewC * max(1, len(reps)))(*[B.view() for B in reps])
        check(lib.crdt_lwwreg_fold(self.ctx, views, len(reps), R0.n, R0.marker_words, _p(out.val), _p(out.marker),
                                   _p(n_err), self._stream(stream)), "lwwreg_fold")
        return out, n_err

    def lwwreg_from_bincode(self, blobs, n, val_bytes, marker_bytes, stride=None, out: LWWBatch | None = None,
                            stream=None):
        """to_binary blobs of LWWReg<V, M> (val then the marker words, fixed-width
        little-endian; marker_bytes an int or a 2-tuple) at blobs[i * stride]
        (uint8 device tensor; stride defaults to the blob size) -> LWWBatch."""
        torch = _torch()
        mb = _words(marker_bytes)
        size = blob_bytes(val_bytes, mb)
        stride = size if stride is None else int(stride)
        if n and blobs.numel() < (n - 1) * stride + size:
            raise CrdtError(-1, "blob buffer too small")
        if out is None:
            out = LWWBatch(torch.empty(n, dtype=torch.int64, device=blobs.device),
                           torch.empty((n, len(mb)), dtype=torch.int64, device=blobs.device))
        check(lib.crdt_lwwreg_from_bincode(self.ctx, _p(blobs), stride, n, val_bytes, len(mb), mb[0], mb[-1],
                                           _p(out.val), _p(out.marker), self._stream(stream)), "lwwreg_from_bincode")
        return out

    def lwwreg_to_bincode(self, S: LWWBatch, val_bytes, marker_bytes, stride=None, out=None, stream=None,
                          check_status=True):
        """-> uint8 device tensor, blob i at [i * stride] (stride defaults to
        the blob size; `out` is reused when given, bytes between blobs are not
        touched). A word too wide for its width latches CRDT_ENONCANON: that
        blob is not written."""
        torch = _torch()
        mb = _words(marker_bytes)
        if len(mb) != S.marker_words:
            raise CrdtError(-1, "marker_bytes does not match marker_words")
        size = blob_bytes(val_bytes, mb)
        stride = size if stride is None else int(stride)
        need = (S.n - 1) * stride + size if S.n else 0
        if out is None:
            out = torch.zeros(need, dtype=torch.uint8, device=S.val.device)
        elif out.numel() < need:
            raise CrdtError(-4, "blob buffer too small")
        self._done(lib.crdt_lwwreg_to_bincode(self.ctx, _p(S.val), _p(S.marker), S.n, val_bytes, len(mb), mb[0],
                                              mb[-1], _p(out), stride, self._stream(stream)),
                   "lwwreg_to_bincode", stream, check_status)
        return out
