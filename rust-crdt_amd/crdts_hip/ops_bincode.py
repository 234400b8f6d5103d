"""bincode codec of the Orswot, MVReg and Map op streams: the Engine methods
over crdt_ops_bincode_clk_lens / crdt_ops_from_bincode / crdt_ops_bincode_sizes
/ crdt_ops_to_bincode (include/crdts_hip.h "bincode of the Orswot, MVReg and
Map ops"), and the from_bincode / to_bincode of the five op batch classes.

    Orswot Op  Add: 0 | A actor | u64 counter | M member    Rm: 1 | VClock | M member
    MVReg  Op  Put: 0 | VClock | V val
    Map    Op  Nop: 0    Rm: 1 | VClock | K key    Up: 2 | A actor | u64 counter | K key | <V::Op>
    VClock     u64 n | n x (A actor | u64 counter), actors ascending

Blobs are uint8 device tensors; offsets, lengths and sizes int64 tensors
holding u64 values. Widths are (actor_bytes, key_bytes, key2_bytes, val_bytes);
a width the op type has no field for is ignored (pass 0)."""
from __future__ import annotations

import ctypes as C

from ._lib import CRDT_EINVAL, CRDT_ENONCANON, OP_ARRAYS_FIELDS, OP_LAYOUTS, CrdtError, OpArraysC, OpWidthsC, check, lib
from ._util import _torch, on_stream, ptr as _p

ORSWOT, MVREG, MAP_MVREG, MAP_ORSWOT, MAP_MAP = range(5)  # CRDT_OPS_*
KIND_BAD = 0xFFFFFFFF  # CRDT_OP_KIND_BAD
WIDTHS = (1, 2, 4, 8)
WIDTH_NAMES = ("actor_bytes", "key_bytes", "key2_bytes", "val_bytes")
USED_WIDTHS = {ORSWOT: (0, 2), MVREG: (0, 3), MAP_MVREG: (0, 1, 3), MAP_ORSWOT: (0, 1, 2), MAP_MAP: (0, 1, 2, 3)}
USED_FIELDS = {
    ORSWOT: ("kind", "actor", "counter", "key2"),
    MVREG: ("val",),
    MAP_MVREG: ("kind", "key", "actor", "counter", "val"),
    MAP_ORSWOT: ("kind", "key", "actor", "counter", "key2"),
    MAP_MAP: ("kind", "key", "actor", "counter", "key2", "actor2", "counter2", "val"),
}
U32_FIELDS = OP_LAYOUTS["crdt_op_arrays"].u32
# per batch class: its op type, and its tensors after obj_end named as in crdt_op_arrays (views of _lib.OP_LAYOUTS)
LAYOUT = {l.batch: (l.op_type, l.wire) for l in OP_LAYOUTS.values() if l.op_type is not None}


def check_widths(op_type, widths):
    """(actor, key, key2, val) bytes -> the same tuple of ints, the ones
    op_type uses checked against {1, 2, 4, 8}."""
    if op_type not in USED_WIDTHS:
        raise CrdtError(CRDT_EINVAL, f"op_type {op_type!r} is not one of 0..4")
    w = tuple(int(x or 0) for x in widths)
    if len(w) != 4:
        raise CrdtError(CRDT_EINVAL, "widths are (actor_bytes, key_bytes, key2_bytes, val_bytes)")
    for k in USED_WIDTHS[op_type]:
        if w[k] not in WIDTHS:
            raise CrdtError(CRDT_EINVAL, f"{WIDTH_NAMES[k]} {w[k]!r} is not one of {WIDTHS}")
    return w


def op_blob_bytes(op_type, kind, n_pairs, widths):
    """Size of one op blob: `kind` as in the crdt_*_ops struct of op_type
    (ignored for MVREG), n_pairs clock pairs."""
    wa, wk, w2, wv = check_widths(op_type, widths)
    dot, clock = wa + 8, 8 + int(n_pairs) * (wa + 8)
    if op_type == ORSWOT:
        sizes, clocked = {0: 4 + dot + w2, 1: 4 + clock + w2}, (1,)
    elif op_type == MVREG:
        kind, sizes, clocked = 0, {0: 4 + clock + wv}, (0,)
    else:
        up = 4 + dot + wk + 4
        sizes, clocked = {0: 4, 1: 4 + clock + wk}, (1, 2, 3)
        if op_type == MAP_MVREG:
            sizes[2] = up + clock + wv
        elif op_type == MAP_ORSWOT:
            sizes[2], sizes[3], clocked = up + dot + w2, up + clock + w2, (1, 3)
        else:
            sizes[2], sizes[3], sizes[4] = up + dot + w2 + 4 + clock + wv, up + clock + w2, up
    if kind not in sizes:
        raise CrdtError(CRDT_ENONCANON, f"op type {op_type} has no kind {kind}")
    if n_pairs and kind not in clocked:
        raise CrdtError(CRDT_ENONCANON, f"kind {kind} of op type {op_type} carries no clock")
    return sizes[kind]


def _cwidths(op_type, widths):
    return OpWidthsC(*check_widths(op_type, widths))


def _carrays(arrays, n_ops, n_clk):
    return OpArraysC(*[_p(arrays.get(f)) for f in OP_ARRAYS_FIELDS], n_ops, n_clk)


class OpsBincodeEngine:
    """Engine's op-stream codec methods (mixed into crdts_hip.Engine)."""

    def ops_clk_lens(self, blobs, blob_off, blob_len, op_type, widths, stream=None, check_status=True):
        """Clock pairs of every op blob, from its framing alone -> int32 [n_ops]
        (a badly framed op: 0, or 1 for MVREG, and CRDT_ENONCANON)."""
        torch = _torch()
        n = int(blob_off.numel())
        if blob_len.numel() != n:
            raise CrdtError(CRDT_EINVAL, "blob_off / blob_len lengths differ")
        w = _cwidths(op_type, widths)
        lens = torch.zeros(n, dtype=torch.int32, device=blobs.device)
        self._done(lib.crdt_ops_bincode_clk_lens(self.ctx, _p(blobs), int(blobs.numel()), _p(blob_off), _p(blob_len),
                                                 n, op_type, C.byref(w), _p(lens), self._stream(stream)),
                   "ops_clk_lens", stream, check_status)
        return lens

    def ops_from_bincode(self, blobs, blob_off, blob_len, op_type, widths, op_err=False, stream=None,
                         check_status=True):
        """Op blobs -> a dict of device tensors named as in crdt_op_arrays (the
        fields op_type uses, clk_end, clk_act, clk_ctr; `op_err`: also the
        per-op codes, int32): the framing pass, a cumsum on the device, then
        the fields and the pairs. A bad op has kind KIND_BAD and zero fields."""
        torch = _torch()
        n, dev = int(blob_off.numel()), blobs.device
        lens = self.ops_clk_lens(blobs, blob_off, blob_len, op_type, widths, stream, check_status=False)
        with on_stream(stream):
            clk_end = torch.cumsum(lens.to(torch.int64), 0)
            n_clk = int(clk_end[-1].item()) if n else 0
            a = {f: torch.empty(n, dtype=torch.int32 if f in U32_FIELDS else torch.int64, device=dev)
                 for f in USED_FIELDS[op_type]}
            a["clk_end"] = clk_end
            a["clk_act"] = torch.empty(n_clk, dtype=torch.int32, device=dev)
            a["clk_ctr"] = torch.empty(n_clk, dtype=torch.int64, device=dev)
            err = torch.zeros(n, dtype=torch.int32, device=dev) if op_err else None
        w, c = _cwidths(op_type, widths), _carrays(a, n, n_clk)
        self._done(lib.crdt_ops_from_bincode(self.ctx, _p(blobs), int(blobs.numel()), _p(blob_off), _p(blob_len),
                                             op_type, C.byref(w), C.byref(c), _p(err), self._stream(stream)),
                   "ops_from_bincode", stream, check_status)
        if op_err:
            a["op_err"] = err
        return a

    def ops_to_bincode(self, op_type, widths, arrays, stream=None, check_status=True):
        """A dict of device tensors named as in crdt_op_arrays -> (blobs uint8,
        blob_off int64, blob_len int64), packed back to back (sizes, exclusive
        scan, write). An op that cannot be written has length 0
        (CRDT_ENONCANON)."""
        torch = _torch()
        w = _cwidths(op_type, widths)
        missing = [f for f in USED_FIELDS[op_type] + ("clk_end", "clk_act", "clk_ctr") if arrays.get(f) is None]
        if missing:
            raise CrdtError(CRDT_EINVAL, f"ops_to_bincode: missing arrays {missing}")
        n, n_clk = int(arrays["clk_end"].numel()), int(arrays["clk_act"].numel())
        c, st = _carrays(arrays, n, n_clk), self._stream(stream)
        lens = torch.zeros(n, dtype=torch.int64, device=arrays["clk_end"].device)
        check(lib.crdt_ops_bincode_sizes(self.ctx, op_type, C.byref(w), C.byref(c), _p(lens), st), "ops_bincode_sizes")
        out, off = self._placed(lens, stream)
        self._done(lib.crdt_ops_to_bincode(self.ctx, op_type, C.byref(w), C.byref(c), _p(out), _p(off),
                                           int(out.numel()), st), "ops_to_bincode", stream, check_status)
        return out, off, lens


def _layout(cls):
    """The layout of an op-stream batch class (its own or an ancestor's)."""
    lay = getattr(cls, "LAYOUT", None)
    if lay is None or lay.op_type is None:
        raise CrdtError(CRDT_EINVAL, f"{cls.__name__} is not an op batch class")
    return lay


def ops_from_wire(cls, blobs, blob_off, blob_len, obj_end, widths, engine=None, stream=None, check_status=True):
    """cls.from_bincode: op blobs -> an op batch of class cls. obj_end (int64
    device tensor, or a host array) groups the ops: grouping is not on the
    wire."""
    import numpy as np

    from .host_model import default_engine

    torch = _torch()
    engine = engine or default_engine()
    if not torch.is_tensor(obj_end):
        obj_end = torch.from_numpy(np.ascontiguousarray(np.asarray(obj_end, np.uint64)).view(np.int64)).to(
            blobs.device)
    lay = _layout(cls)
    a = engine.ops_from_bincode(blobs, blob_off, blob_len, lay.op_type, widths, stream=stream,
                                check_status=check_status)
    return cls(obj_end, *[a[f] for f in lay.wire])


def ops_to_wire(ops, widths, engine=None, stream=None, check_status=True):
    """ops.to_bincode: an op batch -> (blobs, blob_off, blob_len)."""
    from .host_model import default_engine

    lay = _layout(type(ops))
    return (engine or default_engine()).ops_to_bincode(lay.op_type, widths, dict(zip(lay.wire, ops.t[1:])), stream,
                                                       check_status)
