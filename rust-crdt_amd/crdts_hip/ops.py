"""The op and query batches that cross the C ABI: per-object op lists as flat
arrays with inclusive ends (the crdt_*_ops structs and crdt_read_queries).
Each class names its struct's layout (_lib.OP_LAYOUTS) and says how its ops
are written down; packing, the C struct and the wire form come from the
layout."""
from __future__ import annotations

import numpy as np

from ._lib import OP_LAYOUTS
from ._util import _torch, longest_op_list, ptr, put


class OpBatch:
    """A batch of ops or queries, grouped per object in order: `t`, the
    tensors of the struct's arrays in ABI order (int32 / int64 holding u32 /
    u64 bits; None for an optional array that is absent), n_obj, and the
    struct's counts (n_ops and n_clk, or n_q) as attributes."""

    LAYOUT = None  # the struct's _lib.OpLayout

    def __init__(self, *tensors):
        lay = self.LAYOUT
        assert len(tensors) == len(lay.fields)
        self.t = tuple(tensors)
        self.n_obj = int(tensors[0].numel())
        for count, f in lay.counts:
            setattr(self, count, int(tensors[lay.fields.index(f)].numel()))

    def cops(self):
        lay = self.LAYOUT
        return lay.ctype(*[ptr(t) for t in self.t], *[getattr(self, c) for c, _ in lay.counts])

    max_ops = None  # the longest op list, where a class records it at pack time

    def longest(self):
        """The longest per-object op list, by which an apply sizes a default
        output: max_ops where it is known, else obj_end is copied to the host
        to find it, which synchronises."""
        if self.max_ops is not None:
            return self.max_ops
        return longest_op_list(self.t[0].cpu().numpy().view(np.uint64)) if self.n_obj else 0

    @classmethod
    def from_arrays(cls, *arrays, device=0):
        """Host numpy arrays (u64 / u32 as in the struct, in its order) -> device
        (device None: the tensors stay on the host); not validated."""
        lay = cls.LAYOUT
        return cls(*[put(x, f in lay.u32, device) for f, x in zip(lay.fields, arrays)])

    @classmethod
    def from_lists(cls, per_obj, device=0):
        """per_obj[i] = object i's ops, as for arrays_from_lists."""
        return cls.from_arrays(*cls.arrays_from_lists(per_obj), device=device)

    @classmethod
    def _from_wire(cls, blobs, blob_off, blob_len, obj_end, widths, engine, stream, check_status):
        """cls.from_bincode: widths are (actor, key, key2, val) bytes, 0 where the op type has no such field."""
        from .ops_bincode import ops_from_wire

        return ops_from_wire(cls, blobs, blob_off, blob_len, obj_end, widths, engine, stream, check_status)

    def _to_wire(self, widths, engine, stream, check_status):
        """The ops' wire form -> (blobs uint8, blob_off int64, blob_len int64),
        packed back to back (crdt_ops_to_bincode)."""
        from .ops_bincode import ops_to_wire

        return ops_to_wire(self, widths, engine, stream, check_status)


def _host_arrays(layout, lists):
    """{field: list} -> the struct's host arrays in ABI order, u32 / u64."""
    return tuple(np.asarray(lists[f], np.uint32 if f in layout.u32 else np.uint64) for f in layout.fields)


class OrswotOps(OpBatch):
    """A batch of Orswot ops (Op::Add / Op::Rm, src/orswot.rs:38-53) on the
    device, grouped per object in order (crdt_orswot_ops)."""

    LAYOUT = OP_LAYOUTS["crdt_orswot_ops"]
    ADD, RM = 0, 1

    def __init__(self, obj_end, kind, member, actor, counter, clk_end, clk_act, clk_ctr):
        super().__init__(obj_end, kind, member, actor, counter, clk_end, clk_act, clk_ctr)

    @classmethod
    def arrays_from_lists(cls, per_obj):
        """per_obj[i] = [("add", actor, counter, member) | ("rm", member, [(actor, counter), ...]), ...]
        -> the eight host arrays of crdt_orswot_ops."""
        a = {f: [] for f in cls.LAYOUT.fields}
        for ops in per_obj:
            for op in ops:
                if op[0] == "add":
                    a["kind"].append(cls.ADD); a["actor"].append(op[1]); a["counter"].append(op[2])
                    a["member"].append(op[3])
                else:
                    a["kind"].append(cls.RM); a["actor"].append(0); a["counter"].append(0); a["member"].append(op[1])
                    for x, c in op[2]:
                        a["clk_act"].append(x); a["clk_ctr"].append(c)
                a["clk_end"].append(len(a["clk_act"]))
            a["obj_end"].append(len(a["kind"]))
        return _host_arrays(cls.LAYOUT, a)

    @classmethod
    def from_bincode(cls, blobs, blob_off, blob_len, obj_end, actor_bytes, member_bytes, engine=None,
                     stream=None, check_status=True):
        """Orswot Op<M, A> blobs (src/orswot.rs:36-53) as they travel between
        replicas — blob j is blobs[blob_off[j] : blob_off[j] + blob_len[j]] (uint8
        / int64 device tensors) — -> an op batch (crdt_ops_from_bincode). obj_end (int64
        device tensor, or a host array) groups them: grouping is not on the
        wire. A malformed op gets the kind every apply rejects
        (CRDT_ENONCANON here too)."""
        return cls._from_wire(blobs, blob_off, blob_len, obj_end, (actor_bytes, 0, member_bytes, 0), engine, stream,
                              check_status)

    def to_bincode(self, actor_bytes, member_bytes, engine=None, stream=None, check_status=True):
        """The ops' wire form -> (blobs uint8, blob_off int64, blob_len int64),
        packed back to back (crdt_ops_to_bincode)."""
        return self._to_wire((actor_bytes, 0, member_bytes, 0), engine, stream, check_status)


class MapOps(OpBatch):
    """A batch of Map<u64, MVReg<u64, A>, A> ops (Op::Nop / Op::Rm / Op::Up
    with an MVReg Put, src/map.rs:104-125) on the device, grouped per object in
    order (crdt_map_mvreg_ops)."""

    LAYOUT = OP_LAYOUTS["crdt_map_mvreg_ops"]
    NOP, RM, UP = 0, 1, 2

    def __init__(self, obj_end, kind, key, actor, counter, val, clk_end, clk_act, clk_ctr):
        super().__init__(obj_end, kind, key, actor, counter, val, clk_end, clk_act, clk_ctr)

    @classmethod
    def from_arrays(cls, obj_end, kind, key, actor, counter, val, clk_end, clk_act, clk_ctr, device=0):
        """Host numpy arrays (u64 / u32 as in crdt_map_mvreg_ops) -> device."""
        return super().from_arrays(obj_end, kind, key, actor, counter, val, clk_end, clk_act, clk_ctr, device=device)

    @staticmethod
    def arrays_from_lists(per_obj):
        """per_obj[i] = [("up", actor, counter, key, [(a, c), ...], val) | ("rm", key, [(a, c), ...]) | ("nop",), ...]
        -> the nine host arrays of crdt_map_mvreg_ops."""
        a = {f: [] for f in MapOps.LAYOUT.fields}
        for ops in per_obj:
            for op in ops:
                if op[0] == "up":
                    kind, (actor, counter, key, pairs, val) = MapOps.UP, op[1:6]
                elif op[0] == "rm":
                    kind, actor, counter, key, pairs, val = MapOps.RM, 0, 0, op[1], op[2], 0
                elif op[0] == "nop":
                    kind, actor, counter, key, pairs, val = MapOps.NOP, 0, 0, 0, (), 0
                else:
                    raise ValueError(f"unknown map op {op[0]!r}")
                a["kind"].append(kind); a["actor"].append(actor); a["counter"].append(counter); a["key"].append(key)
                a["val"].append(val)
                for x, c in pairs:
                    a["clk_act"].append(x); a["clk_ctr"].append(c)
                a["clk_end"].append(len(a["clk_act"]))
            a["obj_end"].append(len(a["kind"]))
        return _host_arrays(MapOps.LAYOUT, a)

    @classmethod
    def from_bincode(cls, blobs, blob_off, blob_len, obj_end, actor_bytes, key_bytes, val_bytes, engine=None,
                     stream=None, check_status=True):
        """Map<K, MVReg> Op blobs (src/map.rs:102-123) as they travel between
        replicas — blob j is blobs[blob_off[j] : blob_off[j] + blob_len[j]] (uint8
        / int64 device tensors) — -> an op batch (crdt_ops_from_bincode). obj_end (int64
        device tensor, or a host array) groups them: grouping is not on the
        wire. A malformed op gets the kind every apply rejects
        (CRDT_ENONCANON here too)."""
        return cls._from_wire(blobs, blob_off, blob_len, obj_end, (actor_bytes, key_bytes, 0, val_bytes), engine,
                              stream, check_status)

    def to_bincode(self, actor_bytes, key_bytes, val_bytes, engine=None, stream=None, check_status=True):
        """The ops' wire form -> (blobs uint8, blob_off int64, blob_len int64),
        packed back to back (crdt_ops_to_bincode)."""
        return self._to_wire((actor_bytes, key_bytes, 0, val_bytes), engine, stream, check_status)


class MVRegOps(OpBatch):
    """A batch of MVReg<u64, A> ops (Op::Put { clock, val }, src/mvreg.rs:51-59)
    on the device, grouped per object in order (crdt_mvreg_ops)."""

    LAYOUT = OP_LAYOUTS["crdt_mvreg_ops"]

    def __init__(self, obj_end, val, clk_end, clk_act, clk_ctr, max_ops=None):
        super().__init__(obj_end, val, clk_end, clk_act, clk_ctr)
        self.max_ops = max_ops  # the longest op list, recorded at pack time (None: not known on the host)

    @classmethod
    def from_arrays(cls, obj_end, val, clk_end, clk_act, clk_ctr, device=0):
        """Host numpy arrays (u64 / u32 as in crdt_mvreg_ops) -> device; not validated."""
        ops = super().from_arrays(obj_end, val, clk_end, clk_act, clk_ctr, device=device)
        ops.max_ops = longest_op_list(obj_end)
        return ops

    @staticmethod
    def arrays_from_lists(per_obj):
        """per_obj[i] = [(clock_pairs, val), ...] with clock_pairs = [(actor, counter), ...]
        -> the five host arrays of crdt_mvreg_ops. A clock must be canonical
        (actors strictly increasing, counters > 0): ValueError otherwise."""
        a = {f: [] for f in MVRegOps.LAYOUT.fields}
        for i, ops in enumerate(per_obj):
            for pairs, v in ops:
                prev = -1
                for x, c in pairs:
                    if x <= prev:
                        raise ValueError(f"object {i}: clock actors not strictly increasing: {list(pairs)!r}")
                    if c <= 0:
                        raise ValueError(f"object {i}: zero counter in clock {list(pairs)!r}")
                    prev = x
                    a["clk_act"].append(x); a["clk_ctr"].append(c)
                a["clk_end"].append(len(a["clk_act"]))
                a["val"].append(v)
            a["obj_end"].append(len(a["val"]))
        return _host_arrays(MVRegOps.LAYOUT, a)

    @classmethod
    def from_bincode(cls, blobs, blob_off, blob_len, obj_end, actor_bytes, val_bytes, engine=None,
                     stream=None, check_status=True):
        """MVReg Op<V, A> blobs (src/mvreg.rs:49-59) as they travel between
        replicas — blob j is blobs[blob_off[j] : blob_off[j] + blob_len[j]] (uint8
        / int64 device tensors) — -> an op batch (crdt_ops_from_bincode). obj_end (int64
        device tensor, or a host array) groups them: grouping is not on the
        wire. A malformed op gets the kind every apply rejects
        (CRDT_ENONCANON here too)."""
        return cls._from_wire(blobs, blob_off, blob_len, obj_end, (actor_bytes, 0, 0, val_bytes), engine, stream,
                              check_status)

    def to_bincode(self, actor_bytes, val_bytes, engine=None, stream=None, check_status=True):
        """The ops' wire form -> (blobs uint8, blob_off int64, blob_len int64),
        packed back to back (crdt_ops_to_bincode)."""
        return self._to_wire((actor_bytes, 0, 0, val_bytes), engine, stream, check_status)


class MapMapOps(OpBatch):
    """A batch of Map<u64, Map<u64, MVReg<u64, A>, A>, A> ops (the reference's
    TestMap: Op::Nop / Op::Rm / Op::Up whose inner op is again a Map op,
    src/map.rs:104-125) on the device, grouped per object in order
    (crdt_map_map_ops). Ops are given in their literal JSON form:

        "nop"
        {"rm": {"clock": [[a, c], ...], "key": k}}
        {"up": {"dot": [a, c], "key": k, "op": INNER}}
        INNER = "nop" | {"rm": {"clock": [...], "key": k2}}
              | {"up": {"dot": [a2, c2], "key": k2, "op": {"put": {"clock": [...], "val": v}}}}"""

    LAYOUT = OP_LAYOUTS["crdt_map_map_ops"]
    NOP, RM, UP_UP, UP_RM, UP_NOP = 0, 1, 2, 3, 4
    FIELDS, U32 = LAYOUT.fields, LAYOUT.u32

    @staticmethod
    def arrays_from_lists(per_obj):
        """per_obj[i] = the object's ops in their JSON form -> the twelve host
        arrays of crdt_map_map_ops, in FIELDS order. Fields an op does not
        have are 0; an op's clock pairs are the outer Rm's clock, the inner
        Rm's clock or the inner Up's Put clock."""
        a = {f: [] for f in MapMapOps.FIELDS}
        for ops in per_obj:
            for op in ops:
                kind, key, dot, key2, dot2, val, pairs = MapMapOps.NOP, 0, (0, 0), 0, (0, 0), 0, ()
                if op == "nop":
                    pass
                elif "rm" in op:
                    kind, key, pairs = MapMapOps.RM, op["rm"]["key"], op["rm"]["clock"]
                elif "up" in op:
                    up = op["up"]
                    key, dot, inner = up["key"], up["dot"], up["op"]
                    if inner == "nop":
                        kind = MapMapOps.UP_NOP
                    elif "rm" in inner:
                        kind, key2, pairs = MapMapOps.UP_RM, inner["rm"]["key"], inner["rm"]["clock"]
                    elif "up" in inner:
                        put_ = inner["up"]["op"]["put"]
                        kind, key2, dot2 = MapMapOps.UP_UP, inner["up"]["key"], inner["up"]["dot"]
                        val, pairs = put_["val"], put_["clock"]
                    else:
                        raise ValueError(f"unknown inner map op {inner!r}")
                else:
                    raise ValueError(f"unknown map op {op!r}")
                a["kind"].append(kind); a["key"].append(key); a["actor"].append(dot[0]); a["counter"].append(dot[1])
                a["key2"].append(key2); a["actor2"].append(dot2[0]); a["counter2"].append(dot2[1]); a["val"].append(val)
                for x, c in pairs:
                    a["clk_act"].append(x); a["clk_ctr"].append(c)
                a["clk_end"].append(len(a["clk_act"]))
            a["obj_end"].append(len(a["kind"]))
        return _host_arrays(MapMapOps.LAYOUT, a)

    @classmethod
    def from_bincode(cls, blobs, blob_off, blob_len, obj_end, actor_bytes, key_bytes, inner_key_bytes, val_bytes,
                     engine=None, stream=None, check_status=True):
        """Map<K, Map<K2, MVReg>> Op blobs (src/map.rs:102-123) as they travel between
        replicas — blob j is blobs[blob_off[j] : blob_off[j] + blob_len[j]] (uint8
        / int64 device tensors) — -> an op batch (crdt_ops_from_bincode). obj_end (int64
        device tensor, or a host array) groups them: grouping is not on the
        wire. A malformed op gets the kind every apply rejects
        (CRDT_ENONCANON here too)."""
        return cls._from_wire(blobs, blob_off, blob_len, obj_end,
                              (actor_bytes, key_bytes, inner_key_bytes, val_bytes), engine, stream, check_status)

    def to_bincode(self, actor_bytes, key_bytes, inner_key_bytes, val_bytes, engine=None, stream=None,
                   check_status=True):
        """The ops' wire form -> (blobs uint8, blob_off int64, blob_len int64),
        packed back to back (crdt_ops_to_bincode)."""
        return self._to_wire((actor_bytes, key_bytes, inner_key_bytes, val_bytes), engine, stream, check_status)


class MapOrswotOps(OpBatch):
    """A batch of Map<u64, Orswot<u64, A>, A> ops (Op::Nop / Op::Rm / Op::Up
    with an Orswot Add or Rm, src/map.rs:104-125) on the device, grouped per
    object in order (crdt_map_orswot_ops). The nested Add's dot is the Up's."""

    LAYOUT = OP_LAYOUTS["crdt_map_orswot_ops"]
    NOP, RM, UP, UP_RM = 0, 1, 2, 3

    def __init__(self, obj_end, kind, key, actor, counter, member, clk_end, clk_act, clk_ctr):
        super().__init__(obj_end, kind, key, actor, counter, member, clk_end, clk_act, clk_ctr)

    @classmethod
    def from_arrays(cls, obj_end, kind, key, actor, counter, member, clk_end, clk_act, clk_ctr, device=0):
        """Host numpy arrays (u64 / u32 as in crdt_map_orswot_ops) -> device."""
        return super().from_arrays(obj_end, kind, key, actor, counter, member, clk_end, clk_act, clk_ctr,
                                   device=device)

    @staticmethod
    def arrays_from_lists(per_obj):
        """per_obj[i] = [("up_add", actor, counter, key, member) | ("up_rm", actor, counter, key, member,
        [(a, c), ...]) | ("rm", key, [(a, c), ...]) | ("nop",), ...] -> the nine host arrays of
        crdt_map_orswot_ops."""
        a = {f: [] for f in MapOrswotOps.LAYOUT.fields}
        for ops in per_obj:
            for op in ops:
                if op[0] == "up_add":
                    kind, (actor, counter, key, member), pairs = MapOrswotOps.UP, op[1:5], ()
                elif op[0] == "up_rm":
                    kind, (actor, counter, key, member, pairs) = MapOrswotOps.UP_RM, op[1:6]
                elif op[0] == "rm":
                    kind, actor, counter, key, member, pairs = MapOrswotOps.RM, 0, 0, op[1], 0, op[2]
                elif op[0] == "nop":
                    kind, actor, counter, key, member, pairs = MapOrswotOps.NOP, 0, 0, 0, 0, ()
                else:
                    raise ValueError(f"unknown map op {op[0]!r}")
                a["kind"].append(kind); a["actor"].append(actor); a["counter"].append(counter); a["key"].append(key)
                a["member"].append(member)
                for x, c in pairs:
                    a["clk_act"].append(x); a["clk_ctr"].append(c)
                a["clk_end"].append(len(a["clk_act"]))
            a["obj_end"].append(len(a["kind"]))
        return _host_arrays(MapOrswotOps.LAYOUT, a)

    @classmethod
    def from_bincode(cls, blobs, blob_off, blob_len, obj_end, actor_bytes, key_bytes, member_bytes, engine=None,
                     stream=None, check_status=True):
        """Map<K, Orswot> Op blobs (src/map.rs:102-123; the nested Add's dot is the Up's) as they travel between
        replicas — blob j is blobs[blob_off[j] : blob_off[j] + blob_len[j]] (uint8
        / int64 device tensors) — -> an op batch (crdt_ops_from_bincode). obj_end (int64
        device tensor, or a host array) groups them: grouping is not on the
        wire. A malformed op gets the kind every apply rejects
        (CRDT_ENONCANON here too)."""
        return cls._from_wire(blobs, blob_off, blob_len, obj_end, (actor_bytes, key_bytes, member_bytes, 0), engine,
                              stream, check_status)

    def to_bincode(self, actor_bytes, key_bytes, member_bytes, engine=None, stream=None, check_status=True):
        """The ops' wire form -> (blobs uint8, blob_off int64, blob_len int64),
        packed back to back (crdt_ops_to_bincode)."""
        return self._to_wire((actor_bytes, key_bytes, member_bytes, 0), engine, stream, check_status)


class ClockOps(OpBatch):
    """A batch of dots for the clocks' op path (crdt_clock_ops), grouped per
    object: VClock::apply / GCounter::apply take (actor, counter) dots
    (src/vclock.rs:126-128, src/gcounter.rs:53-55), PNCounter::apply
    (src/pncounter.rs:82-87) also a direction (0 = Dir::Pos, 1 = Dir::Neg); the
    get calls read the actors only. Tensors: obj_end int64 [n_obj], actor int32
    [n_ops], counter int64 [n_ops] (u64 bits), dir int32 [n_ops] or None.
    `host` keeps the numpy arrays the batch was packed from (None when it was
    built from device tensors)."""

    LAYOUT = OP_LAYOUTS["crdt_clock_ops"]

    def __init__(self, obj_end, actor, counter, dir_=None, host=None):
        super().__init__(obj_end, actor, counter, dir_)
        self.host = host

    @classmethod
    def from_arrays(cls, obj_end, actor, counter=None, dir_=None, device=0):
        """Host numpy arrays (u64 / u32 as in crdt_clock_ops) -> device; not
        validated. counter None: zeros (a query batch); device None: the
        tensors stay on the host."""
        obj_end = np.ascontiguousarray(np.asarray(obj_end, dtype=np.uint64))
        actor = np.ascontiguousarray(np.asarray(actor, dtype=np.uint32))
        counter = np.zeros(actor.size, np.uint64) if counter is None else \
            np.ascontiguousarray(np.asarray(counter, dtype=np.uint64))
        dir_ = None if dir_ is None else np.ascontiguousarray(np.asarray(dir_, dtype=np.uint32))
        ops = super().from_arrays(obj_end, actor, counter, dir_, device=device)
        ops.host = (obj_end, actor, counter, dir_)
        return ops

    @staticmethod
    def arrays_from_lists(per_obj, with_dir=False):
        """per_obj[i] = [(actor, counter), ...] — or [(actor, counter, dir), ...]
        with with_dir, or bare actors for a query batch — -> (obj_end u64
        [n_obj], actor u32 [n_ops], counter u64 [n_ops], dir u32 [n_ops] or None)."""
        ends, act, ctr, dr = [], [], [], []
        for ops in per_obj:
            for op in ops:
                op = op if isinstance(op, (tuple, list)) else (op, 0)
                act.append(op[0]); ctr.append(op[1])
                if with_dir:
                    dr.append(op[2])
            ends.append(len(act))
        return (np.asarray(ends, np.uint64), np.asarray(act, np.uint32), np.asarray(ctr, np.uint64),
                np.asarray(dr, np.uint32) if with_dir else None)

    @classmethod
    def from_lists(cls, per_obj, with_dir=False, device=0):
        """per_obj[i] = object i's dots, see arrays_from_lists."""
        return cls.from_arrays(*cls.arrays_from_lists(per_obj, with_dir), device=device)

    # The dots' wire form is fixed-size blobs at a stride (crdt_clock_ops_*_bincode),
    # not the length-framed stream of the other op types: a codec of its own.
    @classmethod
    def from_bincode(cls, blobs, stride, obj_end, actor_bytes, with_dir=False, engine=None, stream=None,
                     check_status=True):
        """Op blobs as they travel between replicas — Dot<A> (src/vclock.rs:33-39),
        or PNCounter's Op with with_dir (src/pncounter.rs:39-56) — at blobs[j *
        stride] (uint8 device tensor; stride None: the op size) -> ClockOps.
        obj_end (int64 device tensor, or a host array) groups them: grouping is
        not on the wire. A malformed op becomes the sentinel every apply skips
        and latches (CRDT_ENONCANON here too)."""
        from .host_model import default_engine

        torch = _torch()
        engine = engine or default_engine()
        if not torch.is_tensor(obj_end):
            obj_end = torch.from_numpy(np.ascontiguousarray(np.asarray(obj_end, np.uint64)).view(np.int64)).to(
                blobs.device)
        n_ops = int(obj_end[-1].item()) if obj_end.numel() else 0
        actor, counter, dir_ = engine.clock_ops_from_bincode(blobs, n_ops, actor_bytes, with_dir, stride, stream,
                                                             check_status)
        return cls(obj_end, actor, counter, dir_)

    def to_bincode(self, actor_bytes, stride=None, out=None, engine=None, stream=None, check_status=True):
        """The ops' wire form: a uint8 device tensor, op j at [j * stride]
        (PNCounter's Op when the batch carries dir)."""
        from .host_model import default_engine

        engine = engine or default_engine()
        _, actor, counter, dir_ = self.t
        return engine.clock_ops_to_bincode(actor, counter, dir_, actor_bytes, stride, out, stream, check_status)


class ReadQueries(OpBatch):
    """A batch of reads (crdt_read_queries), grouped per object:
    Orswot::contains / Map::get (KEY) and Orswot::value / Map::len (ALL), each
    with the actor to derive an AddCtx for, or NO_ACTOR. Tensors: obj_end int64
    [n_obj], kind int32 [n_q], key int64 [n_q] (u64 bits), actor int32 [n_q] or
    None (no query names an actor)."""

    LAYOUT = OP_LAYOUTS["crdt_read_queries"]
    KEY, ALL = 0, 1
    NO_ACTOR = 0xFFFFFFFF
    NO_SLOT = 0xFFFFFFFF

    def __init__(self, obj_end, kind, key, actor=None):
        super().__init__(obj_end, kind, key, actor)

    cqueries = OpBatch.cops

    @classmethod
    def from_arrays(cls, obj_end, kind, key, actor=None, device=0):
        """Host numpy arrays (u64 / u32 as in crdt_read_queries) -> device; not
        validated. device None: the tensors stay on the host."""
        return super().from_arrays(obj_end, kind, key, actor, device=device)

    @staticmethod
    def arrays_from_lists(per_obj):
        """per_obj[i] = [("key", k) | ("key", k, actor) | ("all",) | ("all", actor), ...]
        -> (obj_end u64 [n_obj], kind u32 [n_q], key u64 [n_q], actor u32 [n_q]
        or None when no query names an actor). An actor of None is NO_ACTOR."""
        ends, kind, key, act = [], [], [], []
        for qs in per_obj:
            for q in qs:
                if q[0] == "key":
                    kind.append(ReadQueries.KEY); key.append(q[1]); a = q[2] if len(q) > 2 else None
                else:
                    kind.append(ReadQueries.ALL); key.append(0); a = q[1] if len(q) > 1 else None
                act.append(ReadQueries.NO_ACTOR if a is None else a)
            ends.append(len(kind))
        named = any(a != ReadQueries.NO_ACTOR for a in act)
        return (np.asarray(ends, np.uint64), np.asarray(kind, np.uint32), np.asarray(key, np.uint64),
                np.asarray(act, np.uint32) if named else None)
