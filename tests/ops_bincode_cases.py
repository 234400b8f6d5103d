"""Shared cases of the op-stream codec tests (tests/test_ops_bincode_ref.py,
tests/test_gpu_ops_bincode.py, tools/ops_bincode_bench.py) — test
infrastructure: the golden blobs, random ops whose values reach the largest
each width holds, the malformed blobs (one per CRDT_ENONCANON class of the
ingest) and the host packing of a flat op list into the arrays of
crdt_op_arrays."""
from __future__ import annotations

import json
import os

import numpy as np

import ops_bincode_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
TYPE_NAMES = ("orswot", "mvreg", "map_mvreg", "map_orswot", "map_map")
WIDTH_SETS = ((1, 1, 1, 1), (8, 8, 8, 8), (1, 2, 4, 8), (8, 4, 2, 1))
FIELDS = ("kind", "key", "actor", "counter", "key2", "actor2", "counter2", "val")
USED = {
    ref.ORSWOT: ("kind", "actor", "counter", "key2"),
    ref.MVREG: ("val",),
    ref.MAP_MVREG: ("kind", "key", "actor", "counter", "val"),
    ref.MAP_ORSWOT: ("kind", "key", "actor", "counter", "key2"),
    ref.MAP_MAP: FIELDS,
}
U32 = ("kind", "actor", "actor2", "clk_act")


def golden():
    with open(os.path.join(REPO, "tests", "golden", "bincode_ops.json")) as f:
        return json.load(f)["ops"]


# ------------------------------------------------------------ op literals
def nested_up(dot, key, inner):
    return {"up": {"dot": list(dot), "key": key, "op": inner}}


def nested_put(pairs, val):
    return {"put": {"clock": [list(p) for p in pairs], "val": val}}


def make_op(op_type, kind, dot, key, key2, dot2, val, pairs):
    """The op literal of a kind of the crdt_*_ops struct from its fields."""
    pairs = [tuple(p) for p in pairs]
    if op_type == ref.ORSWOT:
        return ("add", dot[0], dot[1], key2) if kind == 0 else ("rm", key2, pairs)
    if op_type == ref.MVREG:
        return (pairs, val)
    if op_type == ref.MAP_MAP:
        if kind == 0:
            return "nop"
        if kind == 1:
            return {"rm": {"clock": [list(p) for p in pairs], "key": key}}
        inner = "nop" if kind == 4 else {"rm": {"clock": [list(p) for p in pairs], "key": key2}} if kind == 3 else \
            nested_up(dot2, key2, nested_put(pairs, val))
        return nested_up(dot, key, inner)
    if kind == 0:
        return ("nop",)
    if kind == 1:
        return ("rm", key, pairs)
    if op_type == ref.MAP_MVREG:
        return ("up", dot[0], dot[1], key, pairs, val)
    return ("up_add", dot[0], dot[1], key, key2) if kind == 2 else ("up_rm", dot[0], dot[1], key, key2, pairs)


N_KINDS = {ref.ORSWOT: 2, ref.MVREG: 1, ref.MAP_MVREG: 3, ref.MAP_ORSWOT: 4, ref.MAP_MAP: 5}
CLOCKED = {ref.ORSWOT: (1,), ref.MVREG: (0,), ref.MAP_MVREG: (1, 2), ref.MAP_ORSWOT: (1, 3), ref.MAP_MAP: (1, 2, 3)}


def _value(rng, w):
    top = (1 << (8 * w)) - 1
    return rng.choice([0, 1, top, top, rng.randrange(top + 1)])


def random_clock(rng, n, wa):
    """n pairs, actors ascending below min(2^(8 wa), 2^32), the largest included now and then."""
    top = min(1 << (8 * wa), 1 << 32)
    n = min(n, top)
    if n > top // 2:
        acts = sorted(rng.sample(range(top), n))
    else:
        acts = set()
        if n and rng.random() < 0.3:
            acts.add(top - 1)
        while len(acts) < n:
            acts.add(rng.randrange(top))
        acts = sorted(acts)
    return [(a, rng.choice([1, U64, rng.randrange(1, 1 << 40)])) for a in acts]


def random_op(rng, op_type, widths, kind=None, n_pairs=None):
    """One op whose every field is drawn up to the largest value its width holds."""
    wa, wk, w2, wv = widths
    kind = rng.randrange(N_KINDS[op_type]) if kind is None else kind
    atop = min(1 << (8 * wa), 1 << 32) - 1
    dot = (rng.choice([0, atop, rng.randrange(atop + 1)]), rng.choice([0, 1, U64, rng.randrange(1 << 50)]))
    dot2 = (rng.choice([0, atop, rng.randrange(atop + 1)]), rng.choice([0, 1, U64, rng.randrange(1 << 50)]))
    n = 0
    if kind in CLOCKED[op_type]:
        n = rng.choice([0, 1, 2, 3, 5]) if n_pairs is None else n_pairs
    return make_op(op_type, kind, dot, _value(rng, wk or 1), _value(rng, w2 or 1), dot2, _value(rng, wv or 1),
                   random_clock(rng, n, wa))


def random_ops(rng, op_type, widths, n):
    return [random_op(rng, op_type, widths) for _ in range(n)]


# ------------------------------------------------------------ host packing
def fields_of(op_type, op):
    """kind, key, actor, counter, key2, actor2, counter2, val of one op: fields
    its kind does not carry are 0, as the arrays_from_lists packers write them."""
    f = dict.fromkeys(FIELDS, 0)
    f["kind"] = ref.kind_of(op_type, op) or 0
    if op_type == ref.ORSWOT:
        if op[0] == "add":
            f["actor"], f["counter"], f["key2"] = op[1], op[2], op[3]
        else:
            f["key2"] = op[1]
    elif op_type == ref.MVREG:
        f["val"] = op[1]
    elif op_type == ref.MAP_MAP:
        if op != "nop" and "rm" in op:
            f["key"] = op["rm"]["key"]
        elif op != "nop":
            up = op["up"]
            (f["actor"], f["counter"]), f["key"], inner = up["dot"], up["key"], up["op"]
            if inner != "nop" and "rm" in inner:
                f["key2"] = inner["rm"]["key"]
            elif inner != "nop":
                iu = inner["up"]
                (f["actor2"], f["counter2"]), f["key2"], f["val"] = iu["dot"], iu["key"], iu["op"]["put"]["val"]
    elif op[0] == "rm":
        f["key"] = op[1]
    elif op[0] != "nop":
        f["actor"], f["counter"], f["key"] = op[1], op[2], op[3]
        if op_type == ref.MAP_MVREG:
            f["val"] = op[5]
        else:
            f["key2"] = op[4]
    return f


def arrays_of(op_type, ops):
    """A flat op list -> {field: numpy array} over the fields the type uses,
    clk_end, clk_act and clk_ctr (u32 / u64 as in crdt_op_arrays)."""
    cols = {f: [] for f in USED[op_type]}
    end, act, ctr = [], [], []
    for op in ops:
        f = fields_of(op_type, op)
        for k in cols:
            cols[k].append(f[k])
        for a, c in ref.pairs_of(op_type, op):
            act.append(a)
            ctr.append(c)
        end.append(len(act))
    out = {k: np.asarray(v, np.uint32 if k in U32 else np.uint64) for k, v in cols.items()}
    out["clk_end"] = np.asarray(end, np.uint64)
    out["clk_act"] = np.asarray(act, np.uint32)
    out["clk_ctr"] = np.asarray(ctr, np.uint64)
    return out


# -------------------------------------------------------- malformed blobs
def good_ops(op_type):
    """Two good neighbours of every bad blob: one with a clock, one (where the
    type has such a kind) without."""
    return {
        ref.ORSWOT: [("rm", 9, [(1, 2), (3, 4)]), ("add", 5, 6, 7)],
        ref.MVREG: [([(1, 2), (3, 4)], 9), ([(0, 7)], 8)],
        ref.MAP_MVREG: [("up", 5, 6, 7, [(1, 2), (3, 4)], 9), ("rm", 3, [(0, 7)])],
        ref.MAP_ORSWOT: [("up_rm", 5, 6, 7, 8, [(1, 2), (3, 4)]), ("up_add", 1, 2, 3, 4)],
        ref.MAP_MAP: [nested_up((5, 6), 7, nested_up((1, 2), 8, nested_put([(1, 2), (3, 4)], 9))),
                      nested_up((1, 2), 3, "nop")],
    }[op_type]


def _q(v):
    return int(v).to_bytes(8, "little")


def malformed(op_type, widths):
    """name -> blob: one (or a few) per CRDT_ENONCANON class of the ingest that
    a blob alone can show. Built by splicing raw bytes into a good op whose
    clock comes last but for its tail field."""
    wa, wk, w2, wv = widths
    a = lambda v: int(v).to_bytes(wa, "little")  # noqa: E731
    pair = lambda x, c: a(x) + _q(c)  # noqa: E731
    deep = good_ops(op_type)[0]  # the kind with the most fields, clock [(1, 2), (3, 4)]
    good = ref.encode(op_type, deep, widths)
    tail = {ref.ORSWOT: w2, ref.MVREG: wv, ref.MAP_MVREG: wv, ref.MAP_ORSWOT: w2, ref.MAP_MAP: wv}[op_type]
    at = len(good) - tail - 2 * (wa + 8) - 8  # the clock's length word

    def clock(raw):
        return good[:at] + raw + good[len(good) - tail:]

    two = pair(1, 2) + pair(3, 4)
    last0 = {ref.ORSWOT: 1, ref.MVREG: 0}.get(op_type, 2)
    out = {
        "ends early": good[:-1],
        "ends inside the clock": clock(_q(2) + two[:-3])[:-tail],
        "trailing byte": good + b"\x00",
        "shorter than its variant word": good[:3],
        "empty blob": b"",
        "variant above the last": (last0 + 1).to_bytes(4, "little") + good[4:],
        "variant with a high byte": good[:3] + b"\x01" + good[4:],
        "length word 2^61": clock(_q(1 << 61) + two),
        "length word 2^64-1": clock(_q(U64) + two),
        "length word too large by one": clock(_q(3) + two),
        "length word too small by one": clock(_q(1) + two),
        "descending actors": clock(_q(2) + pair(3, 4) + pair(1, 2)),
        "duplicate actor": clock(_q(2) + pair(3, 1) + pair(3, 2)),
        "zero counter": clock(_q(2) + pair(1, 2) + pair(3, 0)),
        "zero counter first": clock(_q(2) + pair(1, 0) + pair(3, 4)),
    }
    if wa == 8:
        out["clock actor 2^32"] = clock(_q(2) + pair(1, 2) + pair(1 << 32, 4))
    if op_type >= ref.MAP_MVREG:
        v1 = 4 + wa + 8 + wk  # the nested op's variant word
        last1 = {ref.MAP_MVREG: 0, ref.MAP_ORSWOT: 1, ref.MAP_MAP: 2}[op_type]
        out["inner variant above the last"] = good[:v1] + (last1 + 1).to_bytes(4, "little") + good[v1 + 4:]
        out["inner variant with a high byte"] = good[:v1 + 2] + b"\x01" + good[v1 + 3:]
        out["ends inside the inner variant word"] = good[:v1 + 2]
        if wa == 8:
            out["dot actor 2^32"] = good[:4] + pair(1 << 32, 6) + good[4 + wa + 8:]
    if op_type == ref.ORSWOT and wa == 8:
        add = ref.encode(op_type, ("add", 5, 6, 7), widths)
        out["dot actor 2^32"] = add[:4] + pair(1 << 32, 6) + add[4 + wa + 8:]
    if op_type == ref.MAP_ORSWOT:
        add = ref.encode(op_type, ("up_add", 1, 2, 3, 4), widths)
        d2 = 4 + wa + 8 + wk + 4  # the nested Add's dot
        out["dot mismatch: actor"] = add[:d2] + pair(2, 2) + add[d2 + wa + 8:]
        out["dot mismatch: counter"] = add[:d2] + pair(1, 3) + add[d2 + wa + 8:]
    if op_type == ref.MAP_MAP:
        put = 4 + wa + 8 + wk + 4 + wa + 8 + w2  # the innermost Put's variant word
        out["put variant above the last"] = good[:put] + (1).to_bytes(4, "little") + good[put + 4:]
        if wa == 8:
            d2 = 4 + wa + 8 + wk + 4
            out["inner dot actor 2^32"] = good[:d2] + pair(1 << 32, 2) + good[d2 + wa + 8:]
    return out
