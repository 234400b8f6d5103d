"""CPU restatement of the reference's binary form of the Orswot, MVReg and Map
ops — TEST INFRASTRUCTURE ONLY. The product codec is the HIP one behind
crdt_ops_* (rust-crdt_amd/csrc/ops_bincode.hip).

The `Op` enums all derive Serialize / Deserialize:

    orswot::Op<M, A>   Add { dot: Dot<A>, member: M } | Rm { clock: VClock<A>, member: M }
                                                              (src/orswot.rs:36-53)
    mvreg::Op<V, A>    Put { clock: VClock<A>, val: V }       (src/mvreg.rs:49-59)
    map::Op<K, V, A>   Nop | Rm { clock: VClock<A>, key: K }
                       | Up { dot: Dot<A>, key: K, op: V::Op } (src/map.rs:102-123)

bincode 0.9, restated: an enum is its variant index as a little-endian u32
followed by the variant's fields in declaration order; a struct is its fields
with no framing; a map is its length as u64 then its entries in iteration order
(BTreeMap: ascending keys); integers are fixed-width little-endian.

    VClock     u64 n | n x (A actor | u64 counter)
    Dot        A actor | u64 counter

No Rust toolchain exists in the build image, so exact bytes are pinned to this
restatement and not to reference output; the restatement itself is pinned by
the hand-derived blobs of tests/golden/bincode_ops.json.

Widths are (actor_bytes, key_bytes, key2_bytes, val_bytes), each 1, 2, 4 or 8
where the op type has the field. Ops are written as the existing packers take
them (crdts_hip.*Ops.arrays_from_lists / from_lists):

    orswot      ("add", actor, counter, member) | ("rm", member, pairs)
    mvreg       (pairs, val)
    map_mvreg   ("up", actor, counter, key, pairs, val) | ("rm", key, pairs) | ("nop",)
    map_orswot  ("up_add", actor, counter, key, member) | ("up_rm", actor, counter, key, member, pairs)
                | ("rm", key, pairs) | ("nop",)
    map_map     "nop" | {"rm": {"clock": pairs, "key": k}} | {"up": {"dot": [a, c], "key": k, "op": INNER}},
                INNER = "nop" | {"rm": {"clock": pairs, "key": k2}}
                      | {"up": {"dot": [a2, c2], "key": k2, "op": {"put": {"clock": pairs, "val": v}}}}

with pairs = [(actor, counter), ...]. decode raises FormatError for what the
kernels latch CRDT_ENONCANON for: a blob that ends early, has trailing bytes or
is shorter than its variant word; a variant index above the type's last; a
length word larger than the bytes left can hold; clock actors not strictly
ascending; a zero counter in a clock; an actor >= 2^32 in a clock or a dot; a
Map<Orswot> Up whose nested Add carries another dot than the Up.
"""
from __future__ import annotations

from clock_bincode_ref import pack  # noqa: F401  (blobs -> one buffer with offsets and lengths)

ORSWOT, MVREG, MAP_MVREG, MAP_ORSWOT, MAP_MAP = range(5)
TYPES = {"orswot": ORSWOT, "mvreg": MVREG, "map_mvreg": MAP_MVREG, "map_orswot": MAP_ORSWOT, "map_map": MAP_MAP}
KIND_BAD = 0xFFFFFFFF
ACTOR_LIMIT = 1 << 32


class FormatError(ValueError):
    pass


# ------------------------------------------------------------------ encode
def _le(v, w, what):
    if not 0 <= v < 1 << (8 * w):
        raise FormatError(f"{what} {v} does not fit {w} bytes")
    return int(v).to_bytes(w, "little")


def _variant(v):
    return int(v).to_bytes(4, "little")


def _dot(a, c, wa):
    if a >= ACTOR_LIMIT:
        raise FormatError(f"actor {a} >= 2^32")
    return _le(a, wa, "actor") + _le(c, 8, "counter")


def _clock(pairs, wa):
    out, prev = bytearray(_le(len(pairs), 8, "length")), -1
    for a, c in pairs:
        if a <= prev:
            raise FormatError("clock actors not strictly ascending")
        if c == 0:
            raise FormatError("a VClock never stores a zero counter")
        out += _dot(a, c, wa)
        prev = a
    return bytes(out)


def encode(op_type, op, widths):
    wa, wk, w2, wv = widths
    if op_type == ORSWOT:
        if op[0] == "add":
            _, a, c, m = op
            return _variant(0) + _dot(a, c, wa) + _le(m, w2, "member")
        _, m, pairs = op
        return _variant(1) + _clock(pairs, wa) + _le(m, w2, "member")
    if op_type == MVREG:
        pairs, v = op
        return _variant(0) + _clock(pairs, wa) + _le(v, wv, "val")
    if op_type == MAP_MAP:
        if op == "nop":
            return _variant(0)
        if "rm" in op:
            return _variant(1) + _clock(op["rm"]["clock"], wa) + _le(op["rm"]["key"], wk, "key")
        up = op["up"]
        head, inner = _variant(2) + _dot(*up["dot"], wa) + _le(up["key"], wk, "key"), up["op"]
        if inner == "nop":
            return head + _variant(0)
        if "rm" in inner:
            return head + _variant(1) + _clock(inner["rm"]["clock"], wa) + _le(inner["rm"]["key"], w2, "key2")
        iu = inner["up"]
        put = iu["op"]["put"]
        return (head + _variant(2) + _dot(*iu["dot"], wa) + _le(iu["key"], w2, "key2") + _variant(0) +
                _clock(put["clock"], wa) + _le(put["val"], wv, "val"))
    if op[0] == "nop":
        return _variant(0)
    if op[0] == "rm":
        return _variant(1) + _clock(op[2], wa) + _le(op[1], wk, "key")
    head = _variant(2) + _dot(op[1], op[2], wa) + _le(op[3], wk, "key")
    if op_type == MAP_MVREG:
        _, _, _, _, pairs, v = op
        return head + _variant(0) + _clock(pairs, wa) + _le(v, wv, "val")
    if op[0] == "up_add":  # the nested Add's dot is the Up's (Map::update)
        return head + _variant(0) + _dot(op[1], op[2], wa) + _le(op[4], w2, "member")
    return head + _variant(1) + _clock(op[5], wa) + _le(op[4], w2, "member")


# ------------------------------------------------------------------ decode
class _Reader:
    def __init__(self, blob):
        self.b, self.pos = bytes(blob), 0

    def left(self):
        return len(self.b) - self.pos

    def int(self, w, what):
        if self.left() < w:
            raise FormatError(f"blob ends inside {what}")
        v = int.from_bytes(self.b[self.pos:self.pos + w], "little")
        self.pos += w
        return v

    def variant(self, last, what):
        v = self.int(4, f"the variant word of {what}")  # all four bytes
        if v > last:
            raise FormatError(f"{what} has no variant {v}")
        return v

    def dot(self, wa):
        a, c = self.int(wa, "a dot"), self.int(8, "a dot")
        if a >= ACTOR_LIMIT:
            raise FormatError(f"dot actor {a} >= 2^32")
        return a, c

    def clock(self, wa):
        n = self.int(8, "a length word")
        if n > self.left() // (wa + 8):  # before multiplying: n * entry may not fit a u64
            raise FormatError(f"length word {n} exceeds the bytes left")
        pairs, prev = [], -1
        for _ in range(n):
            a, c = self.int(wa, "a clock"), self.int(8, "a clock")
            if c == 0:
                raise FormatError("zero counter")
            if a <= prev:
                raise FormatError("actors not strictly ascending")
            if a >= ACTOR_LIMIT:
                raise FormatError(f"clock actor {a} >= 2^32")
            prev = a
            pairs.append((a, c))
        return pairs

    def end(self):
        if self.left():
            raise FormatError("trailing bytes")


def decode(op_type, blob, widths):
    wa, wk, w2, wv = widths
    r = _Reader(blob)
    op = _decode(op_type, r, wa, wk, w2, wv)
    r.end()
    return op


def _decode(op_type, r, wa, wk, w2, wv):
    if op_type == ORSWOT:
        if r.variant(1, "orswot::Op") == 0:
            a, c = r.dot(wa)
            return ("add", a, c, r.int(w2, "the member"))
        pairs = r.clock(wa)
        return ("rm", r.int(w2, "the member"), pairs)
    if op_type == MVREG:
        r.variant(0, "mvreg::Op")
        pairs = r.clock(wa)
        return (pairs, r.int(wv, "the value"))
    v0 = r.variant(2, "map::Op")
    nested = op_type == MAP_MAP
    if v0 == 0:
        return "nop" if nested else ("nop",)
    if v0 == 1:
        pairs = r.clock(wa)
        key = r.int(wk, "the key")
        return {"rm": {"clock": pairs, "key": key}} if nested else ("rm", key, pairs)
    a, c = r.dot(wa)
    key = r.int(wk, "the key")
    if op_type == MAP_MVREG:
        r.variant(0, "mvreg::Op")
        pairs = r.clock(wa)
        return ("up", a, c, key, pairs, r.int(wv, "the value"))
    if op_type == MAP_ORSWOT:
        if r.variant(1, "orswot::Op") == 0:
            if r.dot(wa) != (a, c):
                raise FormatError("the nested Add's dot is not the Up's")
            return ("up_add", a, c, key, r.int(w2, "the member"))
        pairs = r.clock(wa)
        return ("up_rm", a, c, key, r.int(w2, "the member"), pairs)
    v1 = r.variant(2, "the inner map::Op")
    if v1 == 0:
        inner = "nop"
    elif v1 == 1:
        pairs = r.clock(wa)
        inner = {"rm": {"clock": pairs, "key": r.int(w2, "the inner key")}}
    else:
        a2, c2 = r.dot(wa)
        key2 = r.int(w2, "the inner key")
        r.variant(0, "mvreg::Op")
        pairs = r.clock(wa)
        inner = {"up": {"dot": [a2, c2], "key": key2, "op": {"put": {"clock": pairs, "val": r.int(wv, "the value")}}}}
    return {"up": {"dot": [a, c], "key": key, "op": inner}}


# ------------------------------------------------------- shape of an op
def kind_of(op_type, op):
    """The kind of the crdt_*_ops struct (None for mvreg: no kind array)."""
    if op_type == ORSWOT:
        return 0 if op[0] == "add" else 1
    if op_type == MVREG:
        return None
    if op_type == MAP_MAP:
        if op == "nop":
            return 0
        if "rm" in op:
            return 1
        inner = op["up"]["op"]
        return 4 if inner == "nop" else 3 if "rm" in inner else 2
    return {"nop": 0, "rm": 1, "up": 2, "up_add": 2, "up_rm": 3}[op[0]]


def pairs_of(op_type, op):
    """The op's clock pairs ([] where its kind carries no clock)."""
    if op_type == ORSWOT:
        return list(op[2]) if op[0] == "rm" else []
    if op_type == MVREG:
        return list(op[0])
    if op_type == MAP_MAP:
        if op == "nop":
            return []
        if "rm" in op:
            return list(op["rm"]["clock"])
        inner = op["up"]["op"]
        return [] if inner == "nop" else list(inner["rm"]["clock"]) if "rm" in inner else \
            list(inner["up"]["op"]["put"]["clock"])
    if op[0] in ("rm", "up_rm"):
        return list(op[-1])
    return list(op[4]) if op[0] == "up" else []


def op_bytes(op_type, kind, n_pairs, widths):
    """The size formulas: head + (8 + n (A + 8) where the kind has a clock) + tail."""
    wa, wk, w2, wv = widths
    dot, clock = wa + 8, 8 + n_pairs * (wa + 8)
    if op_type == ORSWOT:
        return 4 + (dot if kind == 0 else clock) + w2
    if op_type == MVREG:
        return 4 + clock + wv
    if kind == 0:
        return 4
    if kind == 1:
        return 4 + clock + wk
    up = 4 + dot + wk + 4
    if op_type == MAP_MVREG:
        return up + clock + wv
    if op_type == MAP_ORSWOT:
        return up + (dot if kind == 2 else clock) + w2
    return up + {2: dot + w2 + 4 + clock + wv, 3: clock + w2, 4: 0}[kind]


def canon(x):
    """An op literal with every sequence a list (JSON and tuples compare equal)."""
    if isinstance(x, dict):
        return {k: canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    return x
