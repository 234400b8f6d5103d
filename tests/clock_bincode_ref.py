"""CPU restatement of the reference's binary form of VClock, GCounter,
PNCounter and of their ops — TEST INFRASTRUCTURE ONLY. The product codec is
the HIP one behind crdt_clock_*_bincode* (rust-crdt_amd/csrc/clock_bincode.hip).

The reference serialises with `to_binary` / `from_binary` (src/lib.rs:62-83):
bincode 0.9 of the serde derives on

    VClock<A>     { dots: BTreeMap<A, u64> }          (src/vclock.rs:53-57)
    GCounter<A>   { inner: VClock<A> }                (src/gcounter.rs:26-28)
    PNCounter<A>  { p: GCounter<A>, n: GCounter<A> }  (src/pncounter.rs:33-36)
    Dot<A>        { actor: A, counter: u64 }          (src/vclock.rs:33-39)
    Op<A>         { dot: Dot<A>, dir: Dir }           (src/pncounter.rs:51-56)
    Dir           Pos | Neg                           (src/pncounter.rs:40-45)

The published data format, restated: a struct is its fields in declaration
order with no framing; a map is its length as u64 followed by its entries in
iteration order (BTreeMap: ascending keys); a unit enum variant is its index
as u32; integers are fixed-width little-endian.

    VClock     u64 n | n x (A actor | u64 counter)
    GCounter   the same bytes
    PNCounter  VClock p | VClock n
    Dot        A actor | u64 counter
    Op         Dot | u32 (Pos = 0, Neg = 1)

A is an unsigned integer of 1, 2, 4 or 8 bytes. No Rust toolchain exists in
the build image, so exact bytes are pinned to this restatement and not to
reference output; the restatement itself is pinned by the hand-derived blobs
of tests/golden/bincode_clocks.json.

A clock here is a dict {actor: counter} (or any iterable of pairs); a state is
a list of one clock (VClock, GCounter) or two (PNCounter: p, n). decode_*
raises FormatError for what the kernels latch CRDT_ENONCANON for: a zero
counter, actors not strictly ascending, an actor at or above `actor_limit`,
truncated or trailing bytes, a length word larger than the bytes left could
hold, a PNCounter whose p leaves no room for n, a Dir index above 1.
"""
from __future__ import annotations

import struct

_FMT = {1: "<B", 2: "<H", 4: "<I", 8: "<Q"}


class FormatError(ValueError):
    pass


def n_clocks(kind):
    return {"vclock": 1, "gcounter": 1, "pncounter": 2}[kind]


# ------------------------------------------------------------------ encode
def encode_clock(clock, actor_bytes):
    pairs = sorted(dict(clock).items())  # BTreeMap order
    out = bytearray(struct.pack("<Q", len(pairs)))
    for a, c in pairs:
        if c == 0:
            raise FormatError("a VClock never stores a zero counter (src/vclock.rs:159-163)")
        out += struct.pack(_FMT[actor_bytes], a) + struct.pack("<Q", c)
    return bytes(out)


def encode_state(clocks, actor_bytes):
    """clocks: [clock] (VClock / GCounter) or [p, n] (PNCounter)."""
    return b"".join(encode_clock(c, actor_bytes) for c in clocks)


def encode_op(actor, counter, actor_bytes, dir_=None):
    """Dot<A>, or PNCounter's Op when dir_ is 0 (Pos) or 1 (Neg)."""
    out = struct.pack(_FMT[actor_bytes], actor) + struct.pack("<Q", counter)
    if dir_ is not None:
        if dir_ not in (0, 1):
            raise FormatError(f"Dir has no variant {dir_}")
        out += struct.pack("<I", dir_)
    return out


def op_bytes(actor_bytes, with_dir):
    return actor_bytes + 8 + (4 if with_dir else 0)


# ------------------------------------------------------------------ decode
def _decode_clock(blob, pos, actor_bytes, actor_limit):
    entry = actor_bytes + 8
    if len(blob) - pos < 8:
        raise FormatError("blob ends inside a length word")
    (n,) = struct.unpack_from("<Q", blob, pos)
    pos += 8
    if n > (len(blob) - pos) // entry:  # before multiplying: n * entry may not fit a u64
        raise FormatError(f"length word {n} exceeds the bytes left")
    pairs, prev = [], -1
    for _ in range(n):
        (a,) = struct.unpack_from(_FMT[actor_bytes], blob, pos)
        (c,) = struct.unpack_from("<Q", blob, pos + actor_bytes)
        pos += entry
        if c == 0:
            raise FormatError("zero counter")
        if a <= prev:
            raise FormatError("actors not strictly ascending")
        if actor_limit is not None and a >= actor_limit:
            raise FormatError(f"actor {a} >= {actor_limit}")
        prev = a
        pairs.append((a, c))
    return pairs, pos


def decode_state(blob, actor_bytes, kind="vclock", actor_limit=None):
    """-> [pairs] or [p_pairs, n_pairs], each a sorted list of (actor, counter)."""
    blob = bytes(blob)
    pos, out = 0, []
    for _ in range(n_clocks(kind)):
        pairs, pos = _decode_clock(blob, pos, actor_bytes, actor_limit)
        out.append(pairs)
    if pos != len(blob):
        raise FormatError("trailing bytes")
    return out


def decode_op(blob, actor_bytes, with_dir=False, actor_limit=1 << 32):
    """-> (actor, counter, dir or None)."""
    blob = bytes(blob)
    if len(blob) != op_bytes(actor_bytes, with_dir):
        raise FormatError("an op blob has a fixed size")
    (a,) = struct.unpack_from(_FMT[actor_bytes], blob, 0)
    (c,) = struct.unpack_from("<Q", blob, actor_bytes)
    if actor_limit is not None and a >= actor_limit:
        raise FormatError(f"actor {a} >= {actor_limit}")
    d = None
    if with_dir:
        (d,) = struct.unpack_from("<I", blob, actor_bytes + 8)  # all four bytes
        if d > 1:
            raise FormatError(f"Dir has no variant {d}")
    return a, c, d


# ----------------------------------------------------------- dense rows
def state_row(clocks, n_actors):
    """The dense row of a state: n_actors slots per clock ([P|N] for two)."""
    row = [0] * (n_actors * len(clocks))
    for k, c in enumerate(clocks):
        for a, v in dict(c).items():
            row[k * n_actors + a] = v
    return row


def row_state(row, n_actors):
    """The clocks of a dense row (zero slots are absent actors)."""
    row = [int(v) for v in row]
    return [{a: v for a, v in enumerate(row[k:k + n_actors]) if v} for k in range(0, len(row), n_actors)]


def pack(blobs, lead=0, gap=0, fill=0xA5):
    """Concatenates blobs with `lead` bytes before the first and `gap` bytes
    (an int, or one per blob) after each but the last -> (buffer bytes,
    offsets, lengths)."""
    buf, off, ln = bytearray([fill] * lead), [], []
    for k, b in enumerate(blobs):
        off.append(len(buf))
        ln.append(len(b))
        buf += b
        if k + 1 < len(blobs):
            buf += bytes([fill] * (gap if isinstance(gap, int) else gap[k]))
    return bytes(buf), off, ln
