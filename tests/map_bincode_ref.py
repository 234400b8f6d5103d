"""CPU restatement of the reference's binary form of an MVReg<V, A> and of a
Map<K, MVReg<V, A>, A> — TEST INFRASTRUCTURE ONLY, after oracle/bincode_ref.py
(the Orswot form). The product codec is the HIP one behind
crdt_mvreg_{from,to}_bincode / crdt_map_mvreg_{from,to}_bincode.

The reference serialises with `to_binary` / `from_binary` (src/lib.rs:62-83):
bincode 0.9 of the serde derives on

    VClock<A>       { dots: BTreeMap<A, u64> }                 (src/vclock.rs:54-57)
    MVReg<V, A>     { vals: Vec<(VClock<A>, V)> }              (src/mvreg.rs:42-46)
    Entry<V, A>     { clock: VClock<A>, val: V }               (src/map.rs:69-77)
    Map<K, V, A>    { clock: VClock<A>,                        (src/map.rs:81-99)
                      entries: BTreeMap<K, Entry<V, A>>,
                      deferred: HashMap<VClock<A>, BTreeSet<K>> }

The published data format, restated: a struct is its fields in declaration
order with no framing; a Vec, map or set is its length as u64 followed by its
elements in iteration order (BTreeMap / BTreeSet: ascending; HashMap:
arbitrary; Vec: as stored, and an MVReg's Vec order is state); a tuple is its
fields; integers are fixed-width little-endian.

    VClock   u64 n | n x (A actor | u64 counter)
    MVReg    u64 n_vals | n_vals x (VClock | V val)
    Map      VClock | u64 n_entries | n_entries x (K key | VClock | MVReg)
                    | u64 n_def | n_def x (VClock | u64 n | n x K)

A, K and V are unsigned integers of a fixed byte width. As with the Orswot
form, no Rust toolchain exists in the build image, so exact bytes are pinned
to this restatement of the published format and not to reference output;
the restatement itself is pinned by the hand-derived blobs of
tests/golden/bincode_map_mvreg.json, and the round-trip property (all the
reference's own tests assert, src/lib.rs:53-60) is tested on every state the
KATs and the generators reach.

States are oracle/crdts_ref.py's MVReg and Map (of MVReg values). The only
unordered container is the map's deferred HashMap: `rng` shuffles its order,
without it the clocks go in CLOCK ORDER (the order the GPU egest writes).
decode_* raises FormatError for a blob the slabs cannot hold: a zero counter,
keys (actors, map keys, deferred-set keys) not strictly ascending, two equal
deferred clocks, truncated or trailing bytes, a length word larger than the
bytes left could hold.
"""
from __future__ import annotations

import struct

from map_slab import crdts_ref

_FMT = {1: "<B", 2: "<H", 4: "<I", 8: "<Q"}


class FormatError(ValueError):
    pass


# ------------------------------------------------------------------ encode
def _clock(out, c, wa):
    pairs = sorted(c.dots.items())  # BTreeMap order
    out += struct.pack("<Q", len(pairs))
    for a, n in pairs:
        out += struct.pack(_FMT[wa], a)
        out += struct.pack("<Q", n)


def _mvreg(out, r, wa, wv):
    out += struct.pack("<Q", len(r.vals))
    for c, v in r.vals:  # Vec order
        _clock(out, c, wa)
        out += struct.pack(_FMT[wv], v)


def encode_mvreg(reg, actor_bytes, val_bytes, rng=None):
    """crdts_ref.MVReg -> bytes (rng: unused, an MVReg holds no unordered container)."""
    out = bytearray()
    _mvreg(out, reg, actor_bytes, val_bytes)
    return bytes(out)


def encode_map_mvreg(m, actor_bytes, key_bytes, val_bytes, rng=None):
    """crdts_ref.Map of MVReg values -> bytes; the deferred HashMap in CLOCK
    ORDER, or shuffled by rng (a random.Random)."""
    out = bytearray()
    _clock(out, m.clock, actor_bytes)
    out += struct.pack("<Q", len(m.entries))
    for key in sorted(m.entries):  # BTreeMap order
        ec, r = m.entries[key]
        out += struct.pack(_FMT[key_bytes], key)
        _clock(out, ec, actor_bytes)
        _mvreg(out, r, actor_bytes, val_bytes)
    defs = crdts_ref.clock_order(list(m.deferred))
    if rng is not None:
        rng.shuffle(defs)
    out += struct.pack("<Q", len(defs))
    for c in defs:
        _clock(out, c, actor_bytes)
        ks = sorted(m.deferred[c])  # BTreeSet order
        out += struct.pack("<Q", len(ks))
        for k in ks:
            out += struct.pack(_FMT[key_bytes], k)
    return bytes(out)


# ------------------------------------------------------------------ decode
class _Reader:
    def __init__(self, blob):
        self.b, self.pos = bytes(blob), 0

    def take(self, w):
        if self.pos + w > len(self.b):
            raise FormatError("truncated")
        v = struct.unpack_from(_FMT[w], self.b, self.pos)[0]
        self.pos += w
        return v

    def length(self, unit):
        """A length word whose elements take at least `unit` bytes each."""
        n = self.take(8)
        if n * unit > len(self.b) - self.pos:
            raise FormatError("length word larger than the bytes left")
        return n

    def clock(self, wa):
        pairs, last = [], None
        for _ in range(self.length(wa + 8)):
            a, c = self.take(wa), self.take(8)
            if last is not None and a <= last:
                raise FormatError("actors not strictly ascending")
            if c == 0:
                raise FormatError("zero counter")
            last = a
            pairs.append((a, c))
        return crdts_ref.VClock(pairs)

    def mvreg(self, wa, wv):
        r = crdts_ref.MVReg()
        for _ in range(self.length(8 + wv)):
            c = self.clock(wa)
            r.vals.append((c, self.take(wv)))
        return r

    def end(self):
        if self.pos != len(self.b):
            raise FormatError("trailing bytes")


def decode_mvreg(blob, actor_bytes, val_bytes):
    rd = _Reader(blob)
    r = rd.mvreg(actor_bytes, val_bytes)
    rd.end()
    return r


def decode_map_mvreg(blob, actor_bytes, key_bytes, val_bytes):
    rd = _Reader(blob)
    m = crdts_ref.Map(crdts_ref.MVReg)
    m.clock = rd.clock(actor_bytes)
    last = None
    for _ in range(rd.length(key_bytes + 16)):
        key = rd.take(key_bytes)
        if last is not None and key <= last:
            raise FormatError("keys not strictly ascending")
        last = key
        ec = rd.clock(actor_bytes)
        m.entries[key] = [ec, rd.mvreg(actor_bytes, val_bytes)]
    for _ in range(rd.length(16)):
        c = rd.clock(actor_bytes)
        if c in m.deferred:
            raise FormatError("duplicate deferred clock")
        ks, last = [], None
        for _ in range(rd.length(key_bytes)):
            k = rd.take(key_bytes)
            if last is not None and k <= last:
                raise FormatError("deferred-set keys not strictly ascending")
            last = k
            ks.append(k)
        m.deferred[c] = set(ks)
    rd.end()
    return m


def mvreg_equal(a, b):
    """Vec order is state: the same (clock, value) list."""
    return [(c.canonical(), v) for c, v in a.vals] == [(c.canonical(), v) for c, v in b.vals]


def map_equal(a, b):
    """Map equality with every register compared in Vec order."""
    if a.clock != b.clock or sorted(a.entries) != sorted(b.entries):
        return False
    for k in a.entries:
        if a.entries[k][0] != b.entries[k][0] or not mvreg_equal(a.entries[k][1], b.entries[k][1]):
            return False
    da = {c.canonical(): sorted(s) for c, s in a.deferred.items()}
    db = {c.canonical(): sorted(s) for c, s in b.deferred.items()}
    return da == db
