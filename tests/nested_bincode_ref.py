"""CPU restatement of the reference's binary form of a Map<K, Orswot<M, A>, A>
and of a Map<K, Map<K2, MVReg<V, A>, A>, A> (the reference's TestMap) — TEST
INFRASTRUCTURE ONLY, after tests/map_bincode_ref.py (MVReg and Map<K, MVReg>).
The product codec is the HIP one behind crdt_map_orswot_{from,to}_bincode /
crdt_map_map_{from,to}_bincode.

`to_binary` (src/lib.rs:62-83) is bincode 0.9 of the serde derives; on top of
the forms map_bincode_ref.py restates:

    Orswot<M, A>    { clock: VClock<A>,                         (src/orswot.rs:26-30)
                      entries: HashMap<M, VClock<A>>,
                      deferred: HashMap<VClock<A>, HashSet<M>> }

    Orswot   VClock | u64 n_mem | n_mem x (M member | VClock)
                    | u64 n_def | n_def x (VClock | u64 n | n x M)
    Map<K,V> VClock | u64 n_entries | n_entries x (K key | VClock | V)
                    | u64 n_def | n_def x (VClock | u64 n | n x K)
    V = Orswot<M, A>                (encode_map_orswot / decode_map_orswot)
    V = Map<K2, MVReg<V2, A>, A>    (encode_map_map / decode_map_map)

A HashMap / HashSet goes out in arbitrary order: the map's deferred clocks,
a nested set's members, its deferred clocks and their member sets; the nested
map's outer and inner deferred clocks. `rng` (a random.Random) shuffles every
one of them; without it they go in the order the GPU egest writes: clocks in
CLOCK ORDER, members ascending. BTreeMap / BTreeSet (map keys, deferred key
sets) go ascending, a Vec (an MVReg's values) as stored.

States are oracle/crdts_ref.py's Map, Orswot and MVReg. decode_* raises
FormatError for what the slabs cannot hold: a zero counter, a BTree sequence
not strictly ascending, two equal members in one nested set or in one
deferred member set, two equal deferred clocks in one container, truncated or
trailing bytes, a length word larger than the bytes left could hold. As in
map_bincode_ref.py no Rust toolchain exists in the build image: exact bytes
are pinned to this restatement, itself pinned by the hand-derived blobs of
tests/golden/bincode_map_orswot.json and tests/golden/bincode_map_map.json.
"""
from __future__ import annotations

import struct

import map_bincode_ref as MB
from map_bincode_ref import FormatError, _FMT, _clock  # noqa: F401
from map_slab import crdts_ref


def _order(clocks, rng):
    out = crdts_ref.clock_order(list(clocks))
    if rng is not None:
        rng.shuffle(out)
    return out


def _members(xs, rng):
    out = sorted(xs)
    if rng is not None:
        rng.shuffle(out)
    return out


# ------------------------------------------------------------------ encode
def _deferred(out, deferred, wa, we, rng, hashset):
    """deferred: {VClock: set}; hashset: the sets are HashSets (shuffled by rng), else BTreeSets."""
    defs = _order(deferred, rng)
    out += struct.pack("<Q", len(defs))
    for c in defs:
        _clock(out, c, wa)
        xs = _members(deferred[c], rng if hashset else None)
        out += struct.pack("<Q", len(xs))
        for x in xs:
            out += struct.pack(_FMT[we], x)


def _orswot(out, o, wa, wm, rng):
    _clock(out, o.clock, wa)
    mem = _members(o.entries, rng)
    out += struct.pack("<Q", len(mem))
    for x in mem:
        out += struct.pack(_FMT[wm], x)
        _clock(out, o.entries[x], wa)
    _deferred(out, o.deferred, wa, wm, rng, True)


def _map(out, m, wa, wk, value, rng):
    _clock(out, m.clock, wa)
    out += struct.pack("<Q", len(m.entries))
    for key in sorted(m.entries):  # BTreeMap order
        ec, v = m.entries[key]
        out += struct.pack(_FMT[wk], key)
        _clock(out, ec, wa)
        value(out, v)
    _deferred(out, m.deferred, wa, wk, rng, False)


def encode_map_orswot(m, actor_bytes, key_bytes, member_bytes, rng=None):
    """crdts_ref.Map of Orswot values -> bytes."""
    out = bytearray()
    _map(out, m, actor_bytes, key_bytes, lambda o, v: _orswot(o, v, actor_bytes, member_bytes, rng), rng)
    return bytes(out)


def encode_map_map(m, actor_bytes, key_bytes, inner_key_bytes, val_bytes, rng=None):
    """crdts_ref.Map of Map<_, MVReg> values -> bytes."""
    out = bytearray()

    def inner(o, v):
        _map(o, v, actor_bytes, inner_key_bytes, lambda o2, r: MB._mvreg(o2, r, actor_bytes, val_bytes), rng)

    _map(out, m, actor_bytes, key_bytes, inner, rng)
    return bytes(out)


# ------------------------------------------------------------------ decode
class _Reader(MB._Reader):
    def deferred(self, wa, we, hashset):
        out = {}
        for _ in range(self.length(16)):
            c = self.clock(wa)
            if c in out:
                raise FormatError("duplicate deferred clock")
            xs, last = [], None
            for _ in range(self.length(we)):
                x = self.take(we)
                if hashset:
                    if x in xs:
                        raise FormatError("duplicate deferred-set member")
                elif last is not None and x <= last:
                    raise FormatError("deferred-set keys not strictly ascending")
                last = x
                xs.append(x)
            out[c] = set(xs)
        return out

    def orswot(self, wa, wm):
        o = crdts_ref.Orswot()
        o.clock = self.clock(wa)
        for _ in range(self.length(wm + 8)):
            x = self.take(wm)
            if x in o.entries:
                raise FormatError("duplicate member")
            o.entries[x] = self.clock(wa)
        o.deferred = self.deferred(wa, wm, True)
        return o

    def map(self, m, wa, wk, unit, value):
        """unit: the least bytes of a value."""
        m.clock = self.clock(wa)
        last = None
        for _ in range(self.length(wk + 8 + unit)):
            key = self.take(wk)
            if last is not None and key <= last:
                raise FormatError("keys not strictly ascending")
            last = key
            ec = self.clock(wa)
            m.entries[key] = [ec, value()]
        m.deferred = self.deferred(wa, wk, False)
        return m


def decode_map_orswot(blob, actor_bytes, key_bytes, member_bytes):
    rd = _Reader(blob)
    m = rd.map(crdts_ref.Map(crdts_ref.Orswot, crdts_ref.clock_order), actor_bytes, key_bytes, 24,
               lambda: rd.orswot(actor_bytes, member_bytes))
    rd.end()
    return m


def _new_inner():
    return crdts_ref.Map(crdts_ref.MVReg)


def decode_map_map(blob, actor_bytes, key_bytes, inner_key_bytes, val_bytes):
    rd = _Reader(blob)

    def inner():
        return rd.map(_new_inner(), actor_bytes, inner_key_bytes, 8, lambda: rd.mvreg(actor_bytes, val_bytes))

    m = rd.map(crdts_ref.Map(_new_inner), actor_bytes, key_bytes, 24, inner)
    rd.end()
    return m


# ------------------------------------------------------------------ equality
def _defs(d):
    return {c.canonical(): sorted(s) for c, s in d.items()}


def orswot_equal(a, b):
    return (a.clock == b.clock and {x: c.canonical() for x, c in a.entries.items()} ==
            {x: c.canonical() for x, c in b.entries.items()} and _defs(a.deferred) == _defs(b.deferred))


def _map_equal(a, b, veq):
    if a.clock != b.clock or sorted(a.entries) != sorted(b.entries) or _defs(a.deferred) != _defs(b.deferred):
        return False
    return all(a.entries[k][0] == b.entries[k][0] and veq(a.entries[k][1], b.entries[k][1]) for k in a.entries)


def map_orswot_equal(a, b):
    return _map_equal(a, b, orswot_equal)


def map_map_equal(a, b):
    """Registers compared in Vec order (map_bincode_ref.map_equal)."""
    return _map_equal(a, b, MB.map_equal)
