"""The value of Map::get for Map<u64, Orswot> and the nested map (src/map.rs:
291-302; crdt_map_orswot_get*, crdt_map_map_get), restated in plain Python
straight on host slab arrays — test infrastructure, no tests here.

orswot_value_record(S, i, k, A) is the canonical record of the Orswot in key
slot k of object i, inner_map_row(S, i, k) the inner map there as a
crdts_ref.Map. Both are written from the layouts of include/crdts_hip.h alone:
neither uses tests/records.py or the readers of tests/map_slab.py
(tests/test_map_get_ref.py holds them against both). k None is an absent key:
Orswot::default() / Map::default().

KNOBS each turn the restatement into one plausible wrong kernel; the case
batches below are chosen so that every knob changes some answer.
"""
from __future__ import annotations

import random
import struct

import numpy as np

import crdts_ref
import map_kat_runner as mkr
import map_orswot_opgen
import map_slab
import nested_opgen

U64 = (1 << 64) - 1
EMPTY_MEMBER_CLOCK = 2
KNOBS = ("actor_major",        # dots emitted actor-major instead of member-major
         "dend_at_step",       # mem_dend off by one at a member that ends exactly on a 64-cell step
         "no_member_pad",      # the 8-byte pad after mem_dend dropped when n_dot + n_mem is odd
         "no_pad16",           # the record not padded to 16
         "no_empty_flag",      # the empty-member-clock flag forgotten
         "sets_by_vscap",      # deferred sets read by vscap instead of vdset_n
         "inner_out_stride")   # an inner row read with out's strides instead of inner's
PARITY_A = (1, 63, 64, 65, 128)
EDGE_A = (65, 128)


# ---------------------------------------------------------------- the restatement
def _u64s(xs):
    return struct.pack(f"<{len(xs)}Q", *xs)


def _u32s(xs):
    return struct.pack(f"<{len(xs)}I", *xs)


def orswot_value_record(S, i, k, A, knob=None):
    """The record of the value in key slot k of object i of the host
    MapOrswotSlab S (k None: Orswot::default()), as bytes."""
    a = S.a
    if k is None:
        clk, keys, rows, defs = [0] * A, [], [], []
    else:
        clk = [int(x) for x in a["vclock"][i, k, :A]]
        nm = int(a["vn_mem"][i, k])
        keys = [int(x) for x in a["vmem"][i, k, :nm]]
        rows = [[(act, int(c)) for act, c in enumerate(a["vmclock"][i, k, m, :A]) if c] for m in range(nm)]
        defs = []
        for d in range(int(a["vn_def"][i, k])):
            n = S.caps["vscap"] if knob == "sets_by_vscap" else int(a["vdset_n"][i, k, d])
            defs.append(([(act, int(c)) for act, c in enumerate(a["vdclock"][i, k, d, :A]) if c],
                         [int(x) for x in a["vdset"][i, k, d, :n]]))
    dots = [(m, act, c) for m, r in enumerate(rows) for act, c in r]
    if knob == "actor_major":
        dots.sort(key=lambda t: (t[1], t[0]))
    dend, e = [], 0
    for m, r in enumerate(rows):
        e += len(r)
        dend.append(e - 1 if knob == "dend_at_step" and ((m + 1) * A) % 64 == 0 and e else e)
    body = _u64s(clk) + _u64s(keys) + _u64s([c for _, _, c in dots]) + _u32s([act for _, act, _ in dots]) + _u32s(dend)
    if (len(dots) + len(keys)) % 2 and knob != "no_member_pad":
        body += bytes(4)
    ddots = [p for c, _ in defs for p in c]
    dkeys = [x for _, s in defs for x in s]
    de, me, dd, mm = [], [], 0, 0
    for c, s in defs:
        dd += len(c)
        mm += len(s)
        de.append(dd)
        me.append(mm)
    body += _u64s([c for _, c in ddots]) + _u64s(dkeys) + _u32s([act for act, _ in ddots]) + _u32s(de) + _u32s(me)
    size = 32 + len(body)
    if knob != "no_pad16":
        size = (size + 15) // 16 * 16
    flags = EMPTY_MEMBER_CLOCK if any(not r for r in rows) and knob != "no_empty_flag" else 0
    head = _u32s([size, A, len(keys), len(dots), len(defs), len(ddots), len(dkeys), flags])
    return (head + body).ljust(size, b"\0")


def inner_map_row(S, i, k, knob=None, out_caps=None):
    """The inner map in key slot k of object i of the host MapMapSlab S (inner
    object i * kcap + k), as a crdts_ref.Map of MVRegs; k None: Map::default().
    The inner arrays are read flat, by the strides of S.inner's capacities."""
    m = crdts_ref.Map(crdts_ref.MVReg)
    if k is None:
        return m
    I = S.inner
    kc, mc, dc, sc = out_caps if knob == "inner_out_stride" else (I.kcap, I.mcap, I.dcap, I.scap)
    A = I.a["clock"].shape[1]
    flat = {f: v.reshape(-1) for f, v in I.a.items()}

    def at(f, idx):
        return int(flat[f][idx % flat[f].size])

    def clock(f, row):
        return crdts_ref.VClock([(x, at(f, row * A + x)) for x in range(A) if at(f, row * A + x)])

    r = i * S.kcap + k
    m.clock = clock("clock", r)
    for s in range(min(at("n_keys", r), 1 << 13)):
        e = r * kc + s
        reg = crdts_ref.MVReg()
        reg.vals = [(clock("mv_clock", e * mc + v), at("mv_val", e * mc + v)) for v in range(min(at("mv_n", e), 256))]
        m.entries[at("keys", e)] = [clock("eclock", e), reg]
    for d in range(min(at("n_def", r), 128)):
        e = r * dc + d
        m.deferred[clock("dclock", e)] = {at("dset", e * sc + x) for x in range(min(at("dset_n", e), 8192))}
    return m


# ---------------------------------------------------------------- the shared cases
def seeded_maps(kind, A, n=40):
    """About n states of `kind` ("orswot" / "nested") from the op generators."""
    if kind == "nested" and A < 3:  # the generator needs three writers: its A = 65 states, every actor renamed to 0
        return [map_slab.relabel(m, {x: 0 for x in range(65)}) for m in seeded_maps(kind, 65, n)]
    out = []
    if kind == "nested":
        for start, ops in nested_opgen.gen_batch(5, n // 2, A, wide=A > 64):
            m = start.clone()
            for op in ops:
                mkr.apply_raw(m, op)
            out += [start.clone(), m]
        return out
    for pre, ops in map_orswot_opgen.gen_batch(7 + A, n, A):
        m = map_orswot_opgen.new_map()
        for op in pre + ops:
            map_orswot_opgen.apply_op(m, op)
        out.append(m)
    return out


def _orswot(clock, entries, deferred=()):
    o = crdts_ref.Orswot()
    o.clock = crdts_ref.VClock(clock)
    o.entries = {m: crdts_ref.VClock(c) for m, c in entries.items()}
    o.deferred = {crdts_ref.VClock(c): set(s) for c, s in deferred}
    return o


EDGE_CAPS = map_orswot_opgen.caps(8, 16, 3, 3, 1, 1)


def edge_maps(A):
    """Hand-made Map<u64, Orswot> states (mcap 16, vdcap 3, vscap 3): a value
    without members; mcap members holding all A dots each; n_dot + n_mem odd and
    even; record ends of 16 k and 16 k + 8 (and + 4, + 12) before the padding;
    vdcap deferred clocks with vscap-full sets; counters, members and keys of 0,
    1 and 2^64 - 1; a member whose clock row is all zero."""
    hi = A - 1
    m = map_orswot_opgen.new_map()
    m.clock = crdts_ref.VClock({0: U64, hi: 1})
    vals = {
        0: _orswot({0: 1, hi: U64}, {}),
        1: _orswot({x: U64 for x in range(A)},
                   {mem: {x: (U64 if (x + j) % 7 == 0 else x + j + 1) for x in range(A)}
                    for j, mem in enumerate(list(range(15)) + [U64])}),
        5: _orswot({0: 1}, {0: {0: 1}}),
        6: _orswot({0: 1, 1: U64, hi: 1}, {1: {0: 1}, U64: {1: U64, hi: 1}}),
        7: _orswot({0: 2}, {3: {0: 2}},
                   [({0: 5}, {0, 1, U64}), ({0: 5, hi: 1}, {2, 3, 4}), ({hi: U64}, {1, 5, U64})]),
        8: _orswot({0: 9, 64: 1}, {4: {}, 9: {64: 1}}, [({0: U64}, {0})]),
        9: _orswot({0: 1}, {0: {0: 1}}, [({0: 1, 1: 1}, {U64}), ({1: 5}, {0, 1})]),
        U64: _orswot({0: 3, 1: 3, hi: 3}, {0: {0: 1, 1: 2}, 1: {hi: 3}, U64: {0: 3, 1: 3, hi: 3}}),
    }
    for key, o in vals.items():
        m.entries[key] = [crdts_ref.VClock({0: 1 + key % 3}), o]
    one = map_orswot_opgen.new_map()
    one.entries[1] = [crdts_ref.VClock({hi: 1}), _orswot({hi: 2}, {1: {hi: 2}})]
    return [m, map_orswot_opgen.new_map(), one]


def _caps_of(kind, maps):
    """The smallest capacities that hold every map: the fullest row has n_keys == kcap."""
    mx = lambda xs: max([1] + list(xs))  # noqa: E731
    vals = [v for m in maps for _, v in m.entries.values()]
    kcap, dcap = mx(len(m.entries) for m in maps), mx(len(m.deferred) for m in maps)
    scap = mx(len(s) for m in maps for s in m.deferred.values())
    if kind == "nested":
        regs = [r for v in vals for _, r in v.entries.values()]
        inner = (mx(len(v.entries) for v in vals), mx(len(r.vals) for r in regs), mx(len(v.deferred) for v in vals),
                 mx(len(s) for v in vals for s in v.deferred.values()))
        return (kcap, dcap, scap), inner
    return map_orswot_opgen.caps(kcap, mx(len(v.entries) for v in vals), mx(len(v.deferred) for v in vals),
                                 mx(len(s) for v in vals for s in v.deferred.values()), dcap, scap)


def _queries(maps, rng):
    """Every present key once, and per map perhaps an absent key and an ALL;
    the first map with two keys gets 70 queries (more than a wave), the last
    seeded map none."""
    per_obj = []
    for m in maps:
        keys = sorted(m.entries)
        qs = [("key", k) for k in keys]
        absent = [k for k in (0, 4, U64) + tuple(x + 1 for x in keys[:2] if x < U64) if k not in m.entries]
        if rng.random() < 0.5 or not keys:
            qs.append(("key", rng.choice(absent)))
        if rng.random() < 0.3:
            qs.append(("all",))
        rng.shuffle(qs)
        per_obj.append(qs)
    wide = next(i for i, m in enumerate(maps) if len(m.entries) >= 2)
    keys = sorted(maps[wide].entries)
    per_obj[wide] = [("all",) if x % 23 == 22 else ("key", keys[x % len(keys)] + (1 if x % 9 == 8 else 0))
                     for x in range(70)]
    return per_obj


_CACHE = {}


def batch(kind, A):
    """dict(kind, A, maps, per_obj, caps): computed once, never modified.
    kind: "orswot" / "nested" (seeded, plus an empty map, a one-key map and an
    object nobody asks), "edges" (edge_maps)."""
    if (kind, A) in _CACHE:
        return _CACHE[kind, A]
    rng = random.Random(1000 * A + len(kind))
    if kind == "edges":
        maps = edge_maps(A)
        keys = sorted(maps[0].entries)
        per_obj = [[("key", k) for k in keys] + [("key", 2), ("key", 10), ("all",)], [("key", 0), ("all",)],
                   [("key", 1), ("key", U64)]]
        b = dict(kind="orswot", A=A, maps=maps, per_obj=per_obj, caps=EDGE_CAPS)
    else:
        maps = seeded_maps(kind, A)
        maps.append(type(maps[0])(maps[0].factory))  # n_keys 0
        one = next(m for m in maps if m.entries).clone()  # n_keys 1
        for k in sorted(one.entries)[1:]:
            del one.entries[k]
        maps.append(one)
        per_obj = _queries(maps, rng)
        per_obj[len(maps) - 3] = []
        b = dict(kind=kind, A=A, maps=maps, per_obj=per_obj, caps=_caps_of(kind, maps))
    _CACHE[kind, A] = b
    return b


def garbage(S):
    """Fills every array of a host slab with non-zero garbage: counts far past
    any capacity, keys and counters of all kinds."""
    for v in (S.a.values() if not hasattr(S, "inner") else list(S.a.values()) + list(S.inner.a.values())):
        v[...] = np.uint64(0xA5C3A5C3A5C3A5C3).astype(v.dtype) if v.dtype == np.uint64 else np.uint32(0xA5C3A5C3)
    return S


def pack(b, fill=True):
    """The batch's maps as a host slab at the batch's capacities; with `fill`
    every slot past a count holds garbage (the row writers of tests/map_slab.py
    touch only what the counts name)."""
    import crdts_hip

    n, A = len(b["maps"]), b["A"]
    if b["kind"] == "nested":
        outer, inner = b["caps"]
        S = crdts_hip.MapMapSlab.alloc(n, A, *outer, inner)
        put = map_slab.nested_map_to_row
    else:
        S = crdts_hip.MapOrswotSlab.alloc(n, A, **b["caps"])
        put = map_slab.orswot_map_to_row
    if fill:
        garbage(S)
    for i, m in enumerate(b["maps"]):
        put(m, S, i, A, zero=False)
    return S


def flat_queries(b):
    """[(object, query, slot or None)]: the slot of a KEY query's present key."""
    out = []
    for i, (m, qs) in enumerate(zip(b["maps"], b["per_obj"])):
        keys = sorted(m.entries)
        for q in qs:
            out.append((i, q, keys.index(q[1]) if q[0] == "key" and q[1] in m.entries else None))
    return out


def expected(b, S, knob=None, out_caps=None):
    """Per query (present, value): the record bytes or the inner crdts_ref.Map."""
    if b["kind"] == "nested":
        return [(int(k is not None), inner_map_row(S, i, k, knob, out_caps)) for i, _, k in flat_queries(b)]
    return [(int(k is not None), orswot_value_record(S, i, k, b["A"], knob)) for i, _, k in flat_queries(b)]
