"""Truncating clocks and states for the batched Map::truncate tests
(crdt_map_mvreg_truncate / crdt_map_orswot_truncate / crdt_map_map_truncate)
— test infrastructure (tests/test_map_truncate_ref.py,
tests/test_gpu_map_truncate.py, tools/map_truncate_bench.py). Needs no GPU.

States come from the existing op-stream generators (map_opgen,
map_orswot_opgen, nested_opgen), replayed on the restatement
(oracle/crdts_ref.py). Each object's truncating clock T is drawn from its own
map clock under a mode:
  below  every component <= the map clock's (60 % of the objects, drawn per
         object);
  mixed  components may exceed it (25 %);
  empty  the empty clock (7.5 %);
  all    every component 2^62 (7.5 %).
Within `below` and `mixed` each actor independently is 0, below its counter,
equal to it, or (mixed only) above it.

The expected state is crdts_ref.Map.truncate on a copy whose deferred dicts
are in CLOCK ORDER, outer and inner (`truncated`): where two deferred clocks
become equal the restatement keeps the set inserted last, and the slab's rule
is "the later one in CLOCK ORDER before the subtract"."""
from __future__ import annotations

import functools
import random

import numpy as np

import map_opgen
import map_orswot_opgen
import map_slab
import nested_opgen
from map_slab import crdts_ref

MODES = ("below", "mixed", "empty", "all")
ALL = 1 << 62


def draw_mode(rng):
    x = rng.random()
    return "below" if x < 0.6 else "mixed" if x < 0.85 else "empty" if x < 0.925 else "all"


def draw_clock(rng, clock, A, mode):
    """T for a map whose clock is `clock` (a crdts_ref.VClock), A actors."""
    if mode == "empty":
        return crdts_ref.VClock()
    if mode == "all":
        return crdts_ref.VClock([(a, ALL) for a in range(A)])
    dots = []
    for a in range(A):
        c = clock.get(a)
        pick = rng.randrange(4 if mode == "mixed" else 3)
        if pick == 1:
            t = rng.randrange(1, c) if c > 1 else 0  # below its counter
        elif pick == 2:
            t = c
        elif pick == 3:
            t = c + rng.randrange(1, 4)
        else:
            t = 0
        if t:
            dots.append((a, t))
    return crdts_ref.VClock(dots)


def draw(seed, states, A, modes=None):
    """-> (modes, clocks) for `states`; `modes`, if given, fixes every object's mode."""
    rng = random.Random(seed)
    ms = [modes[i % len(modes)] if modes else draw_mode(rng) for i in range(len(states))]
    return ms, [draw_clock(rng, m.clock, A, mode) for m, mode in zip(states, ms)]


def clock_rows(clocks, A):
    """Dense u64 [n][A] rows (0 = absent), the d_clock argument."""
    r = np.zeros((len(clocks), A), np.uint64)
    for i, c in enumerate(clocks):
        for a, n in c.dots.items():
            r[i, a] = n
    return r


def pairs(clock):
    return sorted(clock.dots.items())


def in_clock_order(m):
    """A clone of map `m` whose deferred dicts (its own, and its nested maps')
    are in CLOCK ORDER — the order a slab row holds them in."""
    r = m.clone()
    r.deferred = {c: r.deferred[c] for c in crdts_ref.clock_order(list(r.deferred))}
    for k, (c, v) in list(r.entries.items()):
        if isinstance(v, crdts_ref.Map):
            r.entries[k] = [c, in_clock_order(v)]
    return r


def truncated(m, T):
    r = in_clock_order(m)
    r.truncate(T)
    return r


# ------------------------------------------------------------------ states
@functools.lru_cache(maxsize=None)
def mvreg_batch(seed, n, A, n_ops=16):
    """((ops, state), ...): object i's whole op stream and the Map<u64, MVReg> it leaves."""
    out = []
    for pre, ops in map_opgen.gen_batch(seed, n, A, n_ops=n_ops):
        m = crdts_ref.Map(crdts_ref.MVReg)
        for op in pre + ops:
            map_opgen.apply_op(m, op)
        out.append((tuple(pre + ops), m))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def orswot_batch(seed, n, A, n_ops=16):
    out = []
    for pre, ops in map_orswot_opgen.gen_batch(seed, n, A, n_ops=n_ops):
        m = map_orswot_opgen.new_map()
        for op in pre + ops:
            map_orswot_opgen.apply_op(m, op)
        out.append((tuple(pre + ops), m))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nested_batch(seed, n, A, wide=False):
    """(state, ...): nested_opgen's start states after their op lists. (Its
    writers need three actors: below that, outer maps are put together from
    mvreg_batch's maps, with entry clocks, a map clock and deferred removes
    drawn over the actors there are.)"""
    if A < 3:
        rng = random.Random(seed)
        inner = [m for _, m in mvreg_batch(seed + 1, 3 * n, A)]
        out = []
        for i in range(n):
            m = crdts_ref.Map(lambda: crdts_ref.Map(crdts_ref.MVReg))
            for k, key in enumerate(rng.sample(map_opgen.KEYS, rng.randrange(0, 4))):
                m.entries[key] = [crdts_ref.VClock([(rng.randrange(A), rng.randrange(1, 9))]), inner[3 * i + k].clone()]
            m.clock = crdts_ref.VClock([(a, rng.randrange(4, 12)) for a in range(A)])
            for _ in range(rng.randrange(0, 3)):
                m.deferred[crdts_ref.VClock([(rng.randrange(A), rng.randrange(1, 20))])] = \
                    set(rng.sample(map_opgen.KEYS, rng.randrange(1, 3)))
            out.append(m)
        return tuple(out)
    return tuple(nested_opgen.replay(s, ops) for s, ops in nested_opgen.gen_batch(seed, n, A, wide))


def mvreg_caps(states):
    mx = lambda xs: max(max(xs, default=0), 1)  # noqa: E731
    return (mx(len(m.entries) for m in states), mx(len(r.vals) for m in states for _, r in m.entries.values()),
            mx(len(m.deferred) for m in states), mx(len(s) for m in states for s in m.deferred.values()))


def orswot_caps(states):
    mx = lambda xs: max(max(xs, default=0), 1)  # noqa: E731
    sets = [o for m in states for _, o in m.entries.values()]
    return dict(kcap=mx(len(m.entries) for m in states), mcap=mx(len(o.entries) for o in sets),
                vdcap=mx(len(o.deferred) for o in sets), vscap=mx(len(s) for o in sets for s in o.deferred.values()),
                dcap=mx(len(m.deferred) for m in states), scap=mx(len(s) for m in states for s in m.deferred.values()))


def nested_caps(states):
    """-> ((kcap, dcap, scap), (kcap, mcap, dcap, scap))"""
    z = [max(1, max(v)) for v in zip(*[nested_opgen.sizes(m) for m in states])]
    return tuple(z[:3]), tuple(z[3:])


def pack_mvreg(states, A, caps):
    import crdts_hip

    S = crdts_hip.MapSlab.alloc(len(states), A, *caps)
    for i, m in enumerate(states):
        map_slab.mvreg_map_to_row(m, S, i, A)
    return S


def pack_orswot(states, A, caps):
    import crdts_hip

    S = crdts_hip.MapOrswotSlab.alloc(len(states), A, **caps)
    for i, m in enumerate(states):
        map_slab.orswot_map_to_row(m, S, i, A)
    return S


def pack_nested(states, A, caps, inner):
    return nested_opgen.pack(states, A, caps, inner)


KINDS = {
    "mvreg": dict(caps=mvreg_caps, pack=lambda st, A, caps: pack_mvreg(st, A, caps)),
    "orswot": dict(caps=orswot_caps, pack=lambda st, A, caps: pack_orswot(st, A, caps)),
    "nested": dict(caps=nested_caps, pack=lambda st, A, caps: pack_nested(st, A, *caps)),
}


def states_of(kind, seed, n, A, wide=False):
    if kind == "mvreg":
        return [m for _, m in mvreg_batch(seed, n, A)]
    if kind == "orswot":
        return [m for _, m in orswot_batch(seed, n, A)]
    return list(nested_batch(seed, n, A, wide))


# ------------------------------------------------------------------ what a truncate exercises
def _size(v):
    return len(v.vals) if isinstance(v, crdts_ref.MVReg) else len(v.entries)


def _def_events(before, T, ev, pre):
    left = []
    for c in before:
        d = c.clone()
        d.subtract(T)
        if d.is_empty():
            ev[pre + "def_dropped"] += 1
        else:
            ev[pre + "def_changed"] += d != c
            left.append(d)
    ev["collapse"] += len(set(left)) < len(left)


def events(m, T):
    """Counts of what Map::truncate(T) does to `m` (see tests/test_map_truncate_ref.py)."""
    names = ("entry_dropped", "entry_changed", "entry_unchanged", "entry_emptied", "def_dropped", "def_changed",
             "clock_partly", "member_dropped", "vdef_retired", "member_reduced", "inner_entry_dropped",
             "inner_def_dropped", "inner_def_changed", "collapse")
    ev = dict.fromkeys(names, 0)
    t = truncated(m, T)
    for k, (c, v) in m.entries.items():
        if k not in t.entries:
            ev["entry_dropped"] += 1
            continue
        tv = t.entries[k][1]
        same = tv.canonical() == v.canonical()
        ev["entry_unchanged" if same else "entry_changed"] += 1
        ev["entry_emptied"] += _size(v) > 0 and _size(tv) == 0
        if isinstance(v, crdts_ref.Orswot):
            ev["member_dropped"] += any(x not in tv.entries for x in v.entries)
            ev["vdef_retired"] += len(tv.deferred) < len(v.deferred)
            ev["member_reduced"] += any(x in tv.entries and tv.entries[x] != e and not tv.entries[x].is_empty()
                                        for x, e in v.entries.items())
        elif isinstance(v, crdts_ref.Map):
            ev["inner_entry_dropped"] += any(x not in tv.entries for x in v.entries)
            _def_events(v.deferred, T, ev, "inner_")
    _def_events(m.deferred, T, ev, "")
    ev["clock_partly"] += (not t.clock.is_empty()) and t.clock != m.clock
    return ev
