"""Test helper: the Map value batches of tests/map_lift.py — op-simulated
states with every counter, key, member and value lifted onto a u64 edge — as
host slabs with the oracle's answers, made once and shared (read-only) by the
CPU proof (tests/test_map_lift.py) and the GPU parity tests
(tests/test_gpu_map_edges.py). The oracle of each entry point is the one its
existing test uses: the C++ oracle for the Map<MVReg> and Map<Orswot> merges
and op paths, the Python restatement for the nested map and for truncate."""
import functools
import random

import map_lift as ml
import map_opgen
import map_orswot_opgen as og
import map_slab
import map_truncgen as tg
import nested_gen
import nested_opgen as ng
import oracle_ffi

FLOOR = 20  # the fewest objects of a batch that must show each property
KINDS = ("mvreg", "orswot", "nested")
MERGE_WIDTHS = (2, 16, 63, 64, 65, 100, 128)
N_MERGE = {16: 500, 100: 500}  # the widths of the mutant proofs (at 300 intersection_ignores_counter changes 17..19
N_MERGE_OTHER = 300           # objects); the other widths
MVREG_CAPS = (8, 4, 8, 8)  # tests/test_map_mvreg.py
NESTED_CAPS, NESTED_INNER = (4, 8, 4), (4, 8, 8, 4)  # tests/test_gpu_map_nested.py
FROM_ROW = {"mvreg": map_slab.mvreg_map_from_row, "orswot": map_slab.orswot_map_from_row,
            "nested": map_slab.nested_map_from_row}


def alloc(kind, n, A, caps, device=None):
    import crdts_hip

    if kind == "mvreg":
        return crdts_hip.MapSlab.alloc(n, A, *caps, device=device)
    if kind == "orswot":
        return crdts_hip.MapOrswotSlab.alloc(n, A, device=device, **caps)
    return crdts_hip.MapMapSlab.alloc(n, A, *caps[0], caps[1], device=device)


def summed(kind, caps):
    if kind == "mvreg":
        return tuple(2 * c for c in caps)
    if kind == "orswot":
        return {k: 2 * c for k, c in caps.items()}
    return tuple(2 * c for c in caps[0]), tuple(2 * c for c in caps[1])


def caps_of(kind, S):
    if kind == "mvreg":
        return (S.kcap, S.mcap, S.dcap, S.scap)
    if kind == "orswot":
        return dict(S.caps)
    return (S.kcap, S.dcap, S.scap), S.inner_caps


def pack(kind, states, A, caps):
    S = alloc(kind, len(states), A, caps)
    to_row = {"mvreg": map_slab.mvreg_map_to_row, "orswot": map_slab.orswot_map_to_row,
              "nested": map_slab.nested_map_to_row}[kind]
    for i, m in enumerate(states):
        to_row(m, S, i, A, zero=False)
    return S


def unpack(kind, S):
    return [FROM_ROW[kind](S, i) for i in range(int(S.a["n_keys"].shape[0]))]


def _nested_pairs(seed, n, A):
    rng = random.Random(seed)
    # (the generator's three replicas take three actors: at two actors the third replica shares one)
    pool = list(range(A)) if A >= 3 else [0, 1, 0]
    if A > 64:  # actors of both slots of a lane among the writers
        pool = ng.wide_pool(A)
    return [nested_gen.pair(rng, pool) for _ in range(n)]


def _late_removes(seed, pairs, dcap):
    """In a quarter of the pairs a third replica that has merged both sides
    removes a key with its whole map clock (x.clock ⊔ y.clock), and the remove
    reaches `other` — in half of these `self` too — before anything else of
    that replica does: it stays deferred there, and the merge of the pair is
    the first state whose clock EQUALS the remove's. The generators' own
    deferred removes are behind or ahead of the merged clock, hardly ever at
    it, so without these no input tells `d <= c` from `d < c`."""
    rng = random.Random(seed)
    for x, y in pairs:
        keys = sorted(set(x.entries) | set(y.entries))
        if not keys or rng.random() >= 0.25:
            continue
        z = x.clock.clone()
        z.merge(y.clock)
        for m in (y, x) if rng.random() < 0.5 else (y,):
            if len(m.deferred) < dcap:
                m.apply_rm(rng.choice(keys), z)
    return pairs


def _future_removes(seed, pairs, A, dcap):
    """In half of the pairs that third replica goes on writing and removes
    keys with its whole clock again, so that the removes stay deferred through
    the merge and the output's deferred list holds clocks that differ from the
    merged clock z in one place: z with actor a one and two steps ahead (their
    CLOCK ORDER is decided by two counters at a; past 64 actors a is, half the
    time, an actor >= 64), and z with one more present actor ahead; past 64
    actors also z + {a: 1} and z + {a + 64: ahead} for an actor a < 64 that z
    lacks (decided by the prefix rule at a, where the side lacking a holds the
    lane's other actor)."""
    rng = random.Random(seed)
    for x, y in pairs:
        keys = sorted(set(x.entries) | set(y.entries))
        if not keys or rng.random() >= 0.5:
            continue
        z = x.clock.clone()
        z.merge(y.clock)
        present = sorted(z.dots)
        if not present:
            continue
        high = [a for a in present if a >= 64]
        a1 = rng.choice(high) if high and rng.random() < 0.5 else rng.choice(present)
        clocks = [{a1: z.get(a1) + 1}, {a1: z.get(a1) + 2}]
        lacking = [a for a in range(min(64, A - 64)) if not z.get(a)] if A > 64 else []
        if lacking:
            a = rng.choice(lacking)
            clocks += [{a: 1}, {a + 64: z.get(a + 64) + 1}]
        else:
            a2 = rng.choice(present)
            clocks.append({a2: z.get(a2) + 1})
        for ahead in clocks:
            d = z.clone()
            d.dots.update(ahead)
            for m in (y, x) if rng.random() < 0.5 else (y,):
                if len(m.deferred) < dcap:
                    m.apply_rm(rng.choice(keys), d)
    return pairs


@functools.lru_cache(maxsize=None)
def generated_pairs(kind, A, n):
    """-> (caps, [(x, y)] * n): the replica pairs as the existing random-parity
    tests generate them (restatement objects) plus _late_removes and
    _future_removes, before any lift."""
    if kind == "mvreg":
        caps = MVREG_CAPS
        L, R = oracle_ffi.map_generate(100 + A, n, A, 8 if A >= 16 else 4, 12, caps)
        dcap = caps[2]
    elif kind == "orswot":
        caps = dict(oracle_ffi.MAP_ORSWOT_CAPS)
        L, R = oracle_ffi.map_orswot_generate(0xB0B + A, n, A, keys=4, members=6, ops=10, pct_future=35)
        dcap = caps["dcap"]
    else:
        caps, pairs, dcap = (NESTED_CAPS, NESTED_INNER), _nested_pairs(A, n, A), NESTED_CAPS[1]
    if kind != "nested":
        pairs = list(zip(unpack(kind, L), unpack(kind, R)))
    if kind != "nested":
        # the C++ generators spread their writers over all actors (the Orswot one keeps the last for future
        # removes): in the odd objects the last actor changes places with the pair's busiest, so that actor A - 1
        # (past 64 actors: a lane's second slot) writes in half of the batch
        for i in range(1, len(pairs), 2):
            x, y = pairs[i]
            top = max(range(A), key=lambda a: x.clock.get(a) + y.clock.get(a))
            swap = {a: a for a in range(A)}
            swap[top], swap[A - 1] = A - 1, top
            pairs[i] = (map_slab.relabel(x, swap), map_slab.relabel(y, swap))
    return caps, _future_removes(A + 1, _late_removes(A, pairs, dcap), A, dcap)


def oracle_merge(kind, S, O, A, caps):
    """self ⊔ other by the entry point's own oracle -> host slab of the summed capacities."""
    if kind == "mvreg":
        return oracle_ffi.map_merge(S, O, A)
    if kind == "orswot":
        return oracle_ffi.map_orswot_merge(S, O, A)
    out = []
    for x, y in zip(unpack(kind, S), unpack(kind, O)):
        x.merge(y)
        out.append(x)
    return pack(kind, out, A, summed(kind, caps))


@functools.lru_cache(maxsize=None)
def merge_case(kind, A, lifted=True, n=None):
    """-> dict: A, caps, base (the generated pairs), lifts, pairs (lifted), S,
    O (host slabs), SO, OS (the oracle's self ⊔ other and other ⊔ self)."""
    n = n or N_MERGE.get(A, N_MERGE_OTHER)
    caps, base = generated_pairs(kind, A, n)
    lifts = ml.draw_lifts(0x11F7 + A, [((x, y), None, ()) for x, y in base], kind, identity=not lifted)
    pairs = [(ml.lift_map(x, f), ml.lift_map(y, f)) for (x, y), f in zip(base, lifts)]
    S, O = pack(kind, [p[0] for p in pairs], A, caps), pack(kind, [p[1] for p in pairs], A, caps)
    return dict(A=A, caps=caps, base=base, lifts=lifts, pairs=pairs, S=S, O=O,
                SO=oracle_merge(kind, S, O, A, caps), OS=oracle_merge(kind, O, S, A, caps))


def assert_merge_batch(kind, A):
    """What every merge batch must hold: the last actor, past 64 actors both
    slots of a lane, counters from 2^63, and outputs with several deferred clocks."""
    import numpy as np

    c = merge_case(kind, A)
    for X, out in ((c["S"], c["SO"]), (c["O"], c["OS"])):
        assert (X.a["clock"][:, A - 1] != 0).sum() >= 10, (kind, A)
        assert A <= 64 or (X.a["clock"][:, 64:].any(axis=1) & X.a["clock"][:, :64].any(axis=1)).sum() >= FLOOR
        assert (X.a["clock"] >= np.uint64(2**63)).any(axis=1).sum() >= FLOOR
        assert (out.a["n_def"] > 1).sum() >= FLOOR and (out.a["n_keys"] > 1).sum() >= FLOOR


@functools.lru_cache(maxsize=None)
def truncate_case(kind, A, lifted=True, n=200):
    """-> dict: base states and clocks, lifts, states, clocks (lifted), caps,
    S, rows (the truncating clock rows) and E, the restatement's truncated rows."""
    base = tg.states_of(kind, 0xB0 + A, n, A, A > 16)
    _, bclocks = tg.draw(5, base, A)
    lifts = ml.draw_lifts(0x7C + A, [((m,), None, (T,)) for m, T in zip(base, bclocks)], kind, identity=not lifted)
    states = [ml.lift_map(m, f) for m, f in zip(base, lifts)]
    clocks = [ml.lift_clock(T, f) for T, f in zip(bclocks, lifts)]
    caps = tg.KINDS[kind]["caps"](states)
    E = tg.KINDS[kind]["pack"]([tg.truncated(m, T) for m, T in zip(states, clocks)], A, caps)
    return dict(A=A, caps=caps, base=base, base_clocks=bclocks, lifts=lifts, states=states, clocks=clocks,
                S=tg.KINDS[kind]["pack"](states, A, caps), rows=tg.clock_rows(clocks, A), E=E)


APPLY_CAPS = {"mvreg": ((4, 4, 4, 4), (8, 8, 8, 8)), "orswot": (og.caps(4), og.caps(8)),
              "nested": ((ng.IN_CAPS, ng.IN_INNER), (ng.OUT_CAPS, ng.OUT_INNER))}


def replay(kind, start, ops):
    m = start.clone()
    for op in ops:
        {"mvreg": map_opgen.apply_op, "orswot": og.apply_op, "nested": ng.mkr.apply_raw}[kind](m, op)
    return m


@functools.lru_cache(maxsize=None)
def apply_case(kind, A, lifted=True, n=300):
    """-> dict: base [(start state, pre ops, ops)], lifts, starts, ops
    (lifted), S and E: the start rows and the rows after the ops, by the
    oracle of the entry point's own op-path test (the C++ handles for MVReg
    and Orswot values, the restatement for the nested map)."""
    if kind == "nested":
        base = [(s, [], list(ops)) for s, ops in ng.gen_batch(0x0A55 + A, n, A, A > 16)]
    else:
        gen, new = (map_opgen, lambda: map_slab.crdts_ref.Map(map_slab.crdts_ref.MVReg)) if kind == "mvreg" else \
            (og, og.new_map)
        base = [(replay(kind, new(), pre), pre, ops) for pre, ops in gen.gen_batch(0xA991 + A, n, A)]
    lifts = ml.draw_lifts(0xA9 + A, [((s,), pre + ops, ()) for s, pre, ops in base], kind, identity=not lifted)
    lo = ml.LIFT_OPS[kind]
    starts = [ml.lift_map(s, f) for (s, _, _), f in zip(base, lifts)]
    ops = [lo(o, f) for (_, _, o), f in zip(base, lifts)]
    (cin, cout) = APPLY_CAPS[kind]
    if kind == "nested":
        S, E = pack(kind, starts, A, cin), pack(kind, [replay(kind, s, o) for s, o in zip(starts, ops)], A, cout)
    else:
        gen = map_opgen if kind == "mvreg" else og
        S, E = gen.oracle_slabs(oracle_ffi, [(lo(pre, f), o) for (_, pre, _), f, o in zip(base, lifts, ops)], A, cin,
                                cout)
    return dict(A=A, caps=(cin, cout), base=base, lifts=lifts, starts=starts, ops=ops, S=S, E=E)


def rows_differ(kind, got, exp):
    """The objects on which two slabs' canonical forms differ (outer and inner arrays)."""
    import numpy as np

    g, e = got.canonical(), exp.canonical()
    n = int(e.a["n_keys"].shape[0])
    bad = np.zeros(n, bool)
    for f in e.a:
        bad |= (np.asarray(g.a[f]) != np.asarray(e.a[f])).reshape(n, -1).any(axis=1)
    if kind == "nested":
        for f in e.inner.a:
            bad |= (np.asarray(g.inner.a[f]) != np.asarray(e.inner.a[f])).reshape(n, -1).any(axis=1)
    return np.nonzero(bad)[0]
