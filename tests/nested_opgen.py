"""Nested-map (TestMap = Map<u64, Map<u64, MVReg>>) op streams for the op-path
tests of crdt_map_map_apply — test infrastructure
(tests/test_map_map_apply_ops.py, tests/test_gpu_map_map_apply.py,
tools/map_map_apply_bench.py).

Per object: a start state (one side of nested_gen.pair: built by the op path,
with concurrent values and a third replica's deferred removes, outer and
inner) and an op list made by nested_gen.make_op through the read contexts of
a diverged clone, some ops doubled, then shuffled — duplicate dots, removes
ahead of their adds and deferrals come from the shuffle. The expected state
is always the Python restatement's (map_kat_runner.apply_raw)."""
import contextlib
import functools
import json
import os
import random

import map_kat_runner as mkr
import map_slab
import nested_gen
from map_slab import crdts_ref

IN_CAPS, IN_INNER = (4, 8, 4), (4, 8, 8, 4)     # outer (kcap, dcap, scap), inner (kcap, mcap, dcap, scap)
OUT_CAPS, OUT_INNER = (8, 8, 8), (8, 8, 8, 8)
OPS_FIELDS = ("obj_end", "kind", "key", "actor", "counter", "key2", "actor2", "counter2", "val", "clk_end", "clk_act",
              "clk_ctr")


def wide_pool(A):
    """Actors on the last lanes of each slot (63, 64, A - 1) among the writers."""
    return sorted({x for x in (0, 1, 31, 62, 63, 64, 65, 99, A - 2, A - 1) if 0 <= x < A})


def gen_object(rng, pool, n_ops=None):
    start, _ = nested_gen.pair(rng, pool)
    c = start.clone()
    actors = rng.sample(pool, 3)
    log = []
    for _ in range(n_ops if n_ops is not None else rng.randrange(3, 10)):
        op = nested_gen.make_op(c, rng, rng.choice(actors))
        mkr.apply_raw(c, op)
        log.append(op)
    ops = log + [op for op in log if rng.random() < 0.15]
    if n_ops is not None:
        ops = ops[:n_ops]
    rng.shuffle(ops)
    return start, ops


@functools.lru_cache(maxsize=None)
def gen_batch(seed, n, A, wide=False):
    """[(start, ops)] * n — computed once per (seed, n, A), never modified."""
    rng = random.Random(seed)
    pool = wide_pool(A) if wide else list(range(A))
    return tuple(gen_object(rng, pool) for _ in range(n))


class LiteralOpsBackend(mkr.PyMapBackend):
    """A KAT backend whose every apply step goes through apply_raw as one
    literal op (the form MapMapOps packs)."""

    def apply_nested_put(self, m, dot, key1, key2, clock, val):
        self.apply_raw(m, {"up": {"dot": list(dot), "key": key1,
                                  "op": {"up": {"dot": list(dot), "key": key2,
                                                "op": {"put": {"clock": [list(p) for p in clock], "val": val}}}}}})

    def apply_rm(self, m, key, pairs):
        self.apply_raw(m, {"rm": {"clock": [list(p) for p in pairs], "key": key}})


def _op_parts(op):
    """(dots, clocks) of a literal op: lists of the [actor, counter] lists it holds."""
    if op == "nop":
        return [], []
    if "rm" in op:
        return [], [op["rm"]["clock"]]
    up = op["up"]
    d, c = _op_parts(up["op"]) if "put" not in up["op"] else ([], [up["op"]["put"]["clock"]])
    return [up["dot"]] + d, c


def op_actors(op):
    dots, clocks = _op_parts(op)
    return {d[0] for d in dots} | {p[0] for c in clocks for p in c}


def relabel_op(op, f):
    """A copy of the literal op with every actor a renamed to f[a]."""
    if op == "nop":
        return op
    if "rm" in op:
        return {"rm": {"clock": [[f[a], c] for a, c in op["rm"]["clock"]], "key": op["rm"]["key"]}}
    if "put" in op:
        return {"put": {"clock": [[f[a], c] for a, c in op["put"]["clock"]], "val": op["put"]["val"]}}
    up = op["up"]
    return {"up": {"dot": [f[up["dot"][0]], up["dot"][1]], "key": up["key"], "op": relabel_op(up["op"], f)}}


def peak_sizes(start, ops):
    """The seven capacities the object needs at any step of its op list."""
    m = start.clone()
    peak = sizes(m)
    for op in ops:
        mkr.apply_raw(m, op)
        peak = tuple(max(a, b) for a, b in zip(peak, sizes(m)))
    return peak


def replay(start, ops):
    m = start.clone()
    for op in ops:
        mkr.apply_raw(m, op)
    return m


def sizes(m):
    """(outer keys, outer deferred, outer set, inner keys, inner values, inner deferred, inner set): the
    seven capacities a state needs."""
    inner = [v for _, v in m.entries.values()]
    mx = lambda xs: max(xs, default=0)  # noqa: E731
    return (len(m.entries), len(m.deferred), mx(len(s) for s in m.deferred.values()),
            mx(len(v.entries) for v in inner), mx(len(r.vals) for v in inner for _, r in v.entries.values()),
            mx(len(v.deferred) for v in inner), mx(len(s) for v in inner for s in v.deferred.values()))


@contextlib.contextmanager
def count_truncations(stats):
    """Counts Map::truncate calls on the restatement while the block runs:
    stats['trunc'] all of them, stats['trunc_def'] those on a map holding
    deferred removes, stats['collapse'] those in which two deferred clocks
    became equal."""
    orig = crdts_ref.Map.truncate

    def counted(self, clock):
        left = 0
        for c in self.deferred:
            c = c.clone()
            c.subtract(clock)
            left += not c.is_empty()
        stats["trunc"] = stats.get("trunc", 0) + 1
        stats["trunc_def"] = stats.get("trunc_def", 0) + bool(self.deferred)
        orig(self, clock)
        stats["collapse"] = stats.get("collapse", 0) + (len(self.deferred) < left)

    crdts_ref.Map.truncate = counted
    try:
        yield stats
    finally:
        crdts_ref.Map.truncate = orig


def batch_stats(batch):
    """Replays the batch on the restatement, counting what the streams exercise."""
    st = dict(ups=0, dup=0, up_up=0, up_rm=0, up_nop=0, rm=0, nop=0, end_outer_def=0, end_inner_def=0,
              peak=(0,) * 7)
    with count_truncations(st):
        for start, ops in batch:
            m = start.clone()
            peak = sizes(m)
            for op in ops:
                if op == "nop":
                    st["nop"] += 1
                elif "rm" in op:
                    st["rm"] += 1
                else:
                    up = op["up"]
                    st["ups"] += 1
                    if m.clock.get(up["dot"][0]) >= up["dot"][1]:
                        st["dup"] += 1
                    st["up_nop" if up["op"] == "nop" else "up_rm" if "rm" in up["op"] else "up_up"] += 1
                mkr.apply_raw(m, op)
                peak = tuple(max(a, b) for a, b in zip(peak, sizes(m)))
            st["peak"] = tuple(max(a, b) for a, b in zip(st["peak"], peak))
            st["end_outer_def"] += bool(m.deferred)
            st["end_inner_def"] += any(v.deferred for _, v in m.entries.values())
    return st


def pack(states, A, caps, inner):
    import crdts_hip

    S = crdts_hip.MapMapSlab.alloc(len(states), A, *caps, inner)
    for i, m in enumerate(states):
        map_slab.nested_map_to_row(m, S, i, A)
    return S


@functools.lru_cache(maxsize=None)
def reference(seed, n, A, wide=False):
    """(batch, S, E): the streams, the packed start rows (IN caps) and the
    restatement's rows after the whole stream (OUT caps) — computed once."""
    batch = gen_batch(seed, n, A, wide)
    S = pack([s for s, _ in batch], A, IN_CAPS, IN_INNER)
    E = pack([replay(s, ops) for s, ops in batch], A, OUT_CAPS, OUT_INNER)
    return batch, S, E


def assert_rows(got, exp, rows=None, what=""):
    """Canonical forms of two host / device MapMapSlabs equal on `rows`, outer and inner."""
    import numpy as np

    g, e = got.canonical(), exp.canonical()
    n = e.n
    rows = np.arange(n) if rows is None else np.asarray(rows)
    for gs, es, per, tag in ((g, e, 1, "outer"), (g.inner, e.inner, e.kcap, "inner")):
        for f in es.a:
            d = (np.asarray(gs.a[f]) != np.asarray(es.a[f])).reshape(n, -1).any(axis=1)[rows] if n else np.zeros(0, bool)
            bad = rows[np.nonzero(d)[0]]
            assert bad.size == 0, f"{what} {tag} {f}: {bad.size} objects differ, first {bad[:5].tolist()}"


# ------------------------------------------------------------ hand-built cases
def load_cases():
    with open(os.path.join(mkr.GOLDEN, "nested_apply_cases.json")) as f:
        return json.load(f)["cases"]


def _vc(pairs):
    return crdts_ref.VClock([tuple(p) for p in pairs])


def _defs(d):
    return sorted((c.canonical(), tuple(sorted(s))) for c, s in d.items())


def check_case_state(m, checks, where=""):
    """The case's checks on a restatement-form state `m`."""
    for ck in checks:
        w = f"{where} {ck}"
        if ck[0] == "clock":
            assert m.clock == _vc(ck[1]), w
        elif ck[0] == "entry_clock":
            assert ck[1] in m.entries and m.entries[ck[1]][0] == _vc(ck[2]), w
        elif ck[0] == "no_entry":
            assert ck[1] not in m.entries, w
        elif ck[0] == "deferred":
            assert _defs(m.deferred) == sorted((_vc(c).canonical(), tuple(sorted(s))) for c, s in ck[1]), w
        elif ck[0] == "inner_deferred":
            # in the order given: CLOCK ORDER, the slab's order
            v = m.entries[ck[1]][1]
            exp = [(_vc(c).canonical(), tuple(sorted(s))) for c, s in ck[2]]
            assert [(c.canonical(), tuple(sorted(v.deferred[c]))) for c in crdts_ref.clock_order(list(v.deferred))] == exp, w
        elif ck[0] == "inner_clock":
            assert m.entries[ck[1]][1].clock == _vc(ck[2]), w
        elif ck[0] == "inner_len":
            assert len(m.entries[ck[1]][1].entries) == ck[2], w
        elif ck[0] == "inner_read":
            assert sorted(m.entries[ck[1]][1].entries[ck[2]][1].read()) == sorted(ck[3]), w
        else:
            raise ValueError(ck[0])


def case_start(case):
    return replay(mkr.nested_map(), case["pre"])
