"""GPU parity: Map<u64, Map<u64, MVReg<u64, A>, A>, A>::apply, batched
(crdt_map_map_apply, rust-crdt_amd/csrc/map_map_apply.hip) — the op path of
the reference's own Map test type (TestMap, test/map.rs:4-8) — slab-row exact
against the Python restatement through map_kat_runner.apply_raw (Map::apply
src/map.rs:160-190, apply_rm :336-350, apply_deferred :325-333, Map::truncate
:131-158, MVReg Put src/mvreg.rs:158-186): the seven nested KATs with every
apply on the kernel, generated streams (tests/nested_opgen.py), structures
past one wave's lanes, the hand-built cases of
tests/golden/nested_apply_cases.json and the call's error contract
(include/crdts_hip.h)."""
import ctypes as C
import random

import numpy as np
import pytest

import map_kat_runner as mkr
import map_slab
import nested_opgen as ng

pytestmark = pytest.mark.gpu
A = 16
SEED = 0x0A55


def _patterned(n, n_actors, caps, inner):
    """A device output slab holding a pattern: the kernel writes only the used
    slots, so canonical forms are compared."""
    import crdts_hip

    out = crdts_hip.MapMapSlab.alloc(n, n_actors, *caps, inner, device="cuda")
    for v in list(out.a.values()) + list(out.inner.a.values()):
        v.fill_(0x5A5A5A5A)
    return out


def _apply(gpu, S, per_obj, n_actors, caps=ng.OUT_CAPS, inner=ng.OUT_INNER, **kw):
    import crdts_hip

    ops = per_obj if isinstance(per_obj, crdts_hip.MapMapOps) else crdts_hip.MapMapOps.from_lists(per_obj)
    S = S if hasattr(S.a["clock"], "data_ptr") else S.to("cuda")
    return gpu.map_map_apply(S, ops, n_actors, out=_patterned(S.n, n_actors, caps, inner), **kw)


# ------------------------------------------------------------------ 1. KATs
IN_CAPS, IN_INNER = ng.IN_CAPS, ng.IN_INNER


def _interned(maps, ops=()):
    acts = sorted(set().union(*[map_slab.actors_of(m) for m in maps], *[ng.op_actors(o) for o in ops])) or [0]
    fwd = {a: i for i, a in enumerate(acts)}
    return fwd, {i: a for a, i in fwd.items()}, len(acts)


class GpuNestedApplyBackend(ng.LiteralOpsBackend):
    """Every apply step is one crdt_map_map_apply call on a one-row slab
    (actors interned order-preserving over state ∪ op); after every apply the
    state must be the Python restatement's. Merges run on crdt_map_map_merge."""

    def __init__(self, eng):
        self.eng = eng
        self.applies = 0

    def apply_raw(self, m, op):
        import crdts_hip

        fwd, back, n = _interned([m], [op])
        S = crdts_hip.MapMapSlab.alloc(1, n, *IN_CAPS, IN_INNER)
        map_slab.nested_map_to_row(map_slab.relabel(m, fwd), S, 0, n)
        R = _apply(self.eng, S, [[ng.relabel_op(op, fwd)]], n).host()
        out = map_slab.relabel(map_slab.nested_map_from_row(R, 0), back)
        exp = m.clone()
        mkr.apply_raw(exp, op)
        assert out == exp, (op, out.canonical(), exp.canonical())
        m.clock, m.entries, m.deferred = out.clock, out.entries, out.deferred
        self.applies += 1

    def merge(self, dst, src):
        import crdts_hip

        fwd, back, n = _interned([dst, src])
        S = crdts_hip.MapMapSlab.alloc(1, n, *IN_CAPS, IN_INNER)
        O = crdts_hip.MapMapSlab.alloc(1, n, *IN_CAPS, IN_INNER)
        map_slab.nested_map_to_row(map_slab.relabel(dst, fwd), S, 0, n)
        map_slab.nested_map_to_row(map_slab.relabel(src, fwd), O, 0, n)
        R = self.eng.map_map_merge(S.to("cuda"), O.to("cuda"), n).host()
        out = map_slab.relabel(map_slab.nested_map_from_row(R, 0), back)
        dst.clock, dst.entries, dst.deferred = out.clock, out.entries, out.deferred


KATS = mkr.load_cases(nested=True)


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_nested_kat_applies_on_gpu(case, gpu):
    assert len(KATS) == 7
    be = GpuNestedApplyBackend(gpu)
    got = mkr.run_case(case, be)  # the reference's asserts, on kernel-made states
    assert be.applies == sum(st[0] == "apply" for st in case["steps"])
    exp = mkr.run_case(case, mkr.PyMapBackend())
    assert all(got[k] == exp[k] for k in exp)


# ------------------------------------------------------- 2. generated batch
def test_map_map_apply_generated_batch(gpu):
    """2,000 generated objects at 16 actors, the whole stream in one call."""
    batch, S, E = ng.reference(SEED, 2000, A)
    assert (S.a["n_keys"] > 0).sum() > 400 and (E.a["n_def"] > 0).sum() > 200 and (E.inner.a["n_def"] > 0).sum() > 50
    ng.assert_rows(_apply(gpu, S, [ops for _, ops in batch], A), E)


def test_map_map_apply_chained_single_ops(gpu):
    """The first 200 of them, one op per call, each call's output the next
    call's input: every intermediate state exact."""
    batch, S, _ = ng.reference(SEED, 2000, A)
    batch = batch[:200]
    n = len(batch)
    cur = ng.pack([s for s, _ in batch], A, IN_CAPS, IN_INNER).to("cuda")
    py = [s.clone() for s, _ in batch]
    for t in range(max(len(ops) for _, ops in batch)):
        step = [ops[t:t + 1] for _, ops in batch]
        for m, ops in zip(py, step):
            for op in ops:
                mkr.apply_raw(m, op)
        cur = _apply(gpu, cur, step, A)
        ng.assert_rows(cur, ng.pack(py, A, ng.OUT_CAPS, ng.OUT_INNER), what=f"step {t}")


# ------------------------------------------------- 3. actor-width boundaries
@pytest.mark.parametrize("n_actors", [64, 65, 100, 128])
def test_map_map_apply_actor_widths(gpu, n_actors):
    """One slot per lane up to 64 actors, two from 65: the last lane of each
    slot (actors 63, 64, n_actors - 1) carries dots and clock entries."""
    batch, S, E = ng.reference(0xB0 + n_actors, 300, n_actors, True)
    assert E.a["clock"][:, n_actors - 1].any() and E.a["clock"][:, 63].any()
    assert n_actors == 64 or E.a["clock"][:, 64:].any()
    assert E.inner.a["clock"][:, n_actors - 1].any() and E.inner.a["dclock"][..., n_actors - 1].any()
    ng.assert_rows(_apply(gpu, S, [ops for _, ops in batch], n_actors), E)


# ------------------------------------------------------- 4. long op lists
def test_map_map_apply_long_op_lists(gpu):
    """Exactly 64, 65 and 150 ops: the kernel stages op headers 64 at a time
    with the first 64 clock pairs of each chunk, and reads the pairs past that
    window from the op arrays."""
    rng = random.Random(0x10E6)
    batch = [ng.gen_object(rng, list(range(A)), n_ops=n) for n in (64, 65, 150)]
    assert [len(ops) for _, ops in batch] == [64, 65, 150]
    import crdts_hip

    arrs = dict(zip(ng.OPS_FIELDS, crdts_hip.MapMapOps.arrays_from_lists([ops for _, ops in batch])))
    ends = arrs["clk_end"]
    assert int(ends[63]) > 64 and int(ends[64 + 65 + 127]) - int(ends[64 + 65 + 63]) > 64  # a chunk's pairs past 64
    peak = tuple(max(x) for x in zip(*[ng.peak_sizes(s, ops) for s, ops in batch]))
    caps = tuple(max(8, x) for x in peak[:3])
    inner = tuple(max(8, x) for x in peak[3:])
    assert max(caps + inner) <= 128
    S = ng.pack([s for s, _ in batch], A, IN_CAPS, IN_INNER)
    E = ng.pack([ng.replay(s, ops) for s, ops in batch], A, caps, inner)
    ng.assert_rows(_apply(gpu, S, [ops for _, ops in batch], A, caps, inner), E)


# -------------------------------- 5. ordered structures past one wave's lanes
def _put(dot, key, key2, clock, val):
    return {"up": {"dot": list(dot), "key": key,
                   "op": {"up": {"dot": list(dot), "key": key2, "op": {"put": {"clock": [list(p) for p in clock], "val": val}}}}}}


def _irm(dot, key, key2, clock):
    return {"up": {"dot": list(dot), "key": key, "op": {"rm": {"clock": [list(p) for p in clock], "key": key2}}}}


def _rm(key, clock):
    return {"rm": {"clock": [list(p) for p in clock], "key": key}}


# One op whose own clock has more than 64 pairs (possible only past 64 actors):
# 100 pairs over actors 0..127 with gaps, actors 63, 64 and 127 among them. The
# staged window holds 64 pairs, so the op's pairs are read from the op arrays,
# 64 at a time, in two rounds.
A128 = 128
WIDE_CLOCK = [(a, a + 1) for a in range(A128) if a % 9 not in (2, 6)]


def _wide_clock_batch():
    """Three objects at 128 actors, each with entries under dots of actors 63,
    64 and 127: the wide Rm as the first op of its list; as op 65 (the first of
    the second staged chunk: its pairs start the refilled window); wide Ups (a
    Put's clock, an inner Rm's clock) as ops 4 and 5, inside a chunk whose
    window starts before them."""
    start = ng.replay(mkr.nested_map(), [_put((63, 5), 7, 1, [(63, 5)], 1), _put((64, 3), 7, 2, [(63, 5), (64, 3)], 2),
                                         _put((127, 200), 8, 1, [(127, 200)], 3)])
    fill = [_put((1, n + 1), 9 + n % 3, 1, [(1, n + 1)], 100 + n) for n in range(64)]
    rm = _rm(7, WIDE_CLOCK)                    # empties key 7's entry and is deferred (actor 127 is ahead of it)
    up = _put((5, 9), 8, 1, WIDE_CLOCK, 4)     # inner key 1's value (127, 200) is not covered: two values
    irm = _irm((5, 10), 8, 1, WIDE_CLOCK)      # deferred in the inner map; only the value under (127, 200) stays
    return [(start, [rm] + fill[:3]), (start, fill + [rm, _rm(8, [(127, 200)])]), (start, fill[:3] + [up, irm, rm])]


def test_map_map_apply_op_clock_past_64_pairs(gpu):
    import crdts_hip

    assert len(WIDE_CLOCK) == 100 and {63, 64, 127} <= {a for a, _ in WIDE_CLOCK}
    batch = _wide_clock_batch()
    lists = [ops for _, ops in batch]
    wide = [list(p) for p in WIDE_CLOCK]
    assert lists[0][0]["rm"]["clock"] == wide and lists[1][64]["rm"]["clock"] == wide
    assert lists[2][3]["up"]["op"]["up"]["op"]["put"]["clock"] == wide and lists[2][4]["up"]["op"]["rm"]["clock"] == wide
    arrs = dict(zip(ng.OPS_FIELDS, crdts_hip.MapMapOps.arrays_from_lists(lists)))
    ends = np.asarray(arrs["clk_end"]).astype(np.int64)
    assert (np.diff(np.concatenate([[0], ends])) > 64).sum() == 5  # the batch holds ops with more than 64 pairs
    caps, inner = (8, 8, 8), (8, 8, 8, 8)
    S = ng.pack([s for s, _ in batch], A128, caps, inner)
    E = ng.pack([ng.replay(s, ops) for s, ops in batch], A128, caps, inner)
    assert (E.a["n_def"] == 1).all() and (np.count_nonzero(E.a["dclock"][:, 0], axis=1) == 100).all()
    assert (np.count_nonzero(E.inner.a["dclock"].reshape(3, -1), axis=1) == [0, 0, 100]).all()  # the inner deferred Rm
    ng.assert_rows(_apply(gpu, S, lists, A128, caps, inner), E)


@pytest.mark.parametrize("at", [0, 64])
def test_map_map_apply_op_clock_past_64_pairs_noncanonical(gpu, at):
    """The same clock with pair 70's actor repeated (in the second round of 64):
    CRDT_ENONCANON for its object, the neighbour exact."""
    import crdts_hip

    bad = list(WIDE_CLOCK)
    bad[70] = (bad[69][0], bad[70][1])
    fill = [_put((1, n + 1), 9, 1, [(1, n + 1)], n) for n in range(at)]
    S = crdts_hip.MapMapSlab.alloc(2, A128, *IN_CAPS, IN_INNER)
    E = ng.pack([ng.replay(mkr.nested_map(), GOOD), mkr.nested_map()], A128, ng.OUT_CAPS, ng.OUT_INNER)
    got = _apply(gpu, S, _raw_ops([GOOD, fill + [_rm(3, bad)]]), A128, check_status=False)
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    ng.assert_rows(got, E, rows=[0])
    gpu.status()


BIG = 100  # the outer key whose inner map is the large one


def _wide_case():
    """63 outer keys, 62 outer deferred clocks; key 100's inner map: 72 keys, a
    register of three concurrent values, 62 inner deferred clocks. The op list
    edits the front, the middle and the end of the outer keys (63 -> 66 -> 62),
    of the outer deferred clocks (-> 66, CLOCK ORDER), of a deferred key set,
    of the inner keys and of the inner deferred clocks (-> 66), truncates the
    large inner map and retires a deferred clock by the Up that covers it."""
    pre = [_put((0, k + 1), 10 * (k + 1), 1, [(0, k + 1)], k) for k in range(63)]
    pre += [_put((1, j + 1), BIG, 10 * (j + 1), [(1, j + 1)], j) for j in range(70)]
    pre += [_put((a, 1), BIG, 5, [(a, 1)], 500 + a) for a in (4, 5, 6)]                    # three concurrent values
    pre += [_irm((7, d + 1), BIG, 7, [(2, 100 + d)]) for d in range(62)]                  # inner deferred, key 7 absent
    pre += [_rm(5, [(3, 100 + d)]) for d in range(62)]                                    # outer deferred, key 5 absent
    ops = [
        _put((8, 1), 1, 1, [(8, 1)], 1000),             # outer keys: below the first,
        _put((8, 2), 355, 1, [(8, 2)], 1001),           # between two,
        _put((8, 3), 10000, 1, [(8, 3)], 1002),         # above the last: 66 keys
        _rm(1, [(8, 1)]),                               # the first entry emptied,
        _rm(350, [(0, 35)]),                            # a middle one,
        _rm(10000, [(8, 3)]),                           # the last,
        _rm(20, [(0, 2)]),                              # and the second: 62 keys
        _rm(6, [(0, 99)]),                              # outer future clocks: the front of CLOCK ORDER,
        _rm(6, [(3, 130), (9, 1)]),                     # the middle ([(3, 130)] is its proper prefix),
        _rm(6, [(9, 5), (10, 1)]),                      # the end,
        _rm(6, [(9, 5)]),                               # and a proper prefix of the last one, before it: 66
        _rm(2, [(3, 110)]),                             # an existing deferred clock: a key below its set's {5}
        _rm(999, [(3, 110)]),                           # and one above
        _irm((8, 4), BIG, 7, [(0, 99)]),                # inner future clocks: front,
        _irm((8, 5), BIG, 7, [(2, 130), (9, 1)]),       # middle,
        _irm((8, 6), BIG, 7, [(9, 5), (10, 1)]),        # end,
        _irm((8, 7), BIG, 7, [(9, 5)]),                 # a proper prefix before it: 66 inner deferred
        _put((8, 8), BIG, 0, [(8, 8)], 2000),           # inner keys: front,
        _put((8, 9), BIG, 355, [(8, 9)], 2001),         # middle,
        _put((8, 10), BIG, 10000, [(8, 10)], 2002),     # end
        _irm((8, 11), BIG, 1, [(0, 10)]),               # inner entries emptied: the first of the old ones,
        _irm((8, 12), BIG, 350, [(1, 35)]),             # a middle one,
        _irm((8, 13), BIG, 10000, [(8, 10)]),           # the last
        _put((8, 14), BIG, 5, [(4, 1), (5, 1), (8, 14)], 777),  # a Put over two of the three concurrent values
        {"up": {"dot": [8, 15], "key": BIG, "op": "nop"}},
        "nop",
        _rm(BIG, [(1, 30)]),                            # Map::truncate of the large inner map: 30 inner entries go
        _rm(40, [(8, 16)]),                             # deferred in the middle of the outer list,
        _put((8, 16), 40, 2, [(8, 16)], 3000),          # and the Up that retires it, truncating key 40's inner map
    ]
    return ng.replay(mkr.nested_map(), pre), ops


def test_map_map_apply_wide_ordered_structures(gpu):
    start, ops = _wide_case()
    in_caps, in_inner = (64, 64, 4), (72, 4, 64, 4)
    out_caps, out_inner = (68, 68, 4), (76, 4, 68, 4)
    z = ng.sizes(start)
    assert z[0] == 63 and z[1] == 62 and z[3] == 72 and z[4] == 3 and z[5] == 62
    trace = []
    py = start.clone()
    for op in ops:
        mkr.apply_raw(py, op)
        trace.append(ng.sizes(py))
    assert max(t[0] for t in trace) == 66 and trace[6][0] == 62 and trace[-1][0] == 62
    assert max(t[1] for t in trace) == 67 and trace[-1][1] == 66 and max(t[2] for t in trace) == 3
    assert max(t[5] for t in trace) == 66 and max(t[3] for t in trace) == 75
    assert len(py.entries[BIG][1].entries) == 75 - 3 - 30 and len(py.entries[BIG][1].entries[5][1].vals) == 2
    S = ng.pack([start], A, in_caps, in_inner)
    # the whole list in one call, and every prefix of it
    for t in range(len(ops), 0, -1):
        E = ng.pack([ng.replay(start, ops[:t])], A, out_caps, out_inner)
        ng.assert_rows(_apply(gpu, S, [ops[:t]], A, out_caps, out_inner), E, what=f"ops[:{t}] {ops[t - 1]}")


# ------------------------------------------------------ 6. hand-built cases
CASES = ng.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_map_map_apply_hand_built_case(case, gpu):
    start = ng.case_start(case)
    S = ng.pack([start], A, IN_CAPS, IN_INNER)
    for ops in [case["ops"]] + ([case["alt_ops"]] if "alt_ops" in case else []):
        R = _apply(gpu, S, [ops], A)
        ng.assert_rows(R, ng.pack([ng.replay(start, ops)], A, ng.OUT_CAPS, ng.OUT_INNER), what=case["name"])
        ng.check_case_state(map_slab.nested_map_from_row(R.canonical(), 0), case["checks"], case["name"])


# ------------------------------------------------ 7. copy-through and empties
def test_map_map_apply_copy_through_and_empties(gpu):
    import crdts_hip

    gen = ng.gen_batch(0xE0, 8, A)
    empty = mkr.nested_map()
    batch = [gen[0],                                   # a map with ops
             (gen[2][0], []),                          # no ops, between two that have some
             gen[3],
             (empty, ["nop"] + list(gen[5][1])),       # an all-empty self map
             (empty, [])]                              # empty map, no ops
    S = ng.pack([s for s, _ in batch], A, IN_CAPS, IN_INNER)
    E = ng.pack([ng.replay(s, ops) for s, ops in batch], A, ng.OUT_CAPS, ng.OUT_INNER)
    assert S.a["n_keys"][1] > 0 and S.a["n_keys"][3] == 0 and not S.a["clock"][3].any()
    ng.assert_rows(_apply(gpu, S, [ops for _, ops in batch], A), E)
    # n_ops == 0: null op arrays, every object copied through (into capacities equal to self's)
    none = crdts_hip.MapMapOps.from_lists([[] for _ in batch])
    assert none.n_ops == 0 and none.cops().kind is None and none.cops().clk_act is None
    ng.assert_rows(_apply(gpu, S, none, A, IN_CAPS, IN_INNER), S)
    # n_obj == 0
    Z = crdts_hip.MapMapSlab.alloc(0, A, *IN_CAPS, IN_INNER)
    out = gpu.map_map_apply(Z.to("cuda"), crdts_hip.MapMapOps.from_lists([]), A, out_caps=ng.OUT_CAPS,
                            inner_out_caps=ng.OUT_INNER)
    assert out.n == 0


# ------------------------------------------------------------- 8. capacities
WHICH = ("kcap", "dcap", "scap", "inner_kcap", "inner_mcap", "inner_dcap", "inner_scap")


def _overflowing(which):
    """An op list on the empty map that needs 5 slots of `which`."""
    if which == "kcap":
        return [{"up": {"dot": [0, k + 1], "key": 100 + k, "op": "nop"}} for k in range(5)]
    if which == "dcap":  # five future clocks
        return [_rm(7, [(3, 10 + d)]) for d in range(5)]
    if which == "scap":  # five keys under one future clock
        return [_rm(100 + k, [(3, 10)]) for k in range(5)]
    if which == "inner_kcap":
        return [_put((0, k + 1), 1, 100 + k, [(0, k + 1)], k) for k in range(5)]
    if which == "inner_mcap":  # five concurrent values of one inner key
        return [_put((a, 1), 1, 7, [(a, 1)], a) for a in range(5)]
    if which == "inner_dcap":
        return [_irm((0, d + 1), 1, 7, [(3, 10 + d)]) for d in range(5)]
    return [_irm((0, k + 1), 1, 100 + k, [(3, 10)]) for k in range(5)]


def _small_neighbours():
    """Two generated objects that need at most 4 slots of every capacity at every step."""
    fit = [(s, ops) for s, ops in ng.gen_batch(SEED, 2000, A)[:200] if max(ng.peak_sizes(s, ops)) <= 4 and ops]
    assert len(fit) >= 2
    return fit[0], fit[1]


def _capacity_check(gpu, S, lists_ok, lists_over, E, caps, inner):
    import crdts_hip

    ng.assert_rows(_apply(gpu, S, lists_ok, A, caps, inner), E)  # it fits: the status is clean and the rows exact
    with pytest.raises(crdts_hip.CrdtError) as e:
        _apply(gpu, S, lists_over, A, caps, inner)
    assert e.value.code == crdts_hip.CRDT_ECAPACITY
    got = _apply(gpu, S, lists_over, A, caps, inner, check_status=False)
    with pytest.raises(crdts_hip.CrdtError):
        gpu.status()
    ng.assert_rows(got, E, rows=[0, 2], what="neighbours")
    gpu.status()  # the latch is cleared: the context is usable again


@pytest.mark.parametrize("which", WHICH)
def test_map_map_apply_capacity(gpu, which):
    n0, n1 = _small_neighbours()
    caps = tuple(4 if c == which else 8 for c in WHICH[:3])
    inner = tuple(4 if c == which else 8 for c in WHICH[3:])
    over = _overflowing(which)
    S = ng.pack([n0[0], mkr.nested_map(), n1[0]], A, (4, 4, 4), (4, 4, 4, 4))
    E = ng.pack([ng.replay(*n0), ng.replay(mkr.nested_map(), over[:4]), ng.replay(*n1)], A, caps, inner)
    assert max(ng.sizes(ng.replay(mkr.nested_map(), over))) == 5
    _capacity_check(gpu, S, [n0[1], over[:4], n1[1]], [n0[1], over, n1[1]], E, caps, inner)


def test_map_map_apply_capacity_intermediate_only(gpu):
    """Case (c) with four keys already there: the fresh key needs a fifth key
    slot although the same Up's deferred pass removes it again."""
    n0, n1 = _small_neighbours()
    start = mkr.nested_map()
    for k in range(4):
        mkr.apply_raw(start, _put((1, k + 1), 10 + k, 1, [(1, k + 1)], k))
    mkr.apply_raw(start, _rm(7, [(0, 1)]))
    op = _put((0, 1), 7, 2, [(0, 1)], 4)
    end = ng.replay(start, [op])
    assert len(start.entries) == 4 and len(end.entries) == 4 and not end.deferred
    S = ng.pack([n0[0], start, n1[0]], A, (4, 4, 4), (4, 4, 4, 4))
    caps, inner = (4, 8, 8), (8, 8, 8, 8)
    E = ng.pack([ng.replay(*n0), start, ng.replay(*n1)], A, caps, inner)
    _capacity_check(gpu, S, [n0[1], [], n1[1]], [n0[1], [op], n1[1]], E, caps, inner)
    E5 = ng.pack([ng.replay(*n0), end, ng.replay(*n1)], A, (5, 8, 8), inner)
    ng.assert_rows(_apply(gpu, S, [n0[1], [op], n1[1]], A, (5, 8, 8), inner), E5)


# ------------------------------------------------------------------ 9. errors
def _raw_ops(per_obj, **patch):
    import crdts_hip

    arrs = dict(zip(ng.OPS_FIELDS, crdts_hip.MapMapOps.arrays_from_lists(per_obj)))
    for k, v in patch.items():
        arrs[k] = np.asarray(v, dtype=arrs[k].dtype)
    return crdts_hip.MapMapOps.from_arrays(*(arrs[k] for k in ng.OPS_FIELDS))


GOOD = [_put((0, 1), 7, 3, [(0, 1)], 5)]
NONCANON = {
    "descending_clock_actors": lambda: _raw_ops([GOOD, [_rm(3, [(2, 1), (1, 1)])], GOOD]),
    "equal_clock_actors": lambda: _raw_ops([GOOD, [_irm((0, 1), 3, 4, [(2, 1), (2, 2)])], GOOD]),
    "zero_counter": lambda: _raw_ops([GOOD, [_rm(3, [(1, 0)])], GOOD]),
    "clock_actor_out_of_range": lambda: _raw_ops([GOOD, [_put((0, 1), 3, 4, [(A, 1)], 5)], GOOD]),
    "dot_actor_out_of_range": lambda: _raw_ops([GOOD, [_put((0, 1), 3, 4, [(0, 1)], 5)], GOOD], actor=[0, A, 0]),
    "inner_dot_actor_out_of_range": lambda: _raw_ops([GOOD, [_put((0, 1), 3, 4, [(0, 1)], 5)], GOOD],
                                                     actor2=[0, A, 0]),
    "up_nop_dot_actor_out_of_range": lambda: _raw_ops([GOOD, [{"up": {"dot": [A, 1], "key": 3, "op": "nop"}}], GOOD]),
    "kind_5": lambda: _raw_ops([GOOD, ["nop"], GOOD], kind=[2, 5, 2]),
    "decreasing_obj_end": lambda: _raw_ops([GOOD, GOOD, GOOD], obj_end=[2, 1, 3]),
    "obj_end_past_n_ops": lambda: _raw_ops([GOOD, GOOD, GOOD], obj_end=[1, 9, 3]),
    "clk_end_past_n_clk": lambda: _raw_ops([GOOD, GOOD, GOOD], clk_end=[1, 7, 3]),
    "decreasing_clk_end": lambda: _raw_ops([GOOD, GOOD, GOOD], clk_end=[1, 0, 3]),
}


@pytest.mark.parametrize("name", sorted(NONCANON))
def test_map_map_apply_noncanonical_ops(gpu, name):
    """A malformed op list latches CRDT_ENONCANON for its object; the first
    object of the batch, whose list is well formed, is exact."""
    import crdts_hip

    S = crdts_hip.MapMapSlab.alloc(3, A, *IN_CAPS, IN_INNER)
    E = ng.pack([ng.replay(mkr.nested_map(), GOOD)] + [mkr.nested_map()] * 2, A, ng.OUT_CAPS, ng.OUT_INNER)
    got = _apply(gpu, S, NONCANON[name](), A, check_status=False)
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    ng.assert_rows(got, E, rows=[0], what=name)
    gpu.status()


@pytest.mark.parametrize("where", ["outer_n_keys", "outer_dset_n", "inner_untouched", "inner_edited"])
def test_map_map_apply_noncanonical_input_row(gpu, where):
    """An input row the merge rejects: a count above its capacity, in the
    outer map, in an inner map no op touches (found when it is placed) and in
    one an op edits (found when it is copied to be edited). The neighbour is exact."""
    import crdts_hip

    good = ng.replay(mkr.nested_map(), GOOD)
    bad = ng.replay(good, [_rm(9, [(5, 5)])])  # one key, one outer deferred clock
    S = ng.pack([good, bad], A, IN_CAPS, IN_INNER)
    if where == "outer_n_keys":
        S.a["n_keys"][1] = IN_CAPS[0] + 1
    elif where == "outer_dset_n":
        S.a["dset_n"][1, 0] = IN_CAPS[2] + 1
    else:
        S.inner.a["mv_n"][1 * IN_CAPS[0] + 0, 0] = IN_INNER[1] + 1
    ops = [GOOD, [_put((1, 1), 7, 3, [(1, 1)], 6)] if where == "inner_edited" else []]
    E = ng.pack([good, good], A, ng.OUT_CAPS, ng.OUT_INNER)
    got = _apply(gpu, S, ops, A, check_status=False)
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    ng.assert_rows(got, E, rows=[0], what=where)
    gpu.status()


def test_map_map_apply_einval(gpu):
    import crdts_hip
    from crdts_hip._lib import MapMapOpsC, lib

    alloc = crdts_hip.MapMapSlab.alloc
    S = alloc(1, A, *IN_CAPS, IN_INNER, device="cuda")
    ops = crdts_hip.MapMapOps.from_lists([GOOD])
    O, I = ng.OUT_CAPS, ng.OUT_INNER
    bad = [dict(S=S, n_actors=129, out_caps=O, inner_out_caps=I),
           dict(S=S, n_actors=A, out_caps=(3, 8, 8), inner_out_caps=I),          # below self's, outer
           dict(S=S, n_actors=A, out_caps=(8, 7, 8), inner_out_caps=I),
           dict(S=S, n_actors=A, out_caps=O, inner_out_caps=(8, 7, 8, 8)),       # below self's, inner
           dict(S=S, n_actors=A, out_caps=O, inner_out_caps=(8, 8, 8, 3)),
           dict(S=S, n_actors=A, out_caps=(8, 129, 8), inner_out_caps=I),        # above twice the merge's limit
           dict(S=S, n_actors=A, out_caps=O, inner_out_caps=(8, 257, 8, 8)),
           dict(S=S, n_actors=A, out_caps=O, inner_out_caps=(8, 8, 129, 8)),
           dict(S=alloc(1, A, 4, 65, 4, IN_INNER, device="cuda"), n_actors=A, out_caps=(8, 65, 8), inner_out_caps=I),
           dict(S=alloc(1, A, *IN_CAPS, (4, 129, 8, 4), device="cuda"), n_actors=A, out_caps=O,
                inner_out_caps=(8, 129, 8, 8)),                                   # self past the merge's per-side limits
           dict(S=S, n_actors=A, out=S)]                                          # in place
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.map_map_apply(kw.pop("S"), ops, **kw)
        assert e.value.code == crdts_hip.CRDT_EINVAL, kw
    # through the C ABI: n_actors 0, null arguments, the scratch, a null op array
    R = alloc(1, A, *O, I, device="cuda")
    s, r, o = S.cstruct(), R.cstruct(), ops.cops()
    need = lib.crdt_map_map_apply_scratch_bytes(C.byref(r), 1, A)
    import torch

    sc = torch.empty(need + 32, dtype=torch.uint8, device="cuda")
    p = sc.data_ptr()
    assert p % 16 == 0
    call = lambda s_, o_, r_, A_, ptr, nb: lib.crdt_map_map_apply(gpu.ctx, s_, o_, r_, 1, A_, ptr, nb, None)  # noqa: E731
    assert call(C.byref(s), C.byref(o), C.byref(r), A, C.c_void_p(p), need) == crdts_hip.CRDT_OK
    gpu.status()
    hole = MapMapOpsC(*[getattr(o, f) for f in ng.OPS_FIELDS], o.n_ops, o.n_clk)
    hole.key2 = None
    for args in ((C.byref(s), C.byref(o), C.byref(r), 0, C.c_void_p(p), need),
                 (None, C.byref(o), C.byref(r), A, C.c_void_p(p), need),
                 (C.byref(s), None, C.byref(r), A, C.c_void_p(p), need),
                 (C.byref(s), C.byref(o), None, A, C.c_void_p(p), need),
                 (C.byref(s), C.byref(o), C.byref(r), A, None, need),
                 (C.byref(s), C.byref(o), C.byref(r), A, C.c_void_p(p), need - 1),
                 (C.byref(s), C.byref(o), C.byref(r), A, C.c_void_p(p + 8), need),
                 (C.byref(s), C.byref(hole), C.byref(r), A, C.c_void_p(p), need)):
        assert call(*args) == crdts_hip.CRDT_EINVAL
    gpu.status()
