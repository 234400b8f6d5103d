"""The structured Orswot generator (tests/orswot_pairgen.py) earns its place
without a GPU: at every shape the GPU edge tests use (tests/
test_gpu_orswot_edges.py) the plain-Python restatements of merge, truncate
and apply (pg.merge_ref / truncate_ref / apply_ref) equal the C++ oracle and
oracle/crdts_ref.py byte-for-byte, every deliberately wrong variant of them
(pg.MUTANTS / TRUNCATE_MUTANTS / APPLY_MUTANTS) changes the output of at
least 20 objects of the batch in both orientations, the batch holds the
intended number of objects per launch tier, and the forced objects, the edge
counters and keys and the hot actor ids all occur. As a contrast, the
low-32-bit and the signed counter compare are invisible to the inputs the
suite had before: tests/truncate_cases.py states and config-3 pairs rebuilt
from the gen_pair recipe (one shared 40-bit base per actor)."""
import collections
import random

import pytest

import crdts_ref
import orswot_pairgen as pg
from orswot_edge_cases import (FLOOR, apply_case, assert_apply_workspaces, assert_merge_tiers, assert_truncate_forms,
                               merge_case, truncate_case)
import records
import truncate_cases as T

HEAVY = 5000  # members: larger objects are left out of the mutant counts (time)


def _ref_merge(L, R, A, sparse):
    a, b = T.to_ref(L), T.to_ref(R)
    a.merge(b)
    return records.from_py(a, A, sparse)


def _light(pairs):
    return [i for i, p in enumerate(pairs) if len(p[0][1]) + len(p[1][1]) <= HEAVY]


# ------------------------------------------------------------------ merge
@pytest.mark.parametrize("name", sorted(pg.MERGE_SHAPES))
def test_merge_tiers(name):
    """Every labelled object takes the tier its label names, and the batch
    holds the shape's number of objects of every tier (pg.SHAPE_TIERS)."""
    A, sparse, pairs, labels, Ls, Rs, _, _ = merge_case(name)
    print(name, sorted(assert_merge_tiers(name).items()))
    assert [lab for lab in labels[:pg.N_FORCED]] == ["forced"] * pg.N_FORCED
    for lab in set(labels) - {"forced"}:
        assert pg.LABEL_TIERS[lab] is not None


def test_limit_objects_are_what_they_say():
    """The A16_limits labels: unions of exactly 64 / 65 members; records of
    exactly 2 048 / 2 064 bytes; 31 / 32 / 33 deferred clocks on the self side
    whose last clock in CLOCK ORDER names a present member and covers its dot."""
    A, sparse, pairs, labels, Ls, Rs, _, _ = merge_case("A16_limits")
    seen = collections.Counter()
    for (L, R), lab, l in zip(pairs, labels, Ls):
        seen[lab] += 1
        if lab.startswith("union"):
            assert len(set(L[1]) | set(R[1])) == int(lab[5:]) and max(len(L[1]), len(R[1])) <= 64
        if lab.startswith("size"):
            assert len(l) == int(lab[4:])
        if lab.startswith("ndef"):
            assert len(L[2]) == int(lab[4:])
            last = max(L[2])
            (m,) = L[2][last]
            sides = (L[1].get(m, {}), R[1].get(m, {}))
            assert any(a in dots and c >= dots[a] for dots in sides for a, c in last), (last, sides)
    assert all(seen[lab] >= 30 for lab in pg.LABEL_TIERS if lab[:4] in ("unio", "size", "ndef")), seen


@pytest.mark.parametrize("name", sorted(pg.MERGE_SHAPES))
def test_merge_references_agree(name):
    """pg.merge_ref with the right knobs == crdts_ref.Orswot.merge == the C++
    oracle, byte-for-byte, in both orientations; most outputs differ from self."""
    A, sparse, pairs, labels, Ls, Rs, lr, rl = merge_case(name)
    moved = 0
    for i, (L, R) in enumerate(pairs):
        for x, y, xr, exp in ((L, R, Ls[i], lr[i]), (R, L, Rs[i], rl[i])):
            assert pg.encode(pg.as_state(pg.merge_ref(x, y)), A, sparse) == exp, (name, i, labels[i])
            if len(x[1]) + len(y[1]) <= HEAVY:
                assert _ref_merge(x, y, A, sparse) == exp, (name, i, labels[i])
            moved += exp != xr
    assert moved >= 1.5 * len(pairs), moved


@pytest.mark.parametrize("mutant", sorted(pg.MUTANTS))
@pytest.mark.parametrize("name", sorted(pg.MERGE_SHAPES))
def test_wrong_merges_differ(name, mutant):
    """A merge that is wrong in one way changes the output of >= 20 objects of
    this very batch, in both orientations: a condition on the inputs, checked
    against the references alone."""
    A, sparse, pairs, labels, Ls, Rs, lr, rl = merge_case(name)
    knobs = pg.MUTANTS[mutant]
    counts = []
    for side, exp in ((0, lr), (1, rl)):
        counts.append(sum(pg.as_shape(pg.merge_ref(pairs[i][side], pairs[i][1 - side], **knobs)) != pg.shape_of(exp[i])
                          for i in _light(pairs)))
    print(f"{name:12s} {mutant:24s} objects changed: self-other {counts[0]:4d}, other-self {counts[1]:4d} "
          f"of {len(pairs)}")
    assert min(counts) >= FLOOR, (name, mutant, counts)


@pytest.mark.parametrize("name", sorted(pg.MERGE_SHAPES))
def test_forced_objects_edges_and_hot_actors_occur(name):
    A, sparse, pairs, labels, Ls, Rs, lr, rl = merge_case(name)
    L, R = [p[0] for p in pairs], [p[1] for p in pairs]
    assert L[0] == R[0] == pg.EMPTY and L[1] == pg.EMPTY != R[1] and R[2] == pg.EMPTY != L[2] and L[3] == R[3]
    assert list(L[4][1]) == [pg.M64] and list(R[5][1]) == [pg.M64]
    assert list(L[6][1]) == [0] and not R[6][1] and A - 1 not in R[6][0] and (L[7], R[7]) == (R[6], L[6])
    ctrs, keys, dot_actors, def_actors = set(), set(), set(), set()
    for s in L + R:
        ctrs.update(s[0].values())
        keys.update(s[1])
        for d in s[1].values():
            ctrs.update(d.values())
            dot_actors.update(d)
        for dk, ms in s[2].items():
            keys.update(ms)
            ctrs.update(c for _, c in dk)
            def_actors.update(a for a, _ in dk)
    assert set(pg.EDGE) <= ctrs and set(pg.KEYS) <= keys
    assert set(pg.hot(A)) <= dot_actors and set(pg.hot(A)) <= def_actors
    ks = sorted(keys)
    assert any(x ^ y < 2**32 for x, y in zip(ks, ks[1:])), "keys that differ only in the low word"
    hi = collections.Counter(k & pg.M32 for k in ks)
    assert max(hi.values()) > 1, "keys that differ only in the high word"


# ------------------------------------------------------------------ the gap, pinned
def _config3_like(rng, A=16, universe=64, ancestor_adds=32):
    """One config-3 pair by the gen_pair recipe (csrc/host.cpp): a shared
    ancestor, then 4-16 divergent ops a side; every counter is its actor's
    shared 40-bit base plus a small count."""
    keys = [rng.getrandbits(64) for _ in range(universe)]
    base = [rng.getrandbits(40) for _ in range(A)]
    nxt = lambda o, a: max(o.clock.get(a), base[a]) + 1  # noqa: E731
    anc = crdts_ref.Orswot()
    for k in rng.sample(range(universe), ancestor_adds):
        a = rng.randrange(A)
        anc.apply_add((a, nxt(anc, a)), keys[k])
    out = []
    for side in range(2):
        o = anc.clone()
        own = range(0, A // 2) if side == 0 else range(A // 2, A)
        oth = range(A // 2, A) if side == 0 else range(0, A // 2)
        for _ in range(rng.randint(4, 16)):
            r = rng.randrange(100)
            if r < 60:
                a = rng.choice(own)
                o.apply_add((a, nxt(o, a)), rng.choice(keys))
            elif r >= 90:
                c = o.clock.clone()
                x = rng.choice(oth)
                c.witness(x, max(c.get(x), base[x]) + 1 + rng.randrange(3))
                o.apply_rm(c, rng.choice(keys))
            elif o.entries:
                m = rng.choice(sorted(o.entries))
                o.apply_rm(o.entries[m].clone(), m)
        out.append(T.ref_state(o))
    return tuple((c, {m: dict(d) for m, d in e.items()}, {k: set(v) for k, v in d}) for c, e, d in out)


@pytest.mark.parametrize("mutant", ["counter_compare_low32", "counter_compare_signed"])
def test_old_style_inputs_cannot_see_the_value_mutants(mutant):
    """2 000 states shaped like truncate_cases.cases (merged pairwise, and
    truncated by their clocks) and 2 000 config-3-like pairs: a join that
    compares the low 32 bits, or compares signed, agrees with the right one on
    >= 99 % of them. The edge generator exists to close this gap."""
    knobs = pg.MUTANTS[mutant]
    states, clocks, _ = T.cases(2000)
    rng = random.Random(3)
    c3 = [_config3_like(rng) for _ in range(2000)]
    same = {
        "truncate_cases merge": sum(pg.as_shape(pg.merge_ref(a, b, **knobs)) == pg.as_shape(pg.merge_ref(a, b))
                                    for a, b in zip(states, states[1:] + states[:1])),
        "truncate_cases truncate": sum(pg.truncate_ref(s, c, **knobs) == pg.truncate_ref(s, c)
                                       for s, c in zip(states, clocks)),
        "config 3 merge": sum(pg.as_shape(pg.merge_ref(a, b, **knobs)) == pg.as_shape(pg.merge_ref(a, b)) and
                              pg.as_shape(pg.merge_ref(b, a, **knobs)) == pg.as_shape(pg.merge_ref(b, a))
                              for a, b in c3),
    }
    print(mutant, same)
    assert all(v >= 0.99 * 2000 for v in same.values()), same
    assert sum(bool(a[2]) for a, _ in c3) > 50 and sum(bool(a[1]) for a, _ in c3) > 1900


# ------------------------------------------------------------------ truncate
def _trunc_shape(res):
    clock, out, deferred = res
    return clock, [(m, sorted(d.items())) for m, d in out], [(dk, sorted(deferred[dk])) for dk in sorted(deferred)]


@pytest.mark.parametrize("name", sorted(pg.TRUNCATE_SHAPES))
def test_truncate_references_agree_and_forms(name):
    """pg.truncate_ref == crdts_ref.Orswot.truncate == the C++ oracle,
    byte-for-byte; the batch holds the shape's number of records of every
    kernel form (the fast form with exactly 1 and exactly 8 deferred clocks)
    and every edge counter and key; members left with an EMPTY clock occur."""
    A, sparse, states, clocks, recs, exp = truncate_case(name)
    print(name, sorted(assert_truncate_forms(name).items()))
    empties = 0
    for i, (S, c) in enumerate(zip(states, clocks)):
        clock, out, deferred = pg.truncate_ref(S, c)
        assert pg.encode((clock, dict((m, d) for m, d in out), deferred), A, sparse) == exp[i], (name, i)
        o = T.to_ref(S)
        o.truncate(crdts_ref.VClock(c))
        rc, re, rd = T.ref_state(o)
        assert (rc, {m: dict(d) for m, d in re.items()}, {k: set(v) for k, v in rd}) == \
            (clock, dict((m, d) for m, d in out), deferred), (name, i)
        empties += any(not d for _, d in out)
    assert empties >= FLOOR, empties
    if name == "long_run_A128":
        assert sum(len(c) > 64 and any(a in S[0] for a in sorted(c)[64:]) for S, c in zip(states, clocks)) >= 200


@pytest.mark.parametrize("mutant", sorted(pg.TRUNCATE_MUTANTS))
@pytest.mark.parametrize("name", sorted(pg.TRUNCATE_SHAPES))
def test_wrong_truncates_differ(name, mutant):
    A, sparse, states, clocks, recs, exp = truncate_case(name)
    knobs = pg.TRUNCATE_MUTANTS[mutant]
    n = sum(_trunc_shape(pg.truncate_ref(S, c, **knobs)) != pg.shape_of(e) for S, c, e in zip(states, clocks, exp))
    print(f"{name:14s} {mutant:24s} records changed: {n:4d} of {len(states)}")
    assert n >= FLOOR, (name, mutant, n)


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("name", sorted(pg.APPLY_SHAPES))
def test_apply_references_agree(name):
    """pg.apply_ref == crdts_ref's op path == the C++ oracle's, byte-for-byte;
    stale Adds at exactly the top counter, Adds at 2^64 - 1, removes left
    deferred and deferred removes released by a later Add all occur, as do
    the shape's small- and large-workspace states and every edge counter and key."""
    A, sparse, states, ops, recs, exp = apply_case(name)
    print(name, "small workspace, > 64 members, > 16 deferred clocks:", assert_apply_workspaces(name))
    seen = collections.Counter()
    for i, (S, per) in enumerate(zip(states, ops)):
        assert pg.encode(pg.as_state(pg.apply_ref(S, per)), A, sparse) == exp[i], (name, i, per)
        o = T.to_ref(S)
        n_def = len(o.deferred)
        for op in per:
            if op[0] == "add":
                seen["stale_at_top"] += o.clock.get(op[1]) == op[2]
                seen["add_at_max"] += op[2] == pg.M64
                o.apply_add((op[1], op[2]), op[3])
                seen["released"] += len(o.deferred) < n_def
            else:
                ctx = crdts_ref.VClock(op[2])
                seen["rm_exact_clock"] += op[1] in o.entries and o.entries[op[1]] == ctx
                o.apply_rm(ctx, op[1])
                seen["deferred"] += len(o.deferred) > n_def
            n_def = len(o.deferred)
        assert records.from_py(o, A, sparse) == exp[i], (name, i, per)
    print(name, dict(seen))
    assert all(seen[k] >= FLOOR for k in ("stale_at_top", "add_at_max", "released", "rm_exact_clock", "deferred")), seen
    assert sorted(pg.state_of(exp[0])[1]) == [0] and sorted(pg.state_of(exp[1])[1]) == [pg.M64 - 1, pg.M64]
    assert not pg.state_of(exp[1])[2] and exp[2] == recs[2]


@pytest.mark.parametrize("mutant", sorted(pg.APPLY_MUTANTS))
@pytest.mark.parametrize("name", sorted(pg.APPLY_SHAPES))
def test_wrong_applies_differ(name, mutant):
    A, sparse, states, ops, recs, exp = apply_case(name)
    knobs = pg.APPLY_MUTANTS[mutant]
    n = sum(pg.as_shape(pg.apply_ref(S, per, **knobs)) != pg.shape_of(e) for S, per, e in zip(states, ops, exp))
    print(f"{name:6s} {mutant:24s} records changed: {n:4d} of {len(states)}")
    assert n >= FLOOR, (name, mutant, n)
