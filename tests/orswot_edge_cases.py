"""Test helper: the batches of tests/orswot_pairgen.py as records with the C++
oracle's answers, made once and shared (read-only) by the CPU proof
(tests/test_orswot_pairgen.py) and the GPU parity tests
(tests/test_gpu_orswot_edges.py), plus the counts both of them assert on the
truncate and apply batches."""
import collections
import functools

import oracle_ffi
import orswot_pairgen as pg
import records
import truncate_cases as T

FLOOR = 20  # the fewest objects of a batch that must show each property


@functools.lru_cache(maxsize=None)
def merge_case(name):
    """-> (A, sparse, pairs, labels, L records, R records, oracle L ⊔ R, oracle R ⊔ L)."""
    A, sparse, pairs, labels = pg.merge_batch(name)
    Ls = [pg.encode(p[0], A, sparse) for p in pairs]
    Rs = [pg.encode(p[1], A, sparse) for p in pairs]
    lb, lo = records.pack_batch(Ls)
    rb, ro = records.pack_batch(Rs)
    lr = records.unpack_batch(*oracle_ffi.orswot_merge_batch(lb, lo, rb, ro, A, threads=16, flags=int(sparse)))
    rl = records.unpack_batch(*oracle_ffi.orswot_merge_batch(rb, ro, lb, lo, A, threads=16, flags=int(sparse)))
    return A, sparse, pairs, labels, Ls, Rs, lr, rl


def assert_merge_tiers(name):
    """Every labelled object takes a tier its label names and the batch holds
    the shape's number of objects of every tier, in both orientations -> the
    counts per (label, tier)."""
    A, sparse, pairs, labels, Ls, Rs, _, _ = merge_case(name)
    counts = pg.check_tiers(A, sparse, Ls, Rs, labels)
    for a, b in ((Ls, Rs), (Rs, Ls)):
        per = pg.tiers(A, a, b, sparse)
        assert all(per.get(t, 0) >= k for t, k in pg.SHAPE_TIERS[name].items()), (name, per)
    return counts


def _values(states):
    """The counters and member keys a list of states holds."""
    ctrs, keys = set(), set()
    for clock, entries, deferred in states:
        ctrs.update(clock.values())
        keys.update(entries)
        for d in entries.values():
            ctrs.update(d.values())
        for dk, ms in deferred.items():
            keys.update(ms)
            ctrs.update(c for _, c in dk)
    return ctrs, keys


@functools.lru_cache(maxsize=None)
def truncate_case(name):
    """-> (A, sparse, states, truncating clocks, records, the oracle's truncated records)."""
    A, sparse, states, clocks = pg.truncate_batch(name)
    recs = [pg.encode(s, A, sparse) for s in states]
    lb, lo = records.pack_batch(recs)
    exp = records.unpack_batch(*oracle_ffi.orswot_truncate_batch(lb, lo, T.clocks_csr(clocks), A, int(sparse),
                                                                 threads=16))
    return A, sparse, states, clocks, recs, exp


def assert_truncate_forms(name):
    """The batch holds the shape's number of records of every kernel form
    (a fast-form shape: also records with exactly 1 and exactly 8 deferred
    clocks), and every edge counter and key occurs in it -> the form counts."""
    A, sparse, states, clocks, recs, _ = truncate_case(name)
    forms = collections.Counter(pg.truncate_form(A, r, sparse) for r in recs)
    assert all(forms[f] >= k for f, k in pg.TRUNCATE_FORMS[name].items()), forms
    if name.startswith("fast"):
        n_def = collections.Counter(len(s[2]) for s, r in zip(states, recs) if pg.truncate_form(A, r, sparse) == "fast")
        assert n_def[1] >= FLOOR and n_def[8] >= FLOOR and all(n_def[k] for k in range(1, 9)), n_def
    ctrs, keys = _values(states)
    assert set(pg.EDGE) <= ctrs and set(pg.EDGE) <= {c for clock in clocks for c in clock.values()}, name
    assert set(pg.KEYS) <= keys, name
    return forms


def oracle_apply(rec, ops, A, flags):
    o = oracle_ffi.OracleOrswot.decode(rec)
    for op in ops:
        if op[0] == "add":
            o.apply_add(op[1], op[2], op[3])
        else:
            o.apply_rm(op[1], op[2])
    return o.encode(A, flags)


@functools.lru_cache(maxsize=None)
def apply_case(name):
    """-> (A, sparse, states, op lists, records, the oracle's records after the ops)."""
    A, sparse, states, ops = pg.apply_batch(name)
    recs = [pg.encode(s, A, sparse) for s in states]
    exp = [oracle_apply(r, o, A, int(sparse)) for r, o in zip(recs, ops)]
    return A, sparse, states, ops, recs, exp


# shape -> the fewest states that start in the small workspace (<= 40 members, <= 2 deferred clocks), past its 64
# members and past its 16 deferred clocks (test_apply_workspace_tiers; the A64 shape is small-workspace only)
APPLY_WORKSPACES = {"A16": (200, 50, 30), "A64": (200, 0, 0), "csr": (200, 50, 0)}


def assert_apply_workspaces(name):
    """The batch holds the shape's number of small- and large-workspace
    states, and every edge counter and key occurs in its states and ops."""
    A, sparse, states, ops, _, _ = apply_case(name)
    small, members, deferred = APPLY_WORKSPACES[name]
    got = (sum(len(s[1]) <= 40 and len(s[2]) <= 2 for s in states), sum(len(s[1]) > 64 for s in states),
           sum(len(s[2]) > 16 for s in states))
    assert got[0] >= small and got[1] >= members and got[2] >= deferred, (name, got)
    ctrs, keys = _values(states)
    for per in ops:
        for op in per:
            keys.add(op[3] if op[0] == "add" else op[1])
            ctrs.update([op[2]] if op[0] == "add" else [c for _, c in op[2]])
    assert set(pg.EDGE) <= ctrs and set(pg.KEYS) <= keys, name
    return got
