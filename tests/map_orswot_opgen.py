"""Seeded generator of Map<u64, Orswot<u64, A>, A> op streams (Op::Up with an
Orswot Add or Rm / Op::Rm, src/map.rs:104-125) — test infrastructure for the
batched Map::apply with Orswot values (crdt_map_orswot_apply). Needs no GPU.

The scheme is tests/map_opgen.py's. Per object: three replicas of one map.
Replicas 1 and 2 author `n_ops` ops, each from the author's own `get(key)`
read context (src/map.rs:291-302):
  - 45 % Up{Add}: dot = add_clock.inc(actor), the nested Add carries the same
    dot (Map::update, src/map.rs:306-317);
  - 20 % Up{Rm}: the same kind of dot, the nested Rm's clock the member's
    `contains` rm-clock (30 % of them: the set's whole clock);
  - 35 % Rm with the entry clock (30 % of them: the whole map clock);
and after each op the two authors merge with probability 0.3. Replica 0 is
sent a random 70 % of the log, shuffled, 15 % of it repeated at the end: that
delivered sequence is the object's op stream. Odd objects fold the first third
of it into replica 0's initial state (`pre`); even objects start from the
empty map.

Authors use disjoint actors (map_opgen._pool: the boundary actors 0, 63, 64
and n_actors - 1 drawn often). Keys and members come from four fixed u64
values each, one of them above 2^63.

Op tuples (crdts_hip.MapOrswotOps): ("up_add", actor, counter, key, member),
("up_rm", actor, counter, key, member, pairs), ("rm", key, pairs), ("nop",).
"""
from __future__ import annotations

import random

from map_opgen import KEYS, _pairs, _pool
from map_slab import crdts_ref

MEMBERS = (2, 9, (1 << 33) + 7, (1 << 63) + 11)
CAP_NAMES = ("kcap", "mcap", "vdcap", "vscap", "dcap", "scap")


def caps(*v):
    """(kcap, mcap, vdcap, vscap, dcap, scap) or one value for all -> dict."""
    return dict(zip(CAP_NAMES, v if len(v) == 6 else v * 6))


def new_map(order=crdts_ref.clock_order):
    return crdts_ref.Map(crdts_ref.Orswot, order)


def apply_op(m, op):
    """One generated op on a crdts_ref.Map of Orswot values."""
    if op[0] == "up_add":
        _, actor, counter, key, member = op
        m.apply_up((actor, counter), key, lambda o: o.apply_add((actor, counter), member))
    elif op[0] == "up_rm":
        _, actor, counter, key, member, pairs = op
        m.apply_up((actor, counter), key, lambda o: o.apply_rm(crdts_ref.VClock(pairs), member))
    elif op[0] == "rm":
        m.apply_rm(op[1], crdts_ref.VClock(op[2]))
    elif op[0] != "nop":
        raise ValueError(op[0])


def apply_op_oracle(h, op):
    """The same op on an oracle_ffi.OracleMap("orswot") handle."""
    if op[0] == "up_add":
        h.apply_up_orswot((op[1], op[2]), op[3], 0, op[4])
    elif op[0] == "up_rm":
        h.apply_up_orswot((op[1], op[2]), op[3], 1, op[4], op[5])
    elif op[0] == "rm":
        h.apply_rm(op[1], op[2])
    elif op[0] != "nop":
        raise ValueError(op[0])


def op_clock(op):
    return op[5] if op[0] == "up_rm" else op[2] if op[0] == "rm" else []


def gen_object(rng, A, keys=KEYS, members=MEMBERS, n_ops=12, fold=False):
    """-> (pre, ops): `pre` the ops folded into replica 0's initial state (empty
    unless `fold`), `ops` the stream to apply to it."""
    reps = [None, new_map(), new_map()]
    pools = [None, _pool(rng, A, 0), _pool(rng, A, 1 if A > 1 else 0)]
    log = []
    for _ in range(n_ops):
        r = rng.choice((1, 2))
        m = reps[r]
        key = rng.choice(keys)
        add, rmc, val = m.get(key)
        x = rng.random()
        if x < 0.65:
            actor = rng.choice(pools[r])
            counter = add.get(actor) + 1
            member = rng.choice(members)
            if x < 0.45:
                op = ("up_add", actor, counter, key, member)
            else:
                o = val if val is not None else crdts_ref.Orswot()
                c = o.read_add_clock() if rng.random() < 0.3 else o.contains_rm_clock(member)
                op = ("up_rm", actor, counter, key, member, _pairs(c))
        else:
            op = ("rm", key, _pairs(add if rng.random() < 0.3 else rmc))
        apply_op(m, op)
        log.append(op)
        if rng.random() < 0.3:
            reps[1].merge(reps[2])
            reps[2].merge(reps[1])
    sent = [op for op in log if rng.random() < 0.7]
    rng.shuffle(sent)
    sent += [op for op in sent if rng.random() < 0.15]
    cut = len(sent) // 3 if fold else 0
    return sent[:cut], sent[cut:]


def gen_batch(seed, n, A, keys=KEYS, members=MEMBERS, n_ops=12):
    """n objects: [(pre, ops), ...] (odd objects folded, see the module docstring)."""
    rng = random.Random(seed)
    return [gen_object(rng, A, keys, members, n_ops, fold=bool(i & 1)) for i in range(n)]


def oracle_slabs(oracle, batch, A, self_caps, out_caps):
    """-> (S, E), host crdts_hip.MapOrswotSlabs: row i of S is replica 0 after
    object i's `pre`, row i of E the same map after its whole stream — both by
    the C++ oracle's handles (oracle_ffi.OracleMap("orswot"))."""
    import ctypes as C

    import crdts_hip

    S = crdts_hip.MapOrswotSlab.alloc(len(batch), A, **self_caps)
    E = crdts_hip.MapOrswotSlab.alloc(len(batch), A, **out_caps)
    s, e, L = S.cstruct(), E.cstruct(), oracle.lib()
    for i, (pre, ops) in enumerate(batch):
        h = oracle.OracleMap("orswot")
        for op in pre:
            apply_op_oracle(h, op)
        assert L.orc_mapor_to_slab(h.h, C.byref(s), i, A) == 0, f"object {i}: self capacity"
        for op in ops:
            apply_op_oracle(h, op)
        assert L.orc_mapor_to_slab(h.h, C.byref(e), i, A) == 0, f"object {i}: out capacity"
    return S, E


def oracle_from_row(oracle, S, i, A):
    """An oracle handle holding row i of a host MapOrswotSlab."""
    import ctypes as C

    s = S.cstruct()
    return oracle.OracleMap("orswot", oracle.lib().orc_mapor_from_slab(C.byref(s), i, A))


# ---- the hand-built cases: (a) a nested Rm that leaves a smaller non-empty
# member clock, (b) a nested duplicate dot under a fresh map dot, (c) a stream
# whose result depends on apply_deferred's order; A >= 3
CASE_A = [("up_add", 0, 1, 7, 1), ("up_add", 1, 1, 7, 1), ("up_rm", 0, 2, 7, 1, [(0, 1)])]
CASE_B_OP = ("up_add", 2, 5, 7, 4)
CASE_C = [("up_rm", 1, 2, 7, 2, [(0, 1), (2, 2)]), ("rm", 7, [(2, 6)]), ("up_rm", 1, 3, 7, 1, [(1, 6)]),
          ("rm", 7, [(0, 6), (2, 1)]), ("up_add", 0, 2, 7, 2)]


def case_b_map():
    """A row no op stream from the empty map reaches: key 7's set has seen
    actor 2 up to 9, the map clock only up to 3."""
    m = new_map()
    m.clock = crdts_ref.VClock([(0, 2), (2, 3)])
    o = crdts_ref.Orswot()
    o.clock = crdts_ref.VClock([(0, 2), (2, 9)])
    o.entries[4] = crdts_ref.VClock([(2, 9)])
    o.entries[6] = crdts_ref.VClock([(0, 2)])
    m.entries[7] = [crdts_ref.VClock([(0, 2), (2, 3)]), o]
    m.deferred[crdts_ref.VClock([(1, 4)])] = {7}      # stays deferred
    m.deferred[crdts_ref.VClock([(2, 5)])] = {7, 8}   # retired by the Up's deferred pass
    return m
