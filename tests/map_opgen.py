"""Seeded generator of Map<u64, MVReg<u64, A>, A> op streams (Op::Up with an
MVReg Put / Op::Rm, src/map.rs:104-125) — test infrastructure for the batched
Map::apply (crdt_map_mvreg_apply). Needs no GPU.

Per object: three replicas of one map. Replicas 1 and 2 author `n_ops` ops,
each from the author's own `get(key)` read context (src/map.rs:291-302):
  - 60 % Up: dot = add_clock.inc(actor), Put clock = add_clock + dot (5 % of
    the Ups carry an empty Put clock);
  - 40 % Rm with the entry clock (30 % of them: the whole map clock);
and after each op the two authors merge with probability 0.3. Replica 0 is
sent a random 70 % of the log, shuffled, 15 % of it repeated at the end: that
delivered sequence is the object's op stream. Odd objects fold the first third
of it into replica 0's initial state (`pre`), so that half of the batch starts
from a non-empty map; even objects start from the empty map.

Authors use disjoint actors (replica r: a small per-object pool of actors of
parity r - 1, the boundary actors 0, 63, 64 and n_actors - 1 drawn often), so
no two ops share a dot unless one is a redelivery. Keys come from four fixed
u64 values, one of them above 2^63.
"""
from __future__ import annotations

import random

from map_slab import crdts_ref

KEYS = (3, 17, (1 << 40) + 1, (1 << 63) + 5)


def _pairs(clock):
    return sorted(clock.dots.items())


def apply_op(m, op):
    """One generated op on a crdts_ref.Map of MVReg values."""
    if op[0] == "up":
        _, actor, counter, key, pairs, val = op
        m.apply_up((actor, counter), key, lambda r: r.apply_put(crdts_ref.VClock(pairs), val))
    elif op[0] == "rm":
        m.apply_rm(op[1], crdts_ref.VClock(op[2]))
    elif op[0] != "nop":
        raise ValueError(op[0])


def apply_op_oracle(h, op):
    """The same op on an oracle_ffi.OracleMap("mvreg") handle."""
    if op[0] == "up":
        _, actor, counter, key, pairs, val = op
        h.apply_up_mvreg((actor, counter), key, pairs, val)
    elif op[0] == "rm":
        h.apply_rm(op[1], op[2])
    elif op[0] != "nop":
        raise ValueError(op[0])


def _pool(rng, A, parity):
    own = [a for a in range(A) if a % 2 == parity] or [0]
    pool = set(rng.sample(own, min(3, len(own))))
    for b in (0, 63, 64, A - 1):
        if 0 <= b < A and b % 2 == parity and rng.random() < 0.5:
            pool.add(b)
    return sorted(pool)


def gen_object(rng, A, keys=KEYS, n_ops=12, fold=False, val0=1):
    """-> (pre, ops): `pre` the ops folded into replica 0's initial state (empty
    unless `fold`), `ops` the stream to apply to it."""
    reps = [None, crdts_ref.Map(crdts_ref.MVReg), crdts_ref.Map(crdts_ref.MVReg)]
    pools = [None, _pool(rng, A, 0), _pool(rng, A, 1 if A > 1 else 0)]
    log = []
    for t in range(n_ops):
        r = rng.choice((1, 2))
        m = reps[r]
        key = rng.choice(keys)
        add, rmc, _ = m.get(key)
        if rng.random() < 0.6:
            actor = rng.choice(pools[r])
            counter = add.get(actor) + 1
            put = add.clone()
            put.witness(actor, counter)
            op = ("up", actor, counter, key, [] if rng.random() < 0.05 else _pairs(put), val0 + t)
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


def oracle_slabs(oracle, batch, A, self_caps, out_caps):
    """-> (S, E), host crdts_hip.MapSlabs: row i of S is replica 0 after object
    i's `pre`, row i of E the same map after its whole stream — both by the C++
    oracle's handles (oracle_ffi.OracleMap("mvreg"))."""
    import ctypes as C

    import crdts_hip

    S = crdts_hip.MapSlab.alloc(len(batch), A, *self_caps)
    E = crdts_hip.MapSlab.alloc(len(batch), A, *out_caps)
    s, e, L = S.cstruct(), E.cstruct(), oracle.lib()
    for i, (pre, ops) in enumerate(batch):
        h = oracle.OracleMap("mvreg")
        for op in pre:
            apply_op_oracle(h, op)
        assert L.orc_mapmv_to_slab(h.h, C.byref(s), i, A) == 0, f"object {i}: self capacity"
        for op in ops:
            apply_op_oracle(h, op)
        assert L.orc_mapmv_to_slab(h.h, C.byref(e), i, A) == 0, f"object {i}: out capacity"
    return S, E


def gen_batch(seed, n, A, keys=KEYS, n_ops=12):
    """n objects: [(pre, ops), ...] (odd objects folded, see the module docstring)."""
    rng = random.Random(seed)
    return [gen_object(rng, A, keys, n_ops, fold=bool(i & 1), val0=1 + 100 * i) for i in range(n)]
