"""CPU reference of the batched read path (crdt_orswot_read*, crdt_map_read*,
crdt_map_mvreg_get; include/crdts_hip.h "Batched read path") over the
pure-Python restatement (oracle/crdts_ref.py) — test infrastructure.

A query is a tuple as crdts_hip.ReadQueries.from_lists takes it:
("key", k[, actor]) = Orswot::contains(k) / Map::get(k), ("all"[, actor]) =
Orswot::value() / Map::len(). The answer is a dict:
  val      1 / 0 (key), the number of members / entries (all)
  slot     the key's index among the ascending members / keys, else NO_SLOT
  dot_ctr  derive_add_ctx(actor).dot.counter (src/ctx.rs:45-55 over
           VClock::inc, src/vclock.rs:182-185); 0 without a usable actor
  add      AddCtx.clock as sorted pairs: add_clock with the dot witnessed
           (the add_clock itself without a usable actor)
  rm       derive_rm_ctx().clock (src/ctx.rs:57-60) as sorted pairs
  list     the members / keys ascending (all), [] (key)
  err      True where the call latches CRDT_ENONCANON for the query: an actor
           >= n_actors, or one whose counter is 2^64 - 1 (inc overflows)
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import crdts_ref  # noqa: E402

NO_SLOT = 0xFFFFFFFF
NO_ACTOR = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1


def pairs(clock):
    return sorted(clock.dots.items())


def _actor_of(q):
    a = (q[2] if len(q) > 2 else None) if q[0] == "key" else (q[1] if len(q) > 1 else None)
    return None if a is None or a == NO_ACTOR else a


def _answer(q, n_actors, add_clock, keys, rm_of_key):
    """keys: the ascending members / keys; rm_of_key(k) -> VClock of a present key."""
    out = dict(dot_ctr=0, err=False)
    if q[0] == "key":
        present = q[1] in keys
        out.update(val=int(present), slot=keys.index(q[1]) if present else NO_SLOT, list=[],
                   rm=pairs(rm_of_key(q[1])) if present else [])
    else:
        out.update(val=len(keys), slot=NO_SLOT, list=list(keys), rm=pairs(add_clock))
    add = add_clock.clone()
    a = _actor_of(q)
    if a is not None:
        if a >= n_actors or add.get(a) == U64_MAX:
            out["err"] = True
        else:
            dot = add.inc(a)
            add.apply(dot)
            out["dot_ctr"] = dot[1]
    out["add"] = pairs(add)
    return out


def orswot_query(o, q, n_actors):
    """One query on a crdts_ref.Orswot: contains (src/orswot.rs:214-224) / value (:227-233)."""
    return _answer(q, n_actors, o.read_add_clock(), sorted(o.value()), o.contains_rm_clock)


def map_query(m, q, n_actors):
    """One query on a crdts_ref.Map: get (src/map.rs:291-302) / len (:282-288)."""
    return _answer(q, n_actors, m.clock, sorted(m.entries), lambda k: m.get(k)[1])


def expect(objs, per_obj, n_actors, query=orswot_query):
    """The flat answers of a query batch, in query order."""
    return [query(o, q, n_actors) for o, qs in zip(objs, per_obj) for q in qs]


def mvreg_get(m, q):
    """The val of Map::get for Map<u64, MVReg>: [(clock pairs, value), ...] in Vec order
    ([] for an absent key, an entry without values and an `all` query)."""
    if q[0] != "key" or q[1] not in m.entries:
        return []
    return [(pairs(c), v) for c, v in m.entries[q[1]][1].vals]


def answers(res, n_q):
    """The dict of device tensors Engine.orswot_read / map_read return -> one
    answer dict per query, holding the fields that were wanted."""
    import numpy as np

    h = {k: v.cpu().numpy() for k, v in res.items()}
    u = lambda k, dt: h[k].view(dt).tolist()  # noqa: E731
    out = [dict() for _ in range(n_q)]
    for name, key, dt in (("val", "val", np.uint64), ("slot", "slot", np.uint32), ("dot_ctr", "dot_ctr", np.uint64)):
        if key in h:
            for a, x in zip(out, u(key, dt)):
                a[name] = x
    for g in ("add", "rm"):
        if g + "_end" in h:
            end, act, ctr = u(g + "_end", np.uint64), u(g + "_act", np.uint32), u(g + "_ctr", np.uint64)
            lens = u(g + "_len", np.uint32)
            for j, a in enumerate(out):
                b = end[j - 1] if j else 0
                assert end[j] - b == lens[j], f"query {j}: {g}_end does not follow {g}_len"
                a[g] = list(zip(act[b:end[j]], ctr[b:end[j]]))
    if "list_end" in h:
        end, keys, lens = u("list_end", np.uint64), u("list_key", np.uint64), u("list_len", np.uint32)
        for j, a in enumerate(out):
            b = end[j - 1] if j else 0
            assert end[j] - b == lens[j]
            a["list"] = keys[b:end[j]]
    return out


def assert_answers(got, exp, what=""):
    """Every field the call was asked for equals the reference's, query by query."""
    assert len(got) == len(exp), what
    for j, (g, e) in enumerate(zip(got, exp)):
        for k, v in g.items():
            assert v == e[k], f"{what} query {j} {k}: got {v}, expected {e[k]}"


class RefReadBackend:
    """Mixin for the KAT backends of tests/kat_runner.py: clock(), entry() and
    value() answered through a `_read(o, queries) -> [answer]` hook, so the
    reference's ctx asserts check the read path under test."""

    reads = 0

    def clock(self, o):
        self.reads += 1
        return self._read(o, [("all",)])[0]["add"]

    def entry(self, o, member):
        self.reads += 1
        r = self._read(o, [("key", member)])[0]
        return r["rm"] if r["val"] else None

    def value(self, o):
        self.reads += 1
        return self._read(o, [("all",)])[0]["list"]
