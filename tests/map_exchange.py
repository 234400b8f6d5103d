"""The reference's Map op-exchange properties (test/map.rs:518-745) as one
harness over three engines — test infrastructure for
tests/test_map_exchange_ref.py (CPU) and tests/test_gpu_map_exchange.py (GPU);
no tests in this module.

Kinds: "mvreg" Map<u64, MVReg>, "orswot" Map<u64, Orswot>, "nested"
Map<u64, Map<u64, MVReg>> (the reference's TestMap).

A case is three op vectors from three distinct actors, built as build_opvec
builds them (test/map.rs:13-46): one actor per vector, op i's clock is
Dot{actor, i}.into() (empty for i = 0), an Up's dot is (actor, i + 1). The
generators (`opvec` for the flat kinds, `rand_opvec` / `distinct` for the
nested one) live here; tests/test_map_props.py and
tests/test_map_nested_oracle.py import them.

Per case the three actors are interned order-preserving to three ids of
[0, A): 0, 1, 2 or the spread ids {3, A // 2, A - 1}. The op vectors are
converted to the kernels' op lists in that id space and every engine runs
those lists, so the restatement's states are the kernel's states as they are.

A property is a pair of expressions over the built maps S1..S3 and the op
lists o1..o3, B(i) = build, P(e, j) = apply of o_j, M(e, f) = merge, T(e) =
truncate by the empty clock; `evaluate` runs an expression on an engine, each
distinct sub-expression once:
  - PyEngine: the Python restatement (oracle/crdts_ref.py), recording the
    peak sizes of every state it makes, intermediate states of an apply
    included — the capacities of the GPU run come from these alone;
  - OracleEngine: the C++ oracle's Map handles (flat kinds; no truncate);
  - GpuEngine: every state a device slab from start to finish. B is one
    *_apply launch from an all-empty slab, every output buffer of every
    launch is pattern-filled first, and nothing is canonicalised, copied to
    the host or repacked between launches.
"""
from __future__ import annotations

import contextlib
import functools
import random

import numpy as np

import map_kat_runner as mkr
import map_opgen
import map_orswot_opgen
import map_slab
import nested_opgen as ng
from map_slab import crdts_ref

SIZE = 100  # quickcheck's default size: u8 draws in [0, 100)
KINDS = ("mvreg", "orswot", "nested")
PATTERN = 0x5A5A5A5A


# ------------------------------------------------------------- generators
def opvec(rng, actor, n_max=24, keys=SIZE, kind="mvreg"):
    ops = []
    for i in range(rng.randrange(0, n_max + 1)):
        choice, inner, key, val = (rng.randrange(SIZE), rng.randrange(SIZE), rng.randrange(keys),
                                   rng.randrange(SIZE))
        clock = [(actor, i)] if i > 0 else []  # Dot{actor, 0}.into() is the empty clock
        dot = (actor, i + 1)
        if choice % 3 == 0:
            ops.append(("up", dot, key, inner % 2 if kind == "orswot" else 0, val, clock))
        elif choice % 3 == 1:
            ops.append(("rm", None, key, None, None, clock))
    return ops


def apply_ops(be, m, ops, kind):
    for op, dot, key, sub, val, clock in ops:
        if op == "rm":
            be.apply_rm(m, key, clock)
        elif kind == "mvreg":
            be.apply_up_put(m, dot, key, clock, val)
        elif sub == 0:
            be.apply_up_add(m, dot, key, val)
        else:
            _apply_up_orswot_rm(be, m, dot, key, val, clock)


def _apply_up_orswot_rm(be, m, dot, key, member, clock):
    if isinstance(be, mkr.OracleMapBackend):
        m.apply_up_orswot(dot, key, 1, member, clock)
    else:
        m.apply_up(dot, key, lambda s: s.apply_rm(crdts_ref.VClock(clock), member))


def build_opvec(actor, prims):
    """test/map.rs:13-46: op i's clock is Dot {actor, i}.into() (empty for
    i = 0: witness of counter 0), an Up's dot is clock.inc(actor)."""
    ops = []
    for i, (choice, inner_choice, key, inner_key, val) in enumerate(prims):
        clock = [[actor, i]] if i > 0 else []
        dot = [actor, i + 1]
        if choice % 3 == 0:
            if inner_choice % 3 == 0:
                inner = {"up": {"dot": dot, "key": inner_key, "op": {"put": {"clock": clock, "val": val}}}}
            elif inner_choice % 3 == 1:
                inner = {"rm": {"clock": clock, "key": inner_key}}
            else:
                inner = "nop"
            ops.append({"up": {"dot": dot, "key": key, "op": inner}})
        elif choice % 3 == 1:
            ops.append({"rm": {"clock": clock, "key": key}})
        else:
            ops.append("nop")
    return actor, ops


def rand_opvec(rng, actor=None, keys=4):
    """An arbitrary (u8, Vec<(u8, u8, u8, u8, u8)>) with keys drawn from a
    small range (quickcheck's u8 keys rarely collide; a small range makes the
    removes and concurrent updates meet)."""
    n = rng.randrange(0, 12)
    prims = [(rng.randrange(256), rng.randrange(256), rng.randrange(keys), rng.randrange(keys), rng.randrange(256))
             for _ in range(n)]
    return build_opvec(rng.randrange(256) if actor is None else actor, prims)


def distinct(rng, k, keys=4):
    acts = rng.sample(range(256), k)
    return [rand_opvec(rng, a, keys) for a in acts]


# ------------------------------------------------------------------ cases
# name -> (cases, n_actors, spread ids, keys drawn from); "k2" is the nested kind's second draw
MODES = {"a16": (1000, 16, False, 4), "a100": (200, 100, True, 4), "k2": (300, 16, False, 2)}
SEEDS = {"mvreg": 1234, "orswot": 1234, "nested": 99}


def modes_of(kind):
    return ("a16", "a100", "k2") if kind == "nested" else ("a16", "a100")


def actor_ids(A, spread):
    return (3, A // 2, A - 1) if spread else (0, 1, 2)


@functools.lru_cache(maxsize=None)
def draw(kind, n, keys):
    """n cases [(actors, vectors)]: three distinct actors and their op vectors
    in the generator's own form. Equal actors are never drawn, so no case is
    discarded. The first cases of a longer draw are the shorter draw's."""
    rng = random.Random(SEEDS[kind])
    cases = []
    for _ in range(n):
        if kind == "nested":
            acts, vecs = zip(*distinct(rng, 3, keys))
        else:
            acts = tuple(rng.sample(range(SIZE), 3))
            vecs = tuple(opvec(rng, a, n_max=12, keys=keys, kind=kind) for a in acts)
        assert len(set(acts)) == 3
        cases.append((tuple(acts), tuple(vecs)))
    return tuple(cases)


def interning(actors, ids):
    """Order-preserving: the smallest actor gets the smallest id (CLOCK ORDER and every comparison are kept)."""
    return dict(zip(sorted(actors), sorted(ids)))


def kernel_ops(kind, vec, fwd):
    """One op vector -> the kernel's op list (MapOps / MapOrswotOps tuples, MapMapOps literal ops), actors
    renamed by fwd."""
    if kind == "nested":
        return [ng.relabel_op(op, fwd) for op in vec]
    out = []
    for op, dot, key, sub, val, clock in vec:
        pairs = [(fwd[a], c) for a, c in clock]
        if op == "rm":
            out.append(("rm", key, pairs))
        elif kind == "mvreg":
            out.append(("up", fwd[dot[0]], dot[1], key, pairs, val))
        elif sub == 0:
            out.append(("up_add", fwd[dot[0]], dot[1], key, val))
        else:
            out.append(("up_rm", fwd[dot[0]], dot[1], key, val, pairs))
    return out


@functools.lru_cache(maxsize=None)
def op_lists(kind, mode):
    """(o1, o2, o3): per vector position, the n cases' kernel op lists."""
    n, A, spread, keys = MODES[mode]
    ids = actor_ids(A, spread)
    cases = draw(kind, MODES["a16"][0] if keys == 4 else n, keys)[:n]
    assert len(cases) == n  # 0 discarded
    return tuple([kernel_ops(kind, vecs[j], interning(acts, ids)) for acts, vecs in cases] for j in range(3))


# ------------------------------------------------------ the restatement's side
def new_map(kind):
    return mkr.PyMapBackend().new(kind)


APPLY_ONE = {"mvreg": map_opgen.apply_op, "orswot": map_orswot_opgen.apply_op, "nested": mkr.apply_raw}
CAP_NAMES = {"mvreg": ("kcap", "mcap", "dcap", "scap"),
             "orswot": map_orswot_opgen.CAP_NAMES,  # kcap, mcap, vdcap, vscap, dcap, scap
             "nested": ("kcap", "dcap", "scap", "inner_kcap", "inner_mcap", "inner_dcap", "inner_scap")}


def sizes(kind, m):
    """The capacities state m needs, in CAP_NAMES[kind] order."""
    if kind == "nested":
        return ng.sizes(m)
    mx = lambda xs: max(xs, default=0)  # noqa: E731
    vals = [v for _, v in m.entries.values()]
    nd, ns = len(m.deferred), mx(len(s) for s in m.deferred.values())
    if kind == "mvreg":
        return (len(m.entries), mx(len(r.vals) for r in vals), nd, ns)
    return (len(m.entries), mx(len(o.entries) for o in vals), mx(len(o.deferred) for o in vals),
            mx(len(s) for o in vals for s in o.deferred.values()), nd, ns)


@contextlib.contextmanager
def _no_deferred_pass():
    saved = crdts_ref.Map.apply_deferred, crdts_ref.Orswot.apply_deferred
    crdts_ref.Map.apply_deferred = crdts_ref.Orswot.apply_deferred = lambda self: None
    try:
        yield
    finally:
        crdts_ref.Map.apply_deferred, crdts_ref.Orswot.apply_deferred = saved


def peak_sizes(kind, start, ops):
    """(end state, peak): the sizes the object needs at any step of its op
    list. Within an Up the state is at its largest after the nested op and
    before the deferred passes (map's and nested set's), which only remove:
    that point is measured on a copy whose deferred passes do nothing."""
    m = start.clone()
    peak = sizes(kind, m)
    for op in ops:
        probe = m.clone()
        with _no_deferred_pass():
            APPLY_ONE[kind](probe, op)
        APPLY_ONE[kind](m, op)
        peak = tuple(max(x) for x in zip(peak, sizes(kind, probe), sizes(kind, m)))
    return m, peak


def ordered(m):
    """Structural identity with MVReg values in Vec order (what a slab row holds)."""
    def val(v):
        if isinstance(v, crdts_ref.Map):
            return ordered(v)
        if isinstance(v, crdts_ref.MVReg):
            return tuple((c.canonical(), x) for c, x in v.vals)
        return v.canonical()
    return (m.clock.canonical(), tuple((k, c.canonical(), val(v)) for k, (c, v) in sorted(m.entries.items())),
            tuple(sorted((c.canonical(), tuple(sorted(s))) for c, s in m.deferred.items())))


# ------------------------------------------------------------ expressions
def B(i):
    return ("B", i)


def P(e, j):
    return ("P", e, j)


def M(e, f):
    return ("M", e, f)


def T(e):
    return ("T", e)


S1, S2, S3 = B(0), B(1), B(2)
X1, X2, MM = P(S1, 1), P(S2, 0), M(S1, S2)
# property -> (pairs that must be ==, further expressions checked for parity only)
PROPERTIES = {
    "op_exchange_same_as_merge": ([(X1, MM), (X2, MM)], []),                              # test/map.rs:520
    "op_exchange_converges": ([(X1, X2)], []),                                            # :546
    "op_exchange_associative": ([(P(X1, 2), P(P(S2, 2), 0))], []),                        # :574, :620
    "op_idempotent": ([(P(S1, 0), S1)], []),                                              # :607
    "merge_commutative": ([(MM, M(S2, S1))], []),                                         # :688
    "merge_associative": ([(M(MM, S3), M(S1, M(S2, S3)))], []),                           # :654
    "merge_idempotent": ([(M(S1, S1), S1)], []),                                          # :716
    "truncate_with_empty_vclock_is_nop": ([(T(MM), MM)], [M(T(MM), S3)]),                 # :732
    "ops_equal_merge_of_three": ([(P(X1, 2), M(MM, S3))], []),
}


def show(e):
    if e[0] == "B":
        return f"S{e[1] + 1}"
    if e[0] == "P":
        return f"P({show(e[1])}, o{e[2] + 1})"
    if e[0] == "M":
        return f"M({show(e[1])}, {show(e[2])})"
    return f"T({show(e[1])})"


def expressions(prop):
    pairs, more = PROPERTIES[prop]
    return [e for p in pairs for e in p] + list(more)


def evaluate(eng, ops, e, memo):
    """The batch expression e denotes on engine eng; memo: expression -> batch (each launch runs once)."""
    if e not in memo:
        if e[0] == "B":
            memo[e] = eng.build(ops[e[1]])
        elif e[0] == "P":
            memo[e] = eng.apply(evaluate(eng, ops, e[1], memo), ops[e[2]])
        elif e[0] == "M":
            memo[e] = eng.merge(evaluate(eng, ops, e[1], memo), evaluate(eng, ops, e[2], memo))
        else:
            memo[e] = eng.truncate_empty(evaluate(eng, ops, e[1], memo))
    return memo[e]


# ----------------------------------------------------------------- engines
class PyEngine:
    """Batches are lists of restatement maps (never modified once made)."""

    def __init__(self, kind):
        self.kind = kind
        self.peak = (0,) * len(CAP_NAMES[kind])  # over every state made by build / apply, intermediate ones included

    def _run(self, starts, lists):
        out = []
        for m, ops in zip(starts, lists):
            end, peak = peak_sizes(self.kind, m, ops)
            self.peak = tuple(max(x) for x in zip(self.peak, peak))
            out.append(end)
        return out

    def build(self, lists):
        return self._run([new_map(self.kind)] * len(lists), lists)

    def apply(self, batch, lists):
        return self._run(batch, lists)

    def merge(self, a, b):
        out = []
        for x, y in zip(a, b):
            x = x.clone()
            x.merge(y)
            out.append(x)
        return out

    def truncate_empty(self, batch):
        out = []
        for x in batch:
            x = x.clone()
            x.truncate(crdts_ref.VClock())
            out.append(x)
        return out

    def view(self, batch):
        return batch


class OracleEngine:
    """Batches are lists of the C++ oracle's Map handles (flat kinds; the handles have no truncate)."""

    def __init__(self, kind, n_actors, caps):
        assert kind in ("mvreg", "orswot")
        self.kind = kind
        self.be = mkr.OracleMapBackend(n_actors, caps)
        self.one = map_opgen.apply_op_oracle if kind == "mvreg" else map_orswot_opgen.apply_op_oracle

    def _run(self, starts, lists):
        for h, ops in zip(starts, lists):
            for op in ops:
                self.one(h, op)
        return starts

    def build(self, lists):
        return self._run([self.be.new(self.kind) for _ in lists], lists)

    def apply(self, batch, lists):
        return self._run([h.clone() for h in batch], lists)

    def merge(self, a, b):
        out = [h.clone() for h in a]
        for x, y in zip(out, b):
            x.merge(y)
        return out

    def truncate_empty(self, batch):
        raise NotImplementedError("the oracle's Map handles have no truncate")

    def view(self, batch):
        return [self.be.view(h) for h in batch]


def _slab_cls(kind):
    import crdts_hip

    return {"mvreg": crdts_hip.MapSlab, "orswot": crdts_hip.MapOrswotSlab, "nested": crdts_hip.MapMapSlab}[kind]


def alloc(kind, n, A, caps, device=None):
    """A zeroed slab; caps in CAP_NAMES[kind] order."""
    cls = _slab_cls(kind)
    if kind == "mvreg":
        return cls.alloc(n, A, *caps, device=device)
    if kind == "orswot":
        return cls.alloc(n, A, device=device, **dict(zip(CAP_NAMES[kind], caps)))
    return cls.alloc(n, A, *caps[:3], tuple(caps[3:]), device=device)


def caps_of(kind, S):
    if kind == "mvreg":
        return (S.kcap, S.mcap, S.dcap, S.scap)
    if kind == "orswot":
        return tuple(S.caps[k] for k in CAP_NAMES[kind])
    return (S.kcap, S.dcap, S.scap) + tuple(S.inner_caps)


TO_ROW = {"mvreg": map_slab.mvreg_map_to_row, "orswot": map_slab.orswot_map_to_row,
          "nested": map_slab.nested_map_to_row}
FROM_ROW = {"mvreg": map_slab.mvreg_map_from_row, "orswot": map_slab.orswot_map_from_row,
            "nested": map_slab.nested_map_from_row}


def pack(kind, states, A, caps):
    """Host slab of restatement states (the to_row writers assert that every state fits)."""
    S = alloc(kind, len(states), A, caps)
    for i, m in enumerate(states):
        TO_ROW[kind](m, S, i, A, zero=False)  # a new slab
    return S


def unpack(kind, H):
    """Host slab -> restatement maps, MVReg values in the slab's order."""
    return [FROM_ROW[kind](H, i) for i in range(int(H.a["n_keys"].shape[0]))]


def _arrays(kind, S):
    return list(S.a.values()) + (list(S.inner.a.values()) if kind == "nested" else [])


class GpuEngine:
    """Batches are device slabs, from the build to the end of the property.
    Every launch writes into a freshly pattern-filled slab and is followed by
    the context's status check (a latched CRDT_ECAPACITY / CRDT_ENONCANON
    raises)."""

    def __init__(self, kind, eng, n_actors, caps):
        import crdts_hip

        self.kind, self.eng, self.A, self.caps = kind, eng, n_actors, tuple(caps)
        self.ops_cls = {"mvreg": crdts_hip.MapOps, "orswot": crdts_hip.MapOrswotOps,
                        "nested": crdts_hip.MapMapOps}[kind]
        name = {"mvreg": "map_mvreg", "orswot": "map_orswot", "nested": "map_map"}[kind]
        self._apply, self._merge, self._truncate = (getattr(eng, f"{name}_{f}") for f in ("apply", "merge", "truncate"))
        self.launches = 0

    def _patterned(self, n, caps):
        out = alloc(self.kind, n, self.A, caps, device="cuda")
        for v in _arrays(self.kind, out):
            v.fill_(PATTERN)
        return out

    def _checked(self, out):
        self.eng.status()
        self.launches += 1
        return out

    def build(self, lists):
        return self.apply(alloc(self.kind, len(lists), self.A, self.caps, device="cuda"), lists)

    def apply(self, S, lists):
        n = int(S.a["n_keys"].shape[0])
        assert len(lists) == n
        out = self._patterned(n, caps_of(self.kind, S))
        return self._checked(self._apply(S, self.ops_cls.from_lists(lists), self.A, out=out))

    def merge(self, S, O):
        n = int(S.a["n_keys"].shape[0])
        caps = tuple(x + y for x, y in zip(caps_of(self.kind, S), caps_of(self.kind, O)))
        return self._checked(self._merge(S, O, self.A, out=self._patterned(n, caps)))

    def truncate_empty(self, S):
        import torch

        n = int(S.a["n_keys"].shape[0])
        rows = torch.zeros((n, self.A), dtype=torch.int64, device="cuda")
        return self._checked(self._truncate(S, rows, self.A, out=self._patterned(n, caps_of(self.kind, S))))


# ---------------------------------------------------- checks on a read-back slab
def assert_rows(kind, got, exp, what=""):
    """Canonical forms of two slabs of equal capacities equal, field by field."""
    if kind == "nested":
        return ng.assert_rows(got, exp, what=what)
    g, e = got.canonical(), exp.canonical()
    n = int(e.a["n_keys"].shape[0])
    for f in e.a:
        d = (np.asarray(g.a[f]) != np.asarray(e.a[f])).reshape(n, -1).any(axis=1)
        bad = np.nonzero(d)[0]
        assert bad.size == 0, f"{what} {f}: {bad.size} objects differ, first {bad[:5].tolist()}"


VALUE_FIELDS = {"mvreg": ("keys", "mv_val", "dset"), "orswot": ("keys", "vmem", "vdset", "dset")}


def pattern_words(kind, H):
    """How many used key / value / set words of host slab H hold the fill
    pattern (as the 64-bit fill leaves it, or in both halves). The generators
    draw keys, values and members below 256."""
    words = []
    if kind == "nested":
        a = H.a
        key = np.arange(H.kcap)[None, :] < a["n_keys"][:, None]
        dfr = np.arange(H.dcap)[None, :] < a["n_def"][:, None]
        dset = dfr[..., None] & (np.arange(H.scap)[None, None, :] < a["dset_n"][..., None])
        words += [a["keys"][key], a["dset"][dset]]
        live = key.reshape(-1)
        masks = H.inner.used_masks()
        for f in VALUE_FIELDS["mvreg"]:
            words.append(H.inner.a[f][live][masks[f][live]])
    else:
        masks = H.used_masks()
        words += [H.a[f][masks[f]] for f in VALUE_FIELDS[kind]]
    w = np.concatenate([x.reshape(-1) for x in words]) if words else np.zeros(0, np.uint64)
    return int(((w == np.uint64(PATTERN)) | (w == np.uint64(PATTERN * 0x100000001))).sum())


# ------------------------------------------------------------ the reference run
def round_up(peak):
    """Capacities from peak sizes: the next even number, at least 2."""
    return tuple(max(2, p + (p & 1)) for p in peak)


@functools.lru_cache(maxsize=None)
def reference(kind, mode):
    """(ops, memo, caps, peak) of the restatement's run of every property —
    computed once per (kind, mode), never modified. memo: expression -> list
    of restatement maps; caps: the rounded peak of every state build / apply
    made (merge outputs take the sums of their inputs' capacities)."""
    ops = op_lists(kind, mode)
    eng = PyEngine(kind)
    memo = {}
    for prop in PROPERTIES:
        for e in expressions(prop):
            evaluate(eng, ops, e, memo)
    caps = round_up(eng.peak)
    assert all(p <= c for p, c in zip(eng.peak, caps))
    return ops, memo, caps, eng.peak


def result_caps(caps, e):
    """The capacities the GPU run gives expression e's slab."""
    if e[0] == "M":
        return tuple(x + y for x, y in zip(result_caps(caps, e[1]), result_caps(caps, e[2])))
    return caps if e[0] == "B" else result_caps(caps, e[1])


# ------------------------------------------------------------- non-vacuity
def _values(kind, m):
    """The leaf registers / sets of a map (the nested kind: of its inner maps)."""
    if kind == "nested":
        return [r for _, v in m.entries.values() for _, r in v.entries.values()]
    return [v for _, v in m.entries.values()]


def _n_values(v):
    return len(v.vals) if isinstance(v, crdts_ref.MVReg) else len(v.entries)


def shares(kind, mode):
    """Shares (of the 3 n built maps, of the n merges m1 ^ m2, of the n
    cases), from the restatement's states alone."""
    _, memo, _, _ = reference(kind, mode)
    built = memo[S1] + memo[S2] + memo[S3]
    mm = memo[MM]
    fresh = ordered(new_map(kind))
    def frac(xs):
        xs = [bool(x) for x in xs]
        return sum(xs) / len(xs)

    if kind == "nested":
        empty = lambda m: any(not v.entries for _, v in m.entries.values())  # noqa: E731
    else:
        empty = lambda m: any(_n_values(v) == 0 for v in _values(kind, m))  # noqa: E731
    out = {
        "built_deferred": frac(m.deferred for m in built),
        "built_empty_value": frac(empty(m) for m in built),
        "built_empty_map": frac(ordered(m) == fresh for m in built),
        "merged_deferred": frac(m.deferred for m in mm),
        "merged_multi_value": frac(any(_n_values(v) >= 2 for v in _values(kind, m)) for m in mm),
        # == (MVReg's set-like PartialEq) although the rows differ in MVReg value order
        "order_sensitive_x1": frac(a == b and ordered(a) != ordered(b) for a, b in zip(memo[X1], mm)),
        "order_sensitive_x2": frac(a == b and ordered(a) != ordered(b) for a, b in zip(memo[X2], mm)),
    }
    if kind == "nested":
        out["built_inner_deferred"] = frac(any(v.deferred for _, v in m.entries.values()) for m in built)
    return out


# The shares the restatement shows at the committed seeds (SEEDS), rounded
# down to three places. A floor is half of its share; a share of 0 has no
# floor. Asserted from restatement states in both test files.
MEASURED = {
    ("mvreg", "a16"): dict(built_deferred=0.258, built_empty_value=0.136, built_empty_map=0.158,
                           merged_deferred=0.457, merged_multi_value=0.225, order_sensitive_x2=0.225),
    ("mvreg", "a100"): dict(built_deferred=0.258, built_empty_value=0.125, built_empty_map=0.160,
                            merged_deferred=0.465, merged_multi_value=0.245, order_sensitive_x2=0.245),
    ("orswot", "a16"): dict(built_deferred=0.258, built_empty_value=0.406, built_empty_map=0.158,
                            merged_deferred=0.457, merged_multi_value=0.224),
    ("orswot", "a100"): dict(built_deferred=0.258, built_empty_value=0.372, built_empty_map=0.160,
                             merged_deferred=0.465, merged_multi_value=0.220),
    ("nested", "a16"): dict(built_deferred=0.260, built_inner_deferred=0.297, built_empty_value=0.517,
                            built_empty_map=0.169, merged_deferred=0.474, merged_multi_value=0.005,
                            order_sensitive_x2=0.005),
    ("nested", "a100"): dict(built_deferred=0.235, built_inner_deferred=0.320, built_empty_value=0.545,
                             built_empty_map=0.160, merged_deferred=0.465, merged_multi_value=0.005,
                             order_sensitive_x2=0.005),
    ("nested", "k2"): dict(built_deferred=0.250, built_inner_deferred=0.223, built_empty_value=0.409,
                           built_empty_map=0.162, merged_deferred=0.460, merged_multi_value=0.020,
                           order_sensitive_x2=0.020),
}
FLOORS = {k: {name: share / 2 for name, share in d.items()} for k, d in MEASURED.items()}


def assert_non_vacuous(kind, mode):
    got = shares(kind, mode)
    for name, floor in FLOORS[kind, mode].items():
        assert got[name] >= floor, f"{kind} {mode}: share {name} {got[name]:.3f} below its floor {floor}"
    return got
