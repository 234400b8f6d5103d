"""Test helper: Map merge batches that sit on the launchers' boundaries
(map_lift.tier_*), lifted like the value batches: the value-row stage on and
off, the deferred-set stages at their limit and past it, 63 / 64 / 65 keys, 64
surviving deferred clocks a side, 128 kept values a side, the Map<Orswot>
workspace within one member of 64 KB with every part full, the 64 / 65 actor
switch. Shared by tests/test_map_lift.py and tests/test_gpu_map_edges.py.

The states are put together directly (capacities this large are out of the op
generators' reach): every side is canonical — sorted keys, entry, value and
member clocks inside the map clock, deferred clocks ahead of it on an actor the
side has not heard from (as a remove from an unseen replica leaves them,
tests/test_gpu_map_orswot.py::_nested_deferred_map) — and the two sides share
keys, value clocks and deferred clocks, so that domination, equal clocks and
united key sets occur."""
import collections
import functools
import random

import map_edge_cases as mc
import map_lift as ml
from map_slab import crdts_ref

VC = crdts_ref.VClock
FLOOR = mc.FLOOR


def _writers(rng, A):
    """(writers of self, writers of other, the two unseen actors) — the ends of the lane mappings among them."""
    hot = [a for a in (0, 63, 64, A - 1) if a < A]
    pool = sorted(set(rng.sample(range(A), min(A, 8))) | set(hot))
    if len(pool) < 4:
        return pool, pool, (pool[-1], pool[0])
    u = (pool.pop(rng.randrange(len(pool))), pool.pop(rng.randrange(len(pool))))
    return pool, pool, u


def _dots(rng, actors, hi=5, k=None):
    acts = rng.sample(actors, min(len(actors), k or rng.randint(1, 3)))
    return VC([(a, rng.randint(1, hi)) for a in acts])


def _antichain(rng, actors, n, lo=0):
    """n pairwise concurrent clocks (one actor: n distinct ones, a chain)."""
    if len(actors) < 2:
        return [VC([(actors[0], lo + j + 1)]) for j in range(n)]
    p, q = rng.sample(actors, 2)
    return [VC([(p, lo + j + 1), (q, lo + n - j)]) for j in range(n)]


def _register(rng, actors, n, shared):
    """An MVReg of n values: some of `shared` (the other side holds them too,
    or holds them one step ahead), the rest an antichain of its own."""
    r = crdts_ref.MVReg()
    take = rng.sample(shared, min(len(shared), rng.randint(0, min(n, 2))))
    for c, v in take:
        r.vals.append((c.clone(), v))
    for c in _antichain(rng, actors, n - len(r.vals), lo=rng.randint(0, 2)):
        if all(c != e for e, _ in r.vals):
            r.vals.append((c, rng.randrange(1, 1 << 40)))
    return r


def _witness_all(m):
    """The map clock: everything the map holds (canonical: every dot inside it)."""
    for c, v in m.entries.values():
        m.clock.merge(c)
        if isinstance(v, crdts_ref.Map):
            _witness_all(v)
            m.clock.merge(v.clock)
        elif isinstance(v, crdts_ref.Orswot):
            for e in v.entries.values():
                v.clock.merge(e)
            m.clock.merge(v.clock)
        else:
            for cc, _ in v.vals:
                m.clock.merge(cc)


def _defer(rng, m, n, keys, unseen, base, set_max, shared=()):
    """n deferred removes ahead of every clock on the unseen actors, through
    the op path (Map::apply_rm: the clock is not inside the map's)."""
    clocks = list(shared)[:n]
    j = 0
    while len(clocks) < n:
        j += 1
        c = VC([(unseen[0], base + j)] + ([(unseen[1], rng.randint(1, 3))] if rng.random() < 0.4 else []))
        if c not in clocks:
            clocks.append(c)
    if unseen[0] in {a for c, _ in m.entries.values() for a in c.dots}:
        keys = [10_000 + k for k in keys]  # (one actor: such a remove would retire every key it names)
    for c in clocks:
        for k in rng.sample(keys, rng.randint(1, min(set_max, len(keys)))):
            m.apply_rm(k, c)
    return clocks


# ------------------------------------------------------------------ Map<u64, MVReg>
def mvreg_pair(rng, A, nk, ms, nd, set_max=2, values=None, disjoint_values=False, same_keys=False,
               share_def=True):
    """nk = (keys of self, of other), ms = (values per key), nd = (deferred
    clocks): a pair of Map<u64, MVReg> over a shared key universe; key 0 is on
    both sides. `values` (per side) is key 0's exact value count: the key that
    fills the value stage. disjoint_values: the sides' value clocks are
    concurrent (all kept); same_keys: both sides hold the same keys;
    share_def=False: no deferred clock is on both sides."""
    ws, wo, unseen = _writers(rng, A)
    universe = list(range(max(nk) + 2))
    out = []
    shared_vals = {k: [(c, rng.randrange(1, 1 << 40)) for c in _antichain(rng, ws, 2, lo=3)] for k in universe}
    for side, (w, n_keys, m_vals, n_def) in enumerate(zip((ws, wo), nk, ms, nd)):
        m = crdts_ref.Map(crdts_ref.MVReg)
        ks = universe[:n_keys] if same_keys else sorted(rng.sample(universe[1:], n_keys - 1) + [0])
        for i, k in enumerate(ks):
            big = values is not None and i == 0  # key 0, on both sides: exactly values[side] values
            n = values[side] if big else rng.randint(1, m_vals) if m_vals > 1 else m_vals
            acts = (w[:len(w) // 2] if side == 0 else w[len(w) // 2:]) if disjoint_values and len(w) >= 4 else w
            reg = _register(rng, acts, n, [] if disjoint_values or big else shared_vals[k])
            ec = _dots(rng, w)
            if rng.random() < 0.3 and len(w) >= 4:
                ec.witness(unseen[0], 1)  # a dot the other side's deferred removes retire
            m.entries[k] = [ec, reg]
        _witness_all(m)
        out.append((m, n_def))
    keys = sorted(set(out[0][0].entries) | set(out[1][0].entries)) or [0]
    base = 8
    shared = _defer(rng, crdts_ref.Map(crdts_ref.MVReg), min(nd) // 2 if share_def else 0, keys, unseen, base, 1)
    for side, (m, n_def) in enumerate(out):
        _defer(rng, m, n_def, keys, unseen, base + 100 * (side + 1), set_max, shared)
    return out[0][0], out[1][0]


# ------------------------------------------------------------------ Map<u64, Orswot>
def _orswot(rng, w, members, n_def, set_n, unseen, base, shared=()):
    o = crdts_ref.Orswot()
    for x in members:
        o.entries[x] = _dots(rng, w)
    for e in o.entries.values():
        o.clock.merge(e)
    clocks = list(shared)[:n_def]
    j = 0
    while len(clocks) < n_def:
        j += 1
        clocks.append(VC([(unseen[1], base + j)]))
    for c in clocks:
        o.deferred[c.clone()] = set(rng.sample(range(1000, 1000 + 4 * max(1, set_n)), set_n)) if set_n else {members[0]}
    return o


def orswot_pair(rng, A, caps, nk, nd, full=False):
    """A pair of Map<u64, Orswot>. full: key 0 holds mcap members a side, all
    different, and vdcap nested deferred clocks, all different; key 1 holds
    vdcap nested deferred clocks the sides share, with vscap members each, all
    different — the merged keys fill the workspace's members, deferred clocks
    and member sets."""
    ws, wo, unseen = _writers(rng, A)
    cs, co = caps
    universe = list(range(max(nk) + 2))
    shared_d = [VC([(unseen[1], 50 + j)]) for j in range(min(cs["vdcap"], co["vdcap"]))]
    out = []
    for side, (w, c, n_keys, n_def) in enumerate(zip((ws, wo), (cs, co), nk, nd)):
        m = crdts_ref.Map(crdts_ref.Orswot)
        ks = sorted(rng.sample(universe[2:], n_keys - 2) + [0, 1]) if full else sorted(rng.sample(universe, n_keys))
        for k in ks:
            if full and k == 0:
                mem = [5000 * side + 2 * j + 1 for j in range(c["mcap"])]
                o = _orswot(rng, w, mem, c["vdcap"], 1, unseen, 100 * (side + 1))
            elif full and k == 1:
                o = _orswot(rng, w, [7 + side], c["vdcap"], 0, unseen, 0, shared_d)
                for d in o.deferred:
                    o.deferred[d] = {2000 + 1000 * side + 10 * j for j in range(c["vscap"])}
            if full and k < 2:  # dots of the side's own writer, ahead of all the other side has seen: all survive
                for j, x in enumerate(sorted(o.entries)):
                    o.entries[x] = VC([(w[side], 10 + j)])
                o.clock = VC([(w[side], 10 + len(o.entries))])
                m.entries[k] = [VC([(w[side], 300)]), o]
                continue
            else:
                mem = rng.sample(range(1, 12), rng.randint(1, min(4, c["mcap"])))
                o = _orswot(rng, w, mem, rng.randint(0, min(2, c["vdcap"])), min(2, c["vscap"]), unseen,
                            20 * (side + 1), shared_d[:1] if rng.random() < 0.5 else ())
            ec = _dots(rng, w)
            if rng.random() < 0.3 and len(w) >= 4:
                ec.witness(unseen[0], 1)
            m.entries[k] = [ec, o]
        _witness_all(m)
        out.append((m, n_def, c))
    keys = sorted(set(out[0][0].entries) | set(out[1][0].entries)) or [0]
    shared = _defer(rng, crdts_ref.Map(crdts_ref.Orswot), min(nd) // 2, keys, unseen, 8, 1)
    for side, (m, n_def, c) in enumerate(out):
        _defer(rng, m, n_def, keys, unseen, 8 + 100 * (side + 1), min(2, c["scap"]), shared)
    return out[0][0], out[1][0]


# ------------------------------------------------------------------ Map<u64, Map<u64, MVReg>>
def nested_pair(rng, A, nk, nd, set_max=2):
    ws, wo, unseen = _writers(rng, A)
    # 40 % of the pairs have heard nothing of each other and write with different actors: no dot of a shared
    # key is retired, and the merged value is truncated by the empty clock
    quiet = rng.random() < 0.4 and len(ws) >= 4
    if quiet:
        ws, wo = ws[:len(ws) // 2], ws[len(ws) // 2:]
    universe = list(range(max(nk) + 2))
    out = []
    for side, (w, n_keys, n_def) in enumerate(zip((ws, wo), nk, nd)):
        m = crdts_ref.Map(lambda: crdts_ref.Map(crdts_ref.MVReg))
        for k in sorted(rng.sample(universe, n_keys)):
            inner = crdts_ref.Map(crdts_ref.MVReg)
            for k2 in rng.sample(range(4), rng.randint(0, 2)):
                inner.entries[k2] = [_dots(rng, w), _register(rng, w, rng.randint(1, 2), [])]
            ec = _dots(rng, w)
            if rng.random() < 0.3 and len(w) >= 4 and not quiet:
                ec.witness(unseen[0], 1)
            m.entries[k] = [ec, inner]
        _witness_all(m)
        out.append((m, n_def))
    # the sides have heard of part of each other: half of the entries' dots are then inside the other's clock
    for (m, _), (o, _) in ((out[0], out[1]), (out[1], out[0])):
        for a, c in list(o.clock.dots.items()):
            if rng.random() < 0.5 and not quiet:
                m.clock.witness(a, c)
                for _, v in m.entries.values():
                    if rng.random() < 0.5:
                        v.clock.witness(a, c)
    keys = sorted(set(out[0][0].entries) | set(out[1][0].entries)) or [0]
    shared = _defer(rng, mc.ng.mkr.nested_map(), min(nd) // 2, keys, unseen, 8, 1)
    for side, (m, n_def) in enumerate(out):
        _defer(rng, m, n_def, keys, unseen, 8 + 100 * (side + 1), set_max, shared)
    return out[0][0], out[1][0]


def nested_key_classes(x, y):
    """The outer keys of a pair by class: "self_only", "other_only", and for a
    key of both sides whether Map::merge truncates its merged value by an
    empty clock ("both_plain") or not ("both_truncated") (src/map.rs:193-268)."""
    got = collections.Counter()
    for k in set(x.entries) | set(y.entries):
        if k not in y.entries:
            got["self_only"] += 1
        elif k not in x.entries:
            got["other_only"] += 1
        else:
            c, oc = x.entries[k][0].clone(), y.entries[k][0].clone()
            common = c.intersection(oc)
            c.subtract(common)
            oc.subtract(common)
            c.subtract(y.clock)
            oc.subtract(x.clock)
            common.merge(c)
            common.merge(oc)
            deleted = x.entries[k][0].clone()
            deleted.merge(y.entries[k][0])
            deleted.subtract(common)
            got["both_plain" if deleted.is_empty() else "both_truncated"] += 1
    return got


# ------------------------------------------------------------------ the batches
def _mo_caps(**kw):
    return dict(dict(kcap=8, mcap=4, vdcap=2, vscap=2, dcap=4, scap=4), **kw)


# Map<Orswot> at 16 actors, the workspace at 64 KB exactly: 65,536 bytes; one more member on a side: 65,816
MO_FULL = _mo_caps(mcap=108, vdcap=8, vscap=4)

# name -> (kind, A, n, (caps of self, caps of other), per-object shapes cycled over the batch)
TIER_BATCHES = {
    # value stage on / off at mcap * A = 128 | 129: key 0 fills the stage (ms * A = 128) or holds ms * A in {64, 65}
    "mv_A16_m8_8": ("mvreg", 16, 66, ((4, 8, 4, 4), (4, 8, 4, 4)), [dict(nk=(3, 3), ms=(3, 3), nd=(2, 2), values=v)
                                                                   for v in ((8, 8), (4, 8), (8, 4))]),
    "mv_A16_m8_9": ("mvreg", 16, 66, ((4, 8, 4, 4), (4, 9, 4, 4)), [dict(nk=(3, 3), ms=(3, 3), nd=(2, 2), values=v)
                                                                   for v in ((8, 9), (4, 8), (8, 4))]),
    "mv_A16_m9_8": ("mvreg", 16, 66, ((4, 9, 4, 4), (4, 8, 4, 4)), [dict(nk=(3, 3), ms=(3, 3), nd=(2, 2), values=v)
                                                                   for v in ((9, 8), (4, 8), (8, 4))]),
    "mv_A64_m2": ("mvreg", 64, 66, ((4, 2, 4, 4), (4, 2, 4, 4)), [dict(nk=(3, 3), ms=(1, 1), nd=(2, 2), values=v)
                                                                 for v in ((2, 2), (1, 2), (2, 1))]),
    "mv_A64_m3": ("mvreg", 64, 60, ((4, 3, 4, 4), (4, 3, 4, 4)), [dict(nk=(3, 3), ms=(2, 2), nd=(2, 2), values=v)
                                                                 for v in ((3, 3), (1, 2), (2, 1))]),
    "mv_A1_m128": ("mvreg", 1, 66, ((4, 128, 4, 4), (4, 128, 4, 4)), [dict(nk=(2, 2), ms=(2, 2), nd=(1, 1), values=v)
                                                                     for v in ((128, 128), (64, 65), (65, 64))]),
    # the deferred stage: used clocks x set capacity = 128 (staged) | 129, the first value past it (not staged)
    "mv_md_stage": ("mvreg", 16, 90, ((4, 2, 16, 8), (4, 2, 16, 9)), [dict(nk=(3, 3), ms=(2, 2), nd=d, set_max=8)
                                                                     for d in ((16, 0), (7, 8), (15, 1))]),
    "mv_keys_64": ("mvreg", 16, 90, ((65, 2, 4, 4), (65, 2, 4, 4)), [dict(nk=k, ms=(2, 2), nd=(2, 2))
                                                                    for k in ((63, 64), (64, 65), (65, 63))]),
    "mv_def_64": ("mvreg", 16, 40, ((4, 2, 64, 2), (4, 2, 64, 2)),
                  [dict(nk=(3, 3), ms=(2, 2), nd=(64, 64), share_def=False)]),
    "mv_vals_128": ("mvreg", 16, 40, ((2, 128, 2, 2), (2, 128, 2, 2)),
                    [dict(nk=(1, 1), ms=(1, 1), nd=(1, 1), values=(128, 128), disjoint_values=True, same_keys=True)]),
    # Map<Orswot>: the workspace within one member of 64 KB and full (so the map deferred sets cannot be staged);
    # the map deferred sets staged; past kMoStageMax; 63 / 64 / 65 keys; 64 | 65 actors
    "mo_full_ws": ("orswot", 16, 40, (MO_FULL, MO_FULL), [dict(nk=(3, 3), nd=(2, 2), full=True)]),
    "mo_staged_A64": ("orswot", 64, 90, (_mo_caps(kcap=65), _mo_caps(kcap=65)),
                      [dict(nk=k, nd=(3, 3)) for k in ((63, 64), (64, 65), (65, 63))]),
    "mo_stage_max_A65": ("orswot", 65, 60, (_mo_caps(dcap=16, scap=65), _mo_caps(dcap=16, scap=65)),
                         [dict(nk=(4, 4), nd=(12, 12))]),
    # the nested map: outer keys of each class, the outer deferred stage at 128 | 129, 63 / 64 / 65 keys, 64 | 65 actors
    "mm_md_stage_A64": ("nested", 64, 90, (((4, 16, 8), (4, 4, 4, 4)), ((4, 16, 9), (4, 4, 4, 4))),
                        [dict(nk=(3, 3), nd=d, set_max=4) for d in ((16, 0), (7, 8), (15, 1))]),
    "mm_keys_64_A65": ("nested", 65, 60, (((65, 4, 4), (4, 4, 4, 4)), ((65, 4, 4), (4, 4, 4, 4))),
                       [dict(nk=k, nd=(2, 2)) for k in ((63, 64), (64, 65), (65, 63))]),
}
PAIR = {"mvreg": mvreg_pair, "nested": nested_pair}


@functools.lru_cache(maxsize=None)
def tier_case(name):
    """-> dict: kind, A, caps, shapes, base, lifts, pairs, S, O, SO, OS (as map_edge_cases.merge_case)."""
    kind, A, n, caps, shapes = TIER_BATCHES[name]
    rng = random.Random(name)
    base = []
    for i in range(n):
        kw = shapes[i % len(shapes)]
        base.append(orswot_pair(rng, A, caps, **kw) if kind == "orswot" else PAIR[kind](rng, A, **kw))
    lifts = ml.draw_lifts(0x71E7, [((x, y), None, ()) for x, y in base], kind)
    pairs = [(ml.lift_map(x, f), ml.lift_map(y, f)) for (x, y), f in zip(base, lifts)]
    S, O = mc.pack(kind, [p[0] for p in pairs], A, caps[0]), mc.pack(kind, [p[1] for p in pairs], A, caps[1])
    return dict(kind=kind, A=A, caps=caps, base=base, lifts=lifts, pairs=pairs, S=S, O=O,
                SO=oracle_merge(kind, S, O, A), OS=oracle_merge(kind, O, S, A))


def oracle_merge(kind, S, O, A):
    """The entry point's own oracle, for sides of different capacities."""
    if kind != "nested":
        return mc.oracle_merge(kind, S, O, A, None)
    out = []
    for x, y in zip(mc.unpack(kind, S), mc.unpack(kind, O)):
        x.merge(y)
        out.append(x)
    caps = (tuple(a + b for a, b in zip((S.kcap, S.dcap, S.scap), (O.kcap, O.dcap, O.scap))),
            tuple(a + b for a, b in zip(S.inner_caps, O.inner_caps)))
    return mc.pack(kind, out, A, caps)


def census(name):
    """The tier counts of a batch, per orientation: [Counter, Counter]."""
    c = tier_case(name)
    kind, A = c["kind"], c["A"]
    out = []
    for X, Y, R in ((c["S"], c["O"], c["SO"]), (c["O"], c["S"], c["OS"])):
        n = collections.Counter()
        a, b = X.a, Y.a
        for i in range(len(c["pairs"])):
            n["keys_%d_%d" % (a["n_keys"][i], b["n_keys"][i])] += 1
            n["keys_" + ml.key_window(int(a["n_keys"][i])) + "_" + ml.key_window(int(b["n_keys"][i]))] += 1
            n["out_def_%d" % R.a["n_def"][i]] += 1
            if kind == "mvreg":
                n[ml.tier_mvreg(A, X.mcap, Y.mcap)] += 1
                sz = int(a["n_def"][i]) * X.scap + int(b["n_def"][i]) * Y.scap
                n["md_%d" % sz if sz in (127, 128, 129) else "md_staged" if sz <= ml.MD_STAGE else "md_unstaged"] += 1
                n["rows_%d_%d" % (int(a["mv_n"][i].max()) * A, int(b["mv_n"][i].max()) * A)] += 1
                n["out_vals_%d" % R.a["mv_n"][i].max()] += 1
            elif kind == "nested":
                sz = int(a["n_def"][i]) * X.scap + int(b["n_def"][i]) * Y.scap
                n["md_%d" % sz if sz in (127, 128, 129) else "md_staged" if sz <= ml.MM_STAGE else "md_unstaged"] += 1
            else:
                n[ml.tier_orswot(X.caps, Y.caps, A)] += 1
                n["out_mem_%d" % R.a["vn_mem"][i].max()] += 1
                n["out_vdef_%d" % R.a["vn_def"][i].max()] += 1
                n["out_vset_%d" % R.a["vdset_n"][i].max()] += 1
        if kind == "nested":
            flip = X is c["O"]
            for x, y in c["pairs"]:
                got = nested_key_classes(*((y, x) if flip else (x, y)))
                for cl in got:
                    n[cl] += 1  # objects holding a key of the class
        out.append(n)
    return out


# batch -> the census entries that must hold FLOOR objects (in both orientations; "a|b": either spelling, the
# orientation swaps the sides)
EXPECT = {
    "mv_A16_m8_8": ["value_stage", "rows_128_128", "rows_64_128|rows_128_64"],
    "mv_A16_m8_9": ["plain", "rows_128_144|rows_144_128", "rows_64_128|rows_128_64"],
    "mv_A16_m9_8": ["plain", "rows_144_128|rows_128_144"],
    "mv_A64_m2": ["value_stage", "rows_128_128", "rows_64_128|rows_128_64"],
    "mv_A64_m3": ["plain", "rows_192_192"],
    "mv_A1_m128": ["value_stage", "rows_128_128", "rows_64_65|rows_65_64"],
    "mv_md_stage": ["md_128", "md_129"],
    "mv_keys_64": ["keys_63_64|keys_64_63", "keys_64_65|keys_65_64", "keys_65_63|keys_63_65",
                   "keys_registers_slab|keys_slab_registers", "keys_registers_registers"],
    "mv_def_64": ["out_def_128"],
    "mv_vals_128": ["out_vals_256"],
    "mo_full_ws": [(1, "unstaged_lds"), "out_mem_%d" % (2 * MO_FULL["mcap"]), "out_vdef_%d" % (2 * MO_FULL["vdcap"]),
                   "out_vset_%d" % (2 * MO_FULL["vscap"])],
    "mo_staged_A64": [(1, "staged"), "keys_63_64|keys_64_63", "keys_64_65|keys_65_64", "keys_65_63|keys_63_65"],
    "mo_stage_max_A65": [(2, "unstaged_stage_max")],
    "mm_md_stage_A64": ["md_128", "md_129", "self_only", "other_only", "both_plain", "both_truncated"],
    "mm_keys_64_A65": ["keys_63_64|keys_64_63", "keys_64_65|keys_65_64", "keys_65_63|keys_63_65", "self_only",
                       "other_only", "both_plain", "both_truncated"],
}


def assert_tiers(name):
    got = census(name)
    for n in got:
        for want in EXPECT[name]:
            alts = want.split("|") if isinstance(want, str) else [want]
            assert sum(n[a] for a in alts) >= FLOOR, (name, want, dict(n))
    if name == "mo_full_ws":  # within one member of the limit
        assert ml.tier_orswot(dict(MO_FULL, mcap=MO_FULL["mcap"] + 1), MO_FULL, 16) == "einval"
    return got
