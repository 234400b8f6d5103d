"""Test helper: monotone lifts, deliberately wrong comparisons and censuses
for the Map merge, truncate and apply kernels (Map<u64, MVReg>, Map<u64,
Orswot>, Map<u64, Map<u64, MVReg>>). Needs no GPU.

Every counter use on those paths is order-only (max, min, >=, ==, subtract to
absent, CLOCK ORDER), so for a map that is strictly increasing per (object,
actor) with 0 -> 0, op(lift(x)) == lift(op(x)); the same holds for a strictly
increasing relabelling of the map keys, of the Orswot members and of the
nested map's inner keys, and for an injective relabelling of the MVReg
values. The op-simulation generators (oracle map_generate, nested_gen,
map_opgen, map_orswot_opgen, nested_opgen, map_truncgen) keep making the
states; a Lift then moves every comparison onto a u64 edge.

A Lift is rank-based: per object and actor it collects the distinct counters
of the whole case (both states, the op list, the truncating clock) and maps
the j-th smallest to the j-th element of an increasing image (CTR_KINDS); keys
likewise per object (KEY_KINDS), one table for the map keys and the deferred
key sets that name them, one for the Orswot members, one for the inner keys.

Two forms: on crdts_ref objects and literal ops (lift_map, lift_ops_*), and on
the arrays of a host slab (lift_slab, by the role tables SLAB_ROLES).

mutant() patches crdts_ref.VClock's comparisons into wrong ones, key_walk()
restates the kernels' sorted key walk with wrong compares, clock_order_census()
counts how the CLOCK ORDER of an output's deferred list was decided, and
tier_mvreg() / deferred_staged() / key_window() / tier_orswot() restate the
merge launchers' rules."""
import contextlib
import random

import numpy as np

from map_slab import crdts_ref
from mvreg_pairgen import EDGE

M64 = 2**64 - 1
VC = crdts_ref.VClock
CTR_KINDS = ("id", "around32", "around63", "top", "hi_only", "hi_up_lo_down", "edge_sample")
KEY_KINDS = ("ends", "ends", "low_word", "high_word", "mid63", "id")
EDGE_TOP = tuple(sorted(set(EDGE) | {M64}))
VAL_TOP = 0xA5 << 56


# ------------------------------------------------------------------ images
def ctr_image(kind, m, rng, vs=None):
    """The increasing image of m distinct nonzero counters (vs: the counters, for "id")."""
    if kind == "edge_sample" and m > len(EDGE_TOP):
        kind = "hi_only"
    if kind == "id":
        return list(vs)
    if kind in ("around32", "around63"):
        E = 2**32 if kind == "around32" else 2**63
        if m == 1:
            return [rng.choice((E - 1, E))]
        p = rng.randrange(m - 1)  # rank p -> E - 1, rank p + 1 -> E
        return [E - 1 + (j - p) for j in range(m)]
    if kind == "top":
        return [M64 - (m - 1 - j) for j in range(m)]
    if kind == "hi_only":
        return [(j + 1) << 32 for j in range(m)]
    if kind == "hi_up_lo_down":
        return [((j + 1) << 32) | (m - j) for j in range(m)]
    if kind == "edge_sample":
        return sorted(rng.sample(EDGE_TOP, m))
    raise ValueError(kind)


def key_image(kind, m, rng, vs=None):
    """The increasing image of m distinct keys: 0 and 2^64 - 1 ("ends", with
    2^63 - 1 next to 2^63 between them), keys equal in the low word (x,
    x + 2^32, ...), keys equal in the high word, keys around 2^63."""
    if kind == "id":
        return list(vs)
    if kind == "ends":
        if m == 1:
            return [rng.choice((0, M64))]
        return [0] + [2**63 - 2 + j for j in range(1, m - 1)] + [M64]
    if kind == "low_word":
        return [((j + 1) << 32) | 9 for j in range(m)]
    if kind == "high_word":
        return [(0x80000001 << 32) | (j + 1) for j in range(m)]
    if kind == "mid63":
        p = rng.randrange(max(1, m - 1))
        return [2**63 - 1 + (j - p) for j in range(m)]
    raise ValueError(kind)


# ------------------------------------------------------------------ object form
class Record:
    """The identity, recording what it is asked for."""

    def __init__(self):
        self.ctrs, self.keys, self.mems, self.keys2 = {}, set(), set(), set()

    def ctr(self, a, c):
        if c:
            self.ctrs.setdefault(a, set()).add(c)
        return c

    def key(self, k):
        self.keys.add(k)
        return k

    def mem(self, x):
        self.mems.add(x)
        return x

    def key2(self, k):
        self.keys2.add(k)
        return k

    def val(self, v):
        return v


class Lift:
    """One object's tables. kinds: {"ctr": {actor: kind}, "key": kind, ...} as drawn."""

    def __init__(self, rec, rng, flip_val, identity=False):
        self.kinds = {"ctr": {}}
        self.c = {}
        for a in sorted(rec.ctrs):
            vs = sorted(rec.ctrs[a])
            kind = "id" if identity else rng.choice(CTR_KINDS)
            self.kinds["ctr"][a] = kind
            self.c[a] = dict(zip(vs, ctr_image(kind, len(vs), rng, vs)))
        self.t = {}
        for role, vals in (("key", rec.keys), ("mem", rec.mems), ("key2", rec.keys2)):
            vs = sorted(vals)
            kind = "id" if identity else rng.choice(KEY_KINDS)
            self.kinds[role] = kind
            self.t[role] = dict(zip(vs, key_image(kind, len(vs), rng, vs)))
        self.flip = flip_val and not identity

    def ctr(self, a, c):
        return self.c[a][c] if c else 0

    def key(self, k):
        return self.t["key"][k]

    def mem(self, x):
        return self.t["mem"][x]

    def key2(self, k):
        return self.t["key2"][k]

    def val(self, v):
        return v ^ VAL_TOP if self.flip else v


def _clock(c, f):
    v = VC()
    v.dots = {a: f.ctr(a, n) for a, n in c.dots.items()}
    return v


def lift_clock(c, f):
    return _clock(c, f)


def lift_map(m, f, depth=0):
    """A copy of map `m` (any value kind) with every counter, key, member,
    inner key and value sent through `f` (a Lift, or a Record to collect
    them). Dict and Vec orders are kept. Modelled on map_slab.relabel."""
    kf = f.key if depth == 0 else f.key2
    r = crdts_ref.Map(m.factory, m.order)
    r.clock = _clock(m.clock, f)
    for k, (c, v) in m.entries.items():
        if isinstance(v, crdts_ref.Map):
            o = lift_map(v, f, depth + 1)
        elif isinstance(v, crdts_ref.Orswot):
            o = crdts_ref.Orswot()
            o.clock = _clock(v.clock, f)
            o.entries = {f.mem(x): _clock(e, f) for x, e in v.entries.items()}
            o.deferred = {_clock(d, f): {f.mem(x) for x in s} for d, s in v.deferred.items()}
        else:
            o = crdts_ref.MVReg()
            o.vals = [(_clock(cc, f), f.val(val)) for cc, val in v.vals]
        r.entries[kf(k)] = [_clock(c, f), o]
    r.deferred = {_clock(d, f): {kf(k) for k in s} for d, s in m.deferred.items()}
    return r


def _pairs(pairs, f):
    return [(a, f.ctr(a, c)) for a, c in pairs]


def lift_ops_mvreg(ops, f):
    """map_opgen's op tuples."""
    out = []
    for op in ops:
        if op[0] == "up":
            _, a, c, key, pairs, val = op
            out.append(("up", a, f.ctr(a, c), f.key(key), _pairs(pairs, f), f.val(val)))
        elif op[0] == "rm":
            out.append(("rm", f.key(op[1]), _pairs(op[2], f)))
        else:
            out.append(op)
    return out


def lift_ops_orswot(ops, f):
    """map_orswot_opgen's op tuples."""
    out = []
    for op in ops:
        if op[0] == "up_add":
            _, a, c, key, x = op
            out.append(("up_add", a, f.ctr(a, c), f.key(key), f.mem(x)))
        elif op[0] == "up_rm":
            _, a, c, key, x, pairs = op
            out.append(("up_rm", a, f.ctr(a, c), f.key(key), f.mem(x), _pairs(pairs, f)))
        elif op[0] == "rm":
            out.append(("rm", f.key(op[1]), _pairs(op[2], f)))
        else:
            out.append(op)
    return out


def lift_ops_nested(ops, f):
    """The nested map's literal ops (crdts_hip.MapMapOps' JSON form)."""
    lp = lambda ps: [[a, f.ctr(a, c)] for a, c in ps]  # noqa: E731
    dot = lambda d: [d[0], f.ctr(d[0], d[1])]  # noqa: E731

    def inner(op):
        if op == "nop":
            return op
        if "rm" in op:
            return {"rm": {"clock": lp(op["rm"]["clock"]), "key": f.key2(op["rm"]["key"])}}
        up, put = op["up"], op["up"]["op"]["put"]
        return {"up": {"dot": dot(up["dot"]), "key": f.key2(up["key"]),
                       "op": {"put": {"clock": lp(put["clock"]), "val": f.val(put["val"])}}}}

    out = []
    for op in ops:
        if op == "nop":
            out.append(op)
        elif "rm" in op:
            out.append({"rm": {"clock": lp(op["rm"]["clock"]), "key": f.key(op["rm"]["key"])}})
        else:
            up = op["up"]
            out.append({"up": {"dot": dot(up["dot"]), "key": f.key(up["key"]), "op": inner(up["op"])}})
    return out


LIFT_OPS = {"mvreg": lift_ops_mvreg, "orswot": lift_ops_orswot, "nested": lift_ops_nested}


def draw_lifts(seed, cases, kind, identity=False):
    """cases[i] = (maps, op list or None, clocks): everything object i's case
    holds -> its Lift (values get their top byte set in the odd objects)."""
    rng = random.Random(seed)
    out = []
    for i, (maps, ops, clocks) in enumerate(cases):
        rec = Record()
        for m in maps:
            lift_map(m, rec)
        if ops is not None:
            LIFT_OPS[kind](ops, rec)
        for c in clocks:
            _clock(c, rec)
        out.append(Lift(rec, rng, bool(i & 1), identity))
    return out


# ------------------------------------------------------------------ slab form
# field -> role: "ctr" a clock row [.., A]; "key" / "mem" / "val" with the field holding its count per slot
SLAB_ROLES = {
    "mvreg": {"clock": "ctr", "eclock": "ctr", "mv_clock": "ctr", "dclock": "ctr", "keys": "key", "dset": "key",
              "mv_val": "val"},
    "orswot": {"clock": "ctr", "eclock": "ctr", "vclock": "ctr", "vmclock": "ctr", "vdclock": "ctr", "dclock": "ctr",
               "keys": "key", "dset": "key", "vmem": "mem", "vdset": "mem"},
    "nested": {"clock": "ctr", "eclock": "ctr", "dclock": "ctr", "keys": "key", "dset": "key"},
}
# the nested map's inner MapSlab: row r belongs to outer object r // kcap; its keys are the inner keys
INNER_ROLES = {"clock": "ctr", "eclock": "ctr", "mv_clock": "ctr", "dclock": "ctr", "keys": "key2", "dset": "key2",
               "mv_val": "val"}


def _lift_arrays(arrays, masks, roles, lifts, obj_of_row):
    out = {}
    for f, v in arrays.items():
        role = roles.get(f)
        if role is None:
            out[f] = v.copy()
            continue
        w = np.zeros_like(v)
        used = np.ones(v.shape, bool) if role == "ctr" else masks[f]
        for idx in zip(*np.nonzero(used if role != "ctr" else v != 0)):
            L = lifts[obj_of_row(idx[0])]
            x = int(v[idx])
            w[idx] = L.ctr(idx[-1], x) if role == "ctr" else getattr(L, role)(x)
        out[f] = w
    return out


def lift_slab(kind, S, lifts):
    """A host slab (canonical: unused slots zero) with every array sent
    through the objects' lifts by the role tables above -> a new host slab."""
    import crdts_hip

    S = S.canonical()
    if kind == "mvreg":
        return crdts_hip.MapSlab(_lift_arrays(S.a, S.used_masks(), SLAB_ROLES[kind], lifts, lambda r: r),
                                 S.kcap, S.mcap, S.dcap, S.scap)
    if kind == "orswot":
        return crdts_hip.MapOrswotSlab(_lift_arrays(S.a, S.used_masks(), SLAB_ROLES[kind], lifts, lambda r: r), S.caps)
    a = S.a
    dfr = np.arange(S.dcap)[None, :] < a["n_def"][:, None]
    masks = {"keys": np.arange(S.kcap)[None, :] < a["n_keys"][:, None],
             "dset": dfr[..., None] & (np.arange(S.scap)[None, None, :] < a["dset_n"][..., None])}
    inner = crdts_hip.MapSlab(_lift_arrays(S.inner.a, S.inner.used_masks(), INNER_ROLES, lifts, lambda r: r // S.kcap),
                              *S.inner_caps)
    return crdts_hip.MapMapSlab(_lift_arrays(a, masks, SLAB_ROLES[kind], lifts, lambda r: r), S.kcap, S.dcap, S.scap,
                                inner)


def lift_clock_rows(rows, lifts):
    """The truncating clock rows u64 [n][A] through the objects' lifts."""
    out = np.zeros_like(rows)
    for i, a in zip(*np.nonzero(rows)):
        out[i, a] = lifts[i].ctr(a, int(rows[i, a]))
    return out


# ------------------------------------------------------------------ wrong comparisons
def _low32(c):
    return c & 0xFFFFFFFF


def _high32(c):
    return c >> 32


def _signed(c):
    return c - 2**64 if c >= 2**63 else c


COMPARE_KEYS = {"counter_compare_low32": _low32, "counter_compare_high32": _high32, "counter_compare_signed": _signed}
VCLOCK_MUTANTS = tuple(COMPARE_KEYS) + ("subtract_strict", "deferred_kept_on_equal", "intersection_ignores_counter",
                                        "high_slot_blind")


@contextlib.contextmanager
def mutant(knob):
    """crdts_ref.VClock with one comparison made wrong, while the block runs:
    counter_compare_low32 / _high32 / _signed  every counter compare (witness,
        partial_cmp, intersection, subtract) looks at that part of the counters;
    subtract_strict  a dot equal to the subtracted clock's survives;
    deferred_kept_on_equal  `d <= c` is `d < c` (a remove whose clock equals
        the map's stays deferred);
    intersection_ignores_counter  a shared actor is common whatever its counters;
    high_slot_blind  partial_cmp and subtract do not see actors >= 64.
    None: unpatched."""
    if knob is None:
        yield
        return
    names = ("witness", "partial_cmp", "intersection", "subtract", "__le__")
    saved = {n: getattr(VC, n) for n in names}
    k = COMPARE_KEYS.get(knob, lambda c: c)
    seen = (lambda a: a < 64) if knob == "high_slot_blind" else (lambda a: True)

    def witness(self, a, c):
        if not (k(self.get(a)) >= k(c)):
            self.dots[a] = c

    def partial_cmp(self, other):
        acts = [a for a in set(self.dots) | set(other.dots) if seen(a)]
        ge = all(k(self.get(a)) >= k(other.get(a)) for a in acts)
        le = all(k(other.get(a)) >= k(self.get(a)) for a in acts)
        return 0 if ge and le else 1 if ge else -1 if le else None

    def intersection(self, other):
        v = VC()
        if knob == "intersection_ignores_counter":
            v.dots = {a: c for a, c in self.dots.items() if a in other.dots}
        else:
            v.dots = {a: c for a, c in self.dots.items() if k(other.get(a)) == k(c)}
        return v

    def subtract(self, other):
        for a, c in other.dots.items():
            if not seen(a):
                continue
            if (k(c) > k(self.get(a))) if knob == "subtract_strict" else (k(c) >= k(self.get(a))):
                self.dots.pop(a, None)

    def le(self, other):
        return self.partial_cmp(other) in ((-1,) if knob == "deferred_kept_on_equal" else (0, -1))

    try:
        for n, fn in zip(names, (witness, partial_cmp, intersection, subtract, le)):
            setattr(VC, n, fn)
        yield
    finally:
        for n, fn in saved.items():
            setattr(VC, n, fn)


def changed(knob, run, expected):
    """Does the wrong comparison change run()'s answer (or make it raise)?"""
    try:
        with mutant(knob):
            got = run()
    except Exception:  # noqa: BLE001
        return True
    return got.canonical() != expected.canonical()


KEY_MUTANTS = ("key_order_signed", "key_equal_on_low_word", "key_compare_high32", "key_all_ones_is_absent")


def key_walk(ks, ko, knob=None):
    """The kernels' walk over two sorted key arrays (map.hip, map_orswot.hip,
    map_map.hip: an exhausted side reads as 2^64 - 1 and is guarded by its
    index) -> [(key, from self, from other)]; `knob` makes it wrong."""
    cv = {"key_order_signed": _signed, "key_compare_high32": _high32}.get(knob, lambda x: x)
    if knob == "key_equal_on_low_word":
        le = lambda x, y: x <= y or _low32(x) == _low32(y)  # noqa: E731
    else:
        le = lambda x, y: cv(x) <= cv(y)  # noqa: E731
    absent = knob == "key_all_ones_is_absent"
    a = b = 0
    out = []
    while True:
        ha = a < len(ks) and not (absent and ks[a] == M64)
        hb = b < len(ko) and not (absent and ko[b] == M64)
        if not (ha or hb):
            return out
        ka, kb = ks[a] if ha else M64, ko[b] if hb else M64
        hs, ho = ha and (not hb or le(ka, kb)), hb and (not ha or le(kb, ka))
        out.append((ka if hs else kb, hs, ho))
        a, b = a + hs, b + ho


# ------------------------------------------------------------------ censuses
ORDER_CLASSES = ("high_word", "low_word", "actor_ge_64", "prefix_other_slot")


def clock_order_census(rows):
    """rows: one object's output deferred clocks, dense u64 [nd][A] -> the set
    of ORDER_CLASSES some pair of them is ordered by: at the first actor where
    two rows differ, by counters that differ only in the high word / only in
    the low word; at an actor >= 64; or by the prefix rule (one side lacks
    that actor) where the lacking side holds the lane's other actor, a + 64."""
    got = set()
    A = rows.shape[1] if len(rows) else 0
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            d = np.nonzero(rows[i] != rows[j])[0]
            if not d.size:
                continue
            a = int(d[0])
            x, y = int(rows[i, a]), int(rows[j, a])
            if a >= 64:
                got.add("actor_ge_64")
            if x and y:
                if _low32(x) == _low32(y):
                    got.add("high_word")
                if _high32(x) == _high32(y):
                    got.add("low_word")
            elif a + 64 < A and int((rows[i] if not x else rows[j])[a + 64]):
                got.add("prefix_other_slot")
    return got


# ------------------------------------------------------------------ launch tiers
# The merge launchers' rules restated (rust-crdt_amd/csrc/map.hip, map_orswot.hip, map_map.hip), as
# orswot_pairgen.tier does for the join: a launcher change that re-routes a shape fails the census of its batch.
VS_ROWS, MD_STAGE, MM_STAGE, KEY_WINDOW = 128, 128, 128, 64
MO_LDS_MAX, MO_STAGE_MAX = 65536, 16384


def tier_mvreg(A, mcap_s, mcap_o):
    """launch_map_mvreg_merge: "two_slots" past 64 actors, else "value_stage"
    when both sides' value rows fit the stage (mcap * A <= 128), else "plain"."""
    if A > 64:
        return "two_slots"
    return "value_stage" if mcap_s * A <= VS_ROWS and mcap_o * A <= VS_ROWS else "plain"


def deferred_staged(nd_s, scap_s, nd_o, scap_o, stage=MD_STAGE):
    """map_mvreg_merge_kernel / map_map_outer_kernel, per object: the map
    deferred sets are staged when used clocks x set capacity fit the stage."""
    return nd_s * scap_s + nd_o * scap_o <= stage


def key_window(n_keys):
    """Keys past the first 64 are read from the slab, not from the lanes' registers."""
    return "registers" if n_keys <= KEY_WINDOW else "slab"


def orswot_lds_bytes(S, O, A):
    """map_orswot_lds_bytes over two capacity dicts."""
    per = lambda m, d, s: 8 * (m + m * A + d * A + d * s)  # noqa: E731
    MW, DW, SW = S["mcap"] + O["mcap"], S["vdcap"] + O["vdcap"], S["vscap"] + O["vscap"]
    return (per(S["mcap"], S["vdcap"], S["vscap"]) + per(O["mcap"], O["vdcap"], O["vscap"]) + per(MW, DW, SW)
            + 8 * ((MW + DW + 1) // 2) + 8 * ((3 * (S["dcap"] + O["dcap"]) + 2 * DW + 1) // 2))


def tier_orswot(S, O, A):
    """launch_map_orswot_merge over two capacity dicts -> (actor slots per
    lane, how the map deferred sets are read): "staged", "unstaged_stage_max"
    (past kMoStageMax), "unstaged_lds" (workspace + stage past 64 KB);
    "einval" when the workspace alone is past 64 KB."""
    lds = orswot_lds_bytes(S, O, A)
    if lds > MO_LDS_MAX:
        return "einval"
    md = 8 * (S["dcap"] * S["scap"] + O["dcap"] * O["scap"])
    how = "unstaged_stage_max" if md > MO_STAGE_MAX else "unstaged_lds" if lds + md > MO_LDS_MAX else "staged"
    return (2 if A > 64 else 1, how)


def key_census(keys):
    """What a sorted key list shows: its classes among "zero", "all_ones",
    "low_word_pair", "high_word_pair", "around_2_63"."""
    got = set()
    ks = [int(k) for k in keys]
    if 0 in ks:
        got.add("zero")
    if M64 in ks:
        got.add("all_ones")
    for x, y in zip(ks, ks[1:]):
        if _low32(x) == _low32(y):
            got.add("low_word_pair")
        if _high32(x) == _high32(y):
            got.add("high_word_pair")
        if x < 2**63 <= y:
            got.add("around_2_63")
    return got
