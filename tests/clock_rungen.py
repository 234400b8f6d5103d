"""Test helper: edge inputs for the sparse (CSR) clock kernels — the merge
(rust-crdt_amd/csrc/csr_merge.hip) and the filters, apply, value and get of
rust-crdt_amd/csrc/clock_ops.hip. Runs are built directly, not drawn: lengths
on both sides of the 64-entry register tier and of its chunks, actors from a
universe that straddles 2^31 (0, 1, 2^31 - 1, 2^31, 2^31 + 1, 2^32 - 2, 2^32 - 1,
pairs that differ only in bit 31 or only in the low 16 bits), the shared
actors at index 0, 63, 64 and last of both runs, and counters on shared actors
below / equal / one above each other across 2^32, 2^63 and up to 2^64 - 1.

The references are plain dicts; ref_*() restate the kernels' walk (an entry's
rank in the other run by binary search, then the compare) with knobs that make
them wrong in one way each (MUTANTS): what the batches must tell apart. Every
batch is made once and is read-only by convention (tuples of tuples)."""
import bisect
import functools
import random

import mvreg_pairgen as pg

M64 = 2**64 - 1
AMAX = 2**32 - 1
LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129, 700)
SPECIAL = (0, 1, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2, 2**32 - 1)
LOWS = (0x0001, 0x8000, 0xFFFF)
HIGHS = tuple(range(0x0100, 0x0100 + 365)) + tuple(range(0x8100, 0x8100 + 365))  # h and h | 0x8000: bit 31 apart
# the counters of a shared actor (smaller, larger): one apart across a word edge, or apart in one word only
PAIRS = tuple((lo, hi) for lo, hi in pg.CMP_PAIRS if lo) + tuple((e, e + 1) for e in pg.EDGE) + (
    (5, 2**32 + 5), (2**32 + 7, 2**33 + 7), (2**63 + 9, 2**63 + 2**32 + 9), (2**32 + 1, 2**32 + 2), (M64 - 1, M64),
    (2**33 + 4, 2**63 + 3))


@functools.lru_cache(maxsize=None)
def universe():
    """Sorted actors: the special ones and the grid (h << 16) | l."""
    return tuple(sorted(set(SPECIAL) | {(h << 16) | l for h in HIGHS for l in LOWS}))


def _counter(rng):
    return rng.choice(pg.EDGE + (M64, M64 - 1, rng.randrange(1, 2**62)))


def _side(rng, L, i0, i63, ilast):
    """U indices of a run of L entries: the anchors i0, i63, i63 + 1 and ilast
    sit at index 0, 63, 64 and last whenever the run reaches them."""
    between, after = range(i0 + 1, i63), range(i63 + 2, ilast)
    if L == 0:
        return []
    if L == 1:
        return [rng.choice([i0, ilast])]
    if L <= 63:
        k = rng.randint(0, min(L - 2, len(between)))
        return [i0] + sorted(rng.sample(between, k) + rng.sample(after, L - 2 - k)) + [ilast]
    run = [i0] + sorted(rng.sample(between, 62)) + [i63]
    if L >= 65:
        run.append(i63 + 1)
    if L >= 66:
        run += sorted(rng.sample(after, L - 66)) + [ilast]
    return run


def pair(rng, Ls, Lo, region=None):
    """-> (self run, other run): sorted (actor, counter) lists. region 0 / 1 /
    2 (default: drawn): the first 65 entries lie below 2^31 / astride it / at
    and above it."""
    U = universe()
    m = bisect.bisect_left(U, 2**31)
    i0 = (0, m - 40, m)[rng.randrange(3) if region is None else region] + rng.randrange(0, 4)
    i63 = i0 + 1 + rng.randrange(130, 260)
    ilast = len(U) - 1 - rng.randrange(0, 3)
    s, o = _side(rng, Ls, i0, i63, ilast), _side(rng, Lo, i0, i63, ilast)
    cs, co = {}, {}
    for k in set(s) & set(o):
        lo, hi = rng.choice(PAIRS)
        cs[k], co[k] = rng.choice([(hi, hi), (lo, lo), (lo, hi), (hi, lo), (lo, hi), (hi, lo)])
    return ([(U[k], cs.get(k) or _counter(rng)) for k in s], [(U[k], co.get(k) or _counter(rng)) for k in o])


@functools.lru_cache(maxsize=None)
def pair_batch(seed=0x0C5B, reps=3):
    """Every pair of LENGTHS, `reps` times -> (S, O): tuples of runs."""
    rng = random.Random(seed)
    S, O = [], []
    for rep in range(reps):
        for Ls in LENGTHS:
            for Lo in LENGTHS:
                s, o = pair(rng, Ls, Lo, (len(S) + rep) % 3)  # every length pair in every region
                S.append(tuple(s))
                O.append(tuple(o))
    return tuple(S), tuple(O)


def placements(S, O):
    """Census: objects whose runs share the actor at index 0 / 63 / 64 / last
    of both runs; by tier (both in registers, either long, both long); shared
    actors by counter relation; objects holding actors on both sides of 2^31;
    the 64-entry runs by where their actors at or above 2^31 sit."""
    c = dict(idx0=0, idx63=0, idx64=0, last=0, regs=0, one_long=0, both_long=0, below=0, equal=0, above=0,
             straddle=0, absent_self=0, absent_other=0, run64_high_lane0=0, run64_high_lane63=0, run64_straddle=0)
    for s, o in zip(S, O):
        for name, k in (("idx0", 0), ("idx63", 63), ("idx64", 64)):
            c[name] += len(s) > k and len(o) > k and s[k][0] == o[k][0]
        c["last"] += bool(s) and bool(o) and s[-1][0] == o[-1][0]
        longs = (len(s) > 64) + (len(o) > 64)
        c[("regs", "one_long", "both_long")[longs]] += 1
        ds, do = dict(s), dict(o)
        for a in ds.keys() & do.keys():
            c["below" if ds[a] < do[a] else "equal" if ds[a] == do[a] else "above"] += 1
        c["absent_other"] += len(ds.keys() - do.keys())
        c["absent_self"] += len(do.keys() - ds.keys())
        acts = [a for a, _ in s] + [a for a, _ in o]
        c["straddle"] += bool(acts) and min(acts) < 2**31 <= max(acts)
        for r in (s, o):  # the 64-entry register runs: actors at or above 2^31 at lane 0, at lane 63, from some lane on
            if len(r) == 64:
                c["run64_high_lane0"] += r[0][0] >= 2**31
                c["run64_high_lane63"] += r[63][0] >= 2**31
                c["run64_straddle"] += r[0][0] < 2**31 <= r[63][0]
    return c


# ------------------------------------------------------- plain references
def merge_dict(s, o):
    d = dict(s)
    for a, c in o:
        d[a] = max(d.get(a, 0), c)
    return sorted(d.items())


def filter_dict(op, s, o):
    od = dict(o)
    if op == "truncate":
        return [(a, min(c, od[a])) for a, c in s if a in od]
    if op == "subtract":
        return [(a, c) for a, c in s if not od.get(a, 0) >= c]
    return [(a, c) for a, c in s if od.get(a) == c]


def apply_dict(s, dots):
    d = dict(s)
    for a, c in dots:
        if c > d.get(a, 0):
            d[a] = c
    return sorted(d.items())


def value_of(s):
    return sum(c for _, c in s) & M64


def i64(x):
    x &= M64
    return x - 2**64 if x >= 2**63 else x


# ------------------------------------- the kernels' walk, with wrong knobs
def _ckey(compare):
    return {None: lambda c: c, "low32": lambda c: c & 0xFFFFFFFF, "high32": lambda c: c >> 32,
            "signed": i64}[compare]


def _akey(signed):
    return (lambda a: a - 2**32 if a >= 2**31 else a) if signed else (lambda a: a)


def _find(o, okeys, a, akey, low16):
    """The entry of run o that the walk takes for actor a: the one at a's rank, if its actor is a's."""
    r = bisect.bisect_left(okeys, akey(a))
    if r < len(o) and (o[r][0] == a or (low16 and (o[r][0] ^ a) & 0xFFFF == 0)):
        return o[r]
    return None


def ref_merge(s, o, compare=None, actor_order_signed=False, actor_equal_on_low16=False):
    ck, ak = _ckey(compare), _akey(actor_order_signed)
    sk, ok = [ak(a) for a, _ in s], [ak(a) for a, _ in o]
    out = []
    for a, c in s:
        e = _find(o, ok, a, ak, actor_equal_on_low16)
        out.append((a, e[1] if e and ck(e[1]) > ck(c) else c))
    out += [(a, c) for a, c in o if not _find(s, sk, a, ak, actor_equal_on_low16)]
    return sorted(out)


def ref_filter(op, s, o, compare=None, actor_order_signed=False, actor_equal_on_low16=False, subtract_strict=False,
               truncate_keeps_absent=False, intersection_ignores_counter=False):
    ck, ak = _ckey(compare), _akey(actor_order_signed)
    ok = [ak(a) for a, _ in o]
    out = []
    for a, c in s:
        e = _find(o, ok, a, ak, actor_equal_on_low16)
        if op == "truncate":
            if e or truncate_keeps_absent:
                out.append((a, e[1] if e and ck(e[1]) < ck(c) else c))
        elif op == "subtract":
            gone = e and (ck(e[1]) > ck(c) if subtract_strict else ck(e[1]) >= ck(c))
            if not gone:
                out.append((a, c))
        elif e and (intersection_ignores_counter or ck(e[1]) == ck(c)):
            out.append((a, c))
    return out


def ref_apply(s, dots, compare=None, actor_order_signed=False, actor_equal_on_low16=False,
              apply_first_dot_wins=False, zero_dot_creates_entry=False):
    """The dots of an actor stand for it by their largest counter (the first of
    equal ones); the standing dots are merged into the run."""
    ck = _ckey(compare)
    stand = {}
    for a, c in dots:
        if not c and not zero_dot_creates_entry:
            continue
        if a not in stand or (not apply_first_dot_wins and ck(c) > ck(stand[a])):
            stand[a] = c
    return ref_merge(s, sorted(stand.items()), compare, actor_order_signed, actor_equal_on_low16)


def ref_value(s, value_low32_sum=False):
    return sum(c & 0xFFFFFFFF for _, c in s) & M64 if value_low32_sum else value_of(s)


def ref_get(s, q, actor_order_signed=False, actor_equal_on_low16=False, get_absent_is_neighbour=False):
    ak = _akey(actor_order_signed)
    keys = [ak(a) for a, _ in s]
    if get_absent_is_neighbour:
        r = bisect.bisect_left(keys, ak(q))
        return s[r][1] if r < len(s) else 0
    e = _find(s, keys, q, ak, actor_equal_on_low16)
    return e[1] if e else 0


_CMP = {f"counter_compare_{k}": dict(compare=k) for k in ("low32", "high32", "signed")}
_WALK = dict(actor_order_signed=dict(actor_order_signed=True), actor_equal_on_low16=dict(actor_equal_on_low16=True))
# operation -> {mutant: knobs}
MUTANTS = {
    "merge": dict(_CMP, **_WALK),
    "truncate": dict(_CMP, **_WALK, truncate_keeps_absent=dict(truncate_keeps_absent=True)),
    "subtract": dict(_CMP, **_WALK, subtract_strict=dict(subtract_strict=True)),
    "intersection": dict(_CMP, **_WALK, intersection_ignores_counter=dict(intersection_ignores_counter=True)),
    "apply": dict(_CMP, **_WALK, apply_first_dot_wins=dict(apply_first_dot_wins=True),
                  zero_dot_creates_entry=dict(zero_dot_creates_entry=True)),
    "value": dict(value_low32_sum=dict(value_low32_sum=True)),
    "get": dict(_WALK, get_absent_is_neighbour=dict(get_absent_is_neighbour=True)),
}


# ------------------------------------------------------------------ apply
DOT_COUNTS = (0, 1, 63, 64, 65, 200)
SELF_LENGTHS = (0, 1, 63, 64, 65, 700)


def _dots(rng, s, m):
    U, keys, dots = universe(), [a for a, _ in s], []
    ds = dict(s)
    for _ in range(m):
        u = rng.random()
        if u < 0.35 and keys:  # a present actor: below / equal / above, or apart in one word only
            a = rng.choice(keys)
            c = ds[a]
            dots.append((a, rng.choice([max(c - 1, 0), c, min(c + 1, M64), c ^ (1 << 32), c ^ (1 << 63), c ^ 1])))
        elif u < 0.60 and dots:  # a repeated actor: the counter apart in the high word only, or in the low word only
            a, c = rng.choice(dots)
            dots.append((a, rng.choice([c ^ (1 << 40), c ^ (1 << 32), c ^ 2, (c + 1) & M64, c, c ^ (1 << 63)])))
        elif u < 0.70:  # a counter-0 dot
            dots.append((rng.choice(keys) if keys and rng.random() < 0.5 else rng.choice(U), 0))
        else:
            dots.append((rng.choice(SPECIAL) if rng.random() < 0.1 else rng.choice(U), _counter(rng)))
    return dots


@functools.lru_cache(maxsize=None)
def apply_batch(seed=0xA991, reps=6):
    """-> (S, P): self runs and dot lists; every (self length, dot count) pair
    `reps` times, then the named cases."""
    rng = random.Random(seed)
    U = universe()
    S, P = [], []
    for _ in range(reps):
        for ns in SELF_LENGTHS:
            for m in DOT_COUNTS:
                s = pair(rng, ns, 0)[0]
                S.append(tuple(s))
                P.append(tuple(_dots(rng, s, m)))
    for ns in (0, 63, 64, 65, 700):
        s = pair(rng, ns, 0)[0]
        free = [a for a in U if a not in dict(s)]
        own = [a for a, _ in s]
        # exactly 64 standing dots, unsorted: every lane stands, one at rank 63
        d = [(a, _counter(rng)) for a in rng.sample(free, 64 - min(20, len(own))) + rng.sample(own, min(20, len(own)))]
        rng.shuffle(d)
        S.append(tuple(s))
        P.append(tuple(d))
        # 64 dots with repeats: 40 actors
        acts = rng.sample(free, 40)
        d = [(a, _counter(rng)) for a in acts] + [(rng.choice(acts), _counter(rng)) for _ in range(24)]
        rng.shuffle(d)
        S.append(tuple(s))
        P.append(tuple(d))
        # one actor repeated, the counters apart in the high word only / the low word only; the maximum first,
        # in the middle, last
        for base, bit in ((2**32 + 5, 32), (2**63 + 2**32, 33), (7, 0), (2**63 + 8, 1)):
            for place in (0, 5, 10):
                cs = [base + (j << bit) for j in range(10)]
                top = cs.pop()
                cs.insert(place, top)
                a = rng.choice(own) if own and place == 5 else rng.choice(free)
                S.append(tuple(s))
                P.append(tuple((a, c) for c in cs))
        # counter-0 dots only; dots at actors 0 and 2^32 - 1
        S.append(tuple(s))
        P.append(tuple((a, 0) for a in rng.sample(free, 5) + own[:3]))
        S.append(tuple(s))
        P.append(((0, 2**63), (AMAX, M64), (0, 2**32), (AMAX, 1)))
    return tuple(S), tuple(P)


# ---------------------------------------------------------------- get, value
@functools.lru_cache(maxsize=None)
def get_batch(seed=0x6E7):
    """-> (S, Q): runs of 2^k - 1, 2^k and 2^k + 1 entries (k = 0..9) and, per
    run, queries for present actors, absent actors between two entries, below
    the first entry and above the last."""
    rng = random.Random(seed)
    U = universe()
    S, Q = [], []
    for k in range(10):
        for L in (2**k - 1, 2**k, 2**k + 1):
            for _ in range(2):
                idx = sorted(rng.sample(range(2, len(U) - 2), L))
                s = [(U[i], _counter(rng)) for i in idx]
                have = set(idx)
                q = [U[i] for i in rng.sample(idx, min(L, 4))]
                q += [U[i] for i in rng.sample([j for j in range(2, len(U) - 2) if j not in have], 4)]
                q += [U[0], U[1], U[-1], U[-2]]  # below the first, above the last
                if idx:
                    q += [U[idx[0]], U[idx[-1]], U[idx[0] - 1], U[idx[-1] + 1]]
                S.append(tuple(s))
                Q.append(tuple(q))
    return tuple(S), tuple(Q)


@functools.lru_cache(maxsize=None)
def value_batch():
    """The self runs of the pair batch, then sums that wrap once and twice."""
    S = list(pair_batch()[0])
    S += [((1, M64), (9, 2)), ((0, M64), (1, M64), (AMAX, M64)), ((5, 2**63), (6, 2**63)),
          ((5, 2**63), (6, 2**63), (7, 2**63), (8, 2**63), (9, 1)), tuple((a, M64) for a in range(1, 130)), ()]
    for k in range(1, 21):
        S += [((1, M64), (AMAX, k)), ((0, M64), (2**31, M64), (AMAX, k + 1))]  # 2^64 + k - 1; 2 * 2^64 + k - 1
    return tuple(S)


def differs(op, batch, knobs):
    """Objects of the batch (queries, for get) on which the walk with the knobs gives another answer."""
    if op == "merge":
        return sum(ref_merge(s, o, **knobs) != merge_dict(s, o) for s, o in zip(*batch))
    if op in ("truncate", "subtract", "intersection"):
        return sum(ref_filter(op, s, o, **knobs) != filter_dict(op, s, o) for s, o in zip(*batch))
    if op == "apply":
        return sum(ref_apply(s, p, **knobs) != apply_dict(s, p) for s, p in zip(*batch))
    if op == "value":
        return sum(ref_value(s, **knobs) != value_of(s) for s in batch)
    return sum(any(ref_get(s, x, **knobs) != dict(s).get(x, 0) for x in q) for s, q in zip(*batch))


@functools.lru_cache(maxsize=None)
def chain_batch(seed=0xC4A1):
    """merge -> subtract -> apply on the pair batch, each output the (gapped)
    input of the next -> (S, O, P, merged, filtered, applied): the dot lists
    are made against the filtered runs, their counts cycling DOT_COUNTS."""
    rng = random.Random(seed)
    S, O = pair_batch()
    merged = [merge_dict(s, o) for s, o in zip(S, O)]
    filtered = [filter_dict("subtract", m, o) for m, o in zip(merged, O)]
    P = [tuple(_dots(rng, f, DOT_COUNTS[i % len(DOT_COUNTS)])) for i, f in enumerate(filtered)]
    applied = [apply_dict(f, p) for f, p in zip(filtered, P)]
    return S, O, tuple(P), merged, filtered, applied
