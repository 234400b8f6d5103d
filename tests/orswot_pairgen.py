"""Test helper: structured Orswot pairs for CvRDT::merge (src/orswot.rs:87-157),
states and clocks for Causal::truncate (:159-172) and states and op lists for
CmRDT::apply (:61-85, :195-211, :235-243), as canonical records
(tests/records.py).

The op-simulated generators (csrc/host.cpp gen_pair / gen_replicas) draw one
40-bit base counter per actor and object and let both sides advance from it by
a few dozen, so the two counters of any comparison agree above their low bits
and a join that compares 32 bits, or compares signed, gives the same records.
Here every comparison the join makes is put on an edge on purpose: per actor
the two top-clock counters are neighbours from EDGE (smaller on either side,
or equal); a member's dot is below, equal to or above the other side's counter
for its actor; dots are shared, self-only and other-only; a deferred clock is
below, equal to or one edge step above the merged clock and names a member
whose dot it covers exactly, or whose dot lies one step past it; member keys
come from KEYS, from pairs that differ only in the high or only in the low
word, and from random draws; actor ids from the ends of the lane and mask
mappings (hot()). States are built directly as records, not by ops (an op
simulator's `counter + 1` overflows at 2^64 - 1), so they are canonical but
not necessarily reachable: tests/truncate_cases.py takes the same stance.

merge_ref() / truncate_ref() / apply_ref() restate the reference on decoded
states with every comparison point a parameter; MUTANTS / TRUNCATE_MUTANTS /
APPLY_MUTANTS name wrong settings of them: what the generated inputs must
tell apart. tier() recomputes, from the launcher's and the kernels' own
limits (csrc/orswot_merge.hip), which kernel joins an
object pair. Nothing here calls into the library."""
import operator
import random
import struct

import numpy as np

import mvreg_pairgen
import records

M32, M64 = 2**32 - 1, 2**64 - 1
EDGE = (1, 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 2, 2**64 - 1)
KEYS = (0, 1, 2**32 - 1, 2**32, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1)
# the two top-clock counters of one actor (smaller, larger; 0: absent on that side)
PAIRS = tuple(zip(EDGE, EDGE[1:])) + tuple(mvreg_pairgen.CMP_PAIRS) + ((2**32 + 1, 2**63), (2, 2**32 - 1))


def up(c):
    """The next edge counter above c (None above 2^64 - 1)."""
    return next((e for e in EDGE if e > c), None)


def down(c):
    """The next edge counter below c (0: none)."""
    return next((e for e in reversed(EDGE) if e < c), 0)


def hot(A):
    """The actor ids at the ends of the lane / mask mappings."""
    return sorted({0, A // 2, min(A - 1, 31), min(A - 1, 32), min(A - 1, 63), min(A - 1, 64), A - 1})


def signed(x):
    return x - 2**64 if x >= 2**63 else x


# ------------------------------------------------------------------ states
# A state is (clock {a: c}, entries {m: {a: c}}, deferred {((a, c), ...): {m, ...}}),
# the arguments of records.encode.
EMPTY = ({}, {}, {})
EMPTY_MEMBER_CLOCK = 2  # header flag CRDT_ORSWOT_EMPTY_MEMBER_CLOCK (include/crdts_hip.h)


def encode(state, A, sparse=False):
    """The state's record; a member with an empty clock (truncate's output
    only) sets the header flag, as the oracle's encoder does."""
    clock, entries, deferred = state
    rec = records.encode(clock, entries, deferred, A, sparse)
    if any(not d for d in entries.values()):
        rec = rec[:28] + struct.pack("<I", struct.unpack_from("<I", rec, 28)[0] | EMPTY_MEMBER_CLOCK) + rec[32:]
    return rec


def state_of(rec):
    d = records.decode(rec)
    return (d["clock"], {m: dict(c) for m, c in d["entries"].items()},
            {tuple(c): set(ms) for c, ms in d["deferred"]})


def shape_of(rec):
    """A record as an ordered structure: what a wrong join's output is compared by."""
    d = records.decode(rec)
    return (d["clock"], [(m, sorted(c)) for m, c in d["entries"].items()],
            [(tuple(c), list(ms)) for c, ms in d["deferred"]])


def _keys(rng, n):
    """n distinct member keys: edge keys, pairs that differ only in the high
    or only in the low word, and random draws."""
    ks = set()
    while len(ks) < n:
        u = rng.random()
        if u < 0.35:
            ks.add(rng.choice(KEYS + (0, M64)))  # (the ends of the key range twice as often)
            continue
        r = rng.getrandbits(64)
        ks.add(r)
        if u < 0.55:
            ks.add(r ^ (1 << rng.randrange(32, 64)))
        elif u < 0.7:
            ks.add(r ^ (1 << rng.randrange(32)))
    ks = sorted(ks)
    rng.shuffle(ks)
    return ks[:n]


def _clock_pair(rng):
    lo, hi = rng.choice(PAIRS)
    u = rng.random()
    if u < 0.4:
        return lo, hi
    if u < 0.8:
        return hi, lo
    v = rng.choice((lo, hi)) or hi
    return v, v


def _dot(rng, own, oth):
    """A dot counter <= own (the side's top counter for the actor), aimed at
    the other side's top counter oth: equal to it, one edge step below or
    above it, the side's own top counter, or any edge counter."""
    aim = [c for c in (oth, down(oth), up(oth) or 0, own, own) if 0 < c <= own]
    if rng.random() < 0.2:
        aim = [e for e in EDGE if e <= own] or aim
    return rng.choice(aim)


def _some(rng, xs, k):
    xs = sorted(xs)
    return rng.sample(xs, min(len(xs), rng.randint(1, k))) if xs else []


def _actors(rng, A, n_act):
    H = hot(A)
    acts = set(rng.sample(H, min(len(H), n_act, rng.randint(1, len(H)))))
    while len(acts) < min(A, n_act):
        acts.add(rng.randrange(A))
    return acts


def _deferred(rng, own, M, ents, keys):
    """One deferred clock of the side whose top clock is `own`, against the
    merged clock M -> (clock pairs, member set), or None. It is pending on
    its own side (some counter above own's) as in a reachable state."""
    acts = sorted(M)
    u = rng.random()
    present = sorted(set(ents[0]) | set(ents[1]))
    names = set(_some(rng, present, 3)) if present and rng.random() < 0.85 else set()
    if not names or rng.random() < 0.2:
        names.add(rng.choice(keys) if keys and rng.random() < 0.7 else rng.getrandbits(64))
    if u < 0.25 and any(own.get(a, 0) < M[a] for a in acts):
        d = dict(M)  # equal to the merged clock
    else:
        d = {}
        for a in _some(rng, acts, 4):
            c = rng.choice([M[a], M[a], down(M[a])] + [e for e in EDGE if e <= M[a]])
            if c:
                d[a] = c
        if u >= 0.6:  # one edge step above the merged clock
            a = rng.choice(acts)
            if up(M[a]):
                d[a] = up(M[a])
        if rng.random() < 0.7:  # cover a named member's dot exactly, or stop one step short of it
            m = rng.choice(sorted(names))
            dots = ents[0].get(m) or ents[1].get(m)
            if dots:
                a, v = rng.choice(sorted(dots.items()))
                c = v if rng.random() < 0.5 else down(v)
                if c:
                    d[a] = c
    if all(own.get(a, 0) >= c for a, c in d.items()):
        behind = [a for a in acts if own.get(a, 0) < M[a]]
        ahead = [a for a in acts if up(M[a])]
        if behind and u < 0.6:
            a = rng.choice(behind)
            d[a] = M[a]  # still <= the merged clock
        elif ahead:
            a = rng.choice(ahead)
            d[a] = up(M[a])
        else:
            return None
    return tuple(sorted(d.items())), names


def pair(rng, A, n_act=None, n_keys=None, n_def=(0, 0), dots=3, sides=(0.5, 0.25), acts=None):
    """One object pair -> (L, R). n_act present actors between the sides,
    n_keys member keys between them (`sides`: the shares on both sides and on
    self only), n_def = (lo, hi) deferred clocks a side, up to `dots` dots a
    member; `acts`: the present actors themselves."""
    n_act = min(A, rng.randint(1, 12) if n_act is None else n_act)
    n_keys = rng.randint(0, 10) if n_keys is None else n_keys
    acts = acts or _actors(rng, A, n_act)
    Lc, Rc = {}, {}
    for a in sorted(acts):
        l, r = _clock_pair(rng)
        if l:
            Lc[a] = l
        if r:
            Rc[a] = r
    keys = _keys(rng, n_keys)
    Le, Re = {}, {}
    for m in keys:
        u = rng.random()
        where = "LR" if u < sides[0] else "L" if u < sides[0] + sides[1] else "R"
        common = {}
        if where == "LR":  # equal dots on both sides
            for a in _some(rng, set(Lc) & set(Rc), dots):
                if rng.random() < 0.5:
                    common[a] = _dot(rng, min(Lc[a], Rc[a]), min(Lc[a], Rc[a]))
        for s in where:
            own, oth, ent = (Lc, Rc, Le) if s == "L" else (Rc, Lc, Re)
            d = dict(common)
            for a in _some(rng, own, dots):
                d.setdefault(a, _dot(rng, own[a], oth.get(a, 0)))
            if d:
                ent[m] = d
    M = {a: max(Lc.get(a, 0), Rc.get(a, 0)) for a in acts}
    Ld, Rd = {}, {}
    for own, out in ((Lc, Ld), (Rc, Rd)):
        for _ in range(rng.randint(*n_def)):
            D = _deferred(rng, own, M, (Le, Re), keys)
            if D:
                out.setdefault(D[0], set()).update(D[1])
    for k, v in list(Ld.items()):  # the same deferred clock on both sides: the member sets are united
        if rng.random() < 0.2 and any(Rc.get(a, 0) < c for a, c in k):
            Rd.setdefault(k, set()).update(_some(rng, v, 2) + [rng.getrandbits(64)])
    return (Lc, Le, Ld), (Rc, Re, Rd)


def forced(rng, A):
    """The objects at the head of every batch: both sides empty; self empty;
    other empty; self == other; a side whose only member is key 2^64 - 1; a
    side whose only member is key 0 next to a side without members whose last
    top-clock word is 0 (the word in front of its empty key section)."""
    g = lambda: pair(rng, A, n_keys=6, n_def=(0, 2))  # noqa: E731
    a0 = min(A - 1, 1)
    ones = ({0: 2**63}, {M64: {0: 2**63}}, {})
    zero = ({0: 2**32}, {0: {0: 2**32}}, {})
    bare = ({a: c for a, c in {0: 2**32 - 1, a0: 1}.items() if a < A - 1}, {}, {})  # (A = 1: the empty clock)
    x = g()[0]
    return [(EMPTY, EMPTY), (EMPTY, g()[1]), (g()[0], EMPTY), (x, x), (ones, g()[1]), (g()[0], ones), (zero, bare),
            (bare, zero)]


N_FORCED = 8


def grow(state, A, size, sparse=False):
    """The state padded to a record of exactly `size` bytes by members added
    to its last deferred clock's set (8 bytes each)."""
    clock, entries, deferred = state
    deferred = {k: set(v) for k, v in deferred.items()}
    n = lambda: len(records.encode(clock, entries, deferred, A, sparse))  # noqa: E731
    last, k = max(deferred), 2**40
    deferred[last].update(range(k, k + max(0, size - n() - 8) // 8))
    k += size
    while n() < size:
        deferred[last].add(k)
        k += 1
    assert n() == size, (n(), size)
    return clock, entries, deferred


# ------------------------------------------------------------------ the reference, restated
def _le(k, d, clock, gt=operator.gt):
    """d <= clock (src/vclock.rs:59-71) under the counter key k: no counter of d above clock's."""
    return not any(gt(k(c), k(clock.get(a, 0))) for a, c in (d.items() if isinstance(d, dict) else d))


def _apply_deferred(k, clock, entries, deferred, pending, kill):
    """apply_deferred (src/orswot.rs:235-243) over entries as a list of
    [key, dots]: every deferred clock removes the dots it covers from the
    members it names (apply_remove :195-211: `c >= dot`, VClock::subtract) and
    stays deferred unless it is <= clock."""
    kept = {}
    for dk, ms in deferred.items():
        if not _le(k, dk, clock, pending):
            kept[dk] = set(ms)
        for e in entries:
            if e[0] in ms:
                e[1] = {a: v for a, v in e[1].items() if not any(b == a and kill(k(c), k(v)) for b, c in dk)}
    return [e for e in entries if e[1]], kept


def merge_ref(L, R, ckey=None, dot_gt=operator.gt, pending=operator.gt, kill=operator.ge, klt=operator.lt,
              keq=operator.eq, absent_key=None, cmax=None):
    """Orswot::merge (src/orswot.rs:87-157) on states -> (clock, [[key, dots]
    ...] in the order a two-pointer walk of the sorted key lists emits them,
    deferred). With the defaults it restates the reference; every knob makes
    it wrong in one way (MUTANTS): ckey the key counters are compared by,
    dot_gt a dot against the other side's top counter, pending a deferred
    counter against the merged clock's, kill a deferred counter against a
    dot's, klt / keq the key order and equality of the walk, absent_key a key
    the walk takes for "side exhausted", cmax the top clock's maximum."""
    k = ckey or (lambda c: c)
    (Lc, Le, Ld), (Rc, Re, Rd) = L, R
    lk = [m for m in sorted(Le) if m != absent_key]
    rk = [m for m in sorted(Re) if m != absent_key]
    out, i, j = [], 0, 0

    def beyond(dots, clock):  # the dots `clock` has not seen (VClock::subtract: removed when clock's >= it)
        return {a: c for a, c in dots.items() if dot_gt(k(c), k(clock.get(a, 0)))}

    while i < len(lk) or j < len(rk):
        if i < len(lk) and j < len(rk) and keq(lk[i], rk[j]):
            x, y = Le[lk[i]], Re[rk[j]]
            d = {a: c for a, c in x.items() if a in y and k(y[a]) == k(c)}  # intersection :109
            rest = [beyond({a: c for a, c in x.items() if a not in d}, Rc),
                    beyond({a: c for a, c in y.items() if a not in d}, Lc)]
            for r in rest:
                for a, c in r.items():
                    if not k(d.get(a, 0)) >= k(c):  # witness
                        d[a] = c
            if d:
                out.append([lk[i], d])
            i, j = i + 1, j + 1
        elif j >= len(rk) or (i < len(lk) and klt(lk[i], rk[j])):
            if beyond(Le[lk[i]], Rc):  # self only: kept whole unless the other side has seen all of it :98-103
                out.append([lk[i], dict(Le[lk[i]])])
            i += 1
        else:
            d = beyond(Re[rk[j]], Lc)  # other only: what self has not seen :132-137
            if d:
                out.append([rk[j], d])
            j += 1
    deferred = {dk: set(v) for dk, v in Ld.items()}
    for dk, v in Rd.items():
        deferred.setdefault(dk, set()).update(v)
    mx = cmax or (lambda x, y: y if k(y) > k(x) else x)
    clock = {}
    for a in sorted(set(Lc) | set(Rc)):
        c = mx(Lc.get(a, 0), Rc.get(a, 0))
        if c:
            clock[a] = c
    out, deferred = _apply_deferred(k, clock, out, deferred, pending, kill)
    return clock, out, deferred


def as_state(res):
    clock, out, deferred = res
    return clock, {m: d for m, d in out}, deferred


def as_shape(res):
    clock, out, deferred = res
    return (clock, [(m, sorted(d.items())) for m, d in out],
            [(dk, sorted(deferred[dk])) for dk in sorted(deferred)])


def _subtract(k, dots, clock, ge):
    return {a: c for a, c in dots.items() if not (a in clock and ge(k(clock[a]), k(c)))}


def truncate_ref(S, T, sub_ge=operator.ge, **knobs):
    """Causal::truncate (src/orswot.rs:159-172): merge with an empty set whose
    clock is T, then subtract T from the top clock and from every member
    clock (a member may be left with an EMPTY clock). sub_ge: the subtract's
    compare (VClock::subtract removes a counter when T's is >= it)."""
    k = knobs.get("ckey") or (lambda c: c)
    clock, out, deferred = merge_ref(S, (dict(T), {}, {}), **knobs)
    return (_subtract(k, clock, T, sub_ge), [[m, _subtract(k, d, T, sub_ge)] for m, d in out], deferred)


def apply_ref(S, ops, ckey=None, stale_ge=operator.ge, pending=operator.gt, kill=operator.ge):
    """CmRDT::apply of the ops in order (src/orswot.rs:61-85, apply_remove
    :195-211, apply_deferred :235-243) -> (clock, [[key, dots] ...] by key,
    deferred). stale_ge: the Add's `clock.get(actor) >= counter` test."""
    k = ckey or (lambda c: c)
    clock = dict(S[0])
    entries = [[m, dict(d)] for m, d in sorted(S[1].items())]
    deferred = {dk: set(v) for dk, v in S[2].items()}
    for op in ops:
        if op[0] == "add":
            _, a, c, m = op
            if stale_ge(k(clock.get(a, 0)), k(c)):
                continue
            e = next((e for e in entries if e[0] == m), None)
            if e is None:
                e = [m, {}]
                entries.append(e)
            if not k(e[1].get(a, 0)) >= k(c):
                e[1][a] = c
            if not k(clock.get(a, 0)) >= k(c):
                clock[a] = c
            entries, deferred = _apply_deferred(k, clock, entries, deferred, pending, kill)
        else:
            _, m, ctx = op
            entries, kept = _apply_deferred(k, clock, entries, {tuple(ctx): {m}}, pending, kill)
            for dk, v in kept.items():
                deferred.setdefault(dk, set()).update(v)
    return clock, sorted(entries), deferred


def _per_half(x, y):
    return (max(x >> 32, y >> 32) << 32) | max(x & M32, y & M32)


MUTANTS = {
    "counter_compare_low32": dict(ckey=lambda c: c & M32),
    "counter_compare_high32": dict(ckey=lambda c: c >> 32),
    "counter_compare_signed": dict(ckey=signed),
    "dot_survives_on_equal": dict(dot_gt=operator.ge),  # `>=` for `>` on a dot against the top clock
    "deferred_kept_on_equal": dict(pending=operator.ge),  # `<` for `<=` on the deferred-clock drop
    "deferred_kill_strict": dict(kill=operator.gt),  # `>` for `>=` in the deferred kill
    "key_order_signed": dict(klt=lambda x, y: signed(x) < signed(y)),
    "key_all_ones_is_absent": dict(absent_key=M64),
    "key_equal_on_low_word": dict(keq=lambda x, y: x & M32 == y & M32),
    "max_per_half": dict(cmax=_per_half),
}
TRUNCATE_MUTANTS = {
    "counter_compare_low32": dict(ckey=lambda c: c & M32),
    "counter_compare_signed": dict(ckey=signed),
    "subtract_strict": dict(sub_ge=operator.gt),  # a counter equal to T's stays
    "dot_survives_on_equal": dict(dot_gt=operator.ge),
    "deferred_kept_on_equal": dict(pending=operator.ge),
    "deferred_kill_strict": dict(kill=operator.gt),
}
APPLY_MUTANTS = {
    "counter_compare_low32": dict(ckey=lambda c: c & M32),
    "counter_compare_signed": dict(ckey=signed),
    "stale_add_strict": dict(stale_ge=operator.gt),  # an Add at exactly the top counter is taken as new
    "deferred_kept_on_equal": dict(pending=operator.ge),
    "deferred_kill_strict": dict(kill=operator.gt),
}


# ------------------------------------------------------------------ launch tiers
FAST_STAGE = 2048        # orswot_join5_kernel: LDS stage per record (kFastStage)
GEN_STAGE = 8192         # the general kernels' stage per record (kGenStage)
BIG_MIN_POS = 128        # union positions past which the general kernels hand an object on (kBigMinPos)
BIG_STAGE = 32768        # orswot_big_kernel: LDS stage per record (kBigStage)
BIG_STAGED_POS = 64 * 96      # ... positions its staged path holds (kWave * kBigChS)
BIG_HBM_POS = 64 * 4096       # ... and its HBM path's tables (kWave * kBigChH); past them one wave
DN_PAIR = 6144           # orswot_sparse_mask_kernel<DN>: pair stage (kSpPair)
CSR_PAIR = 7168          # ... for CSR batches (kSpPairCsr)
WIDE_PAIR = 16384        # orswot_dense_wide_kernel: pair stage (kWdPair)
MAX_DEFERRED = 32        # deferred clocks a side in every mask join
TABLE_ACTORS = 1024      # kSpTableN: the widest dense batch of the dense-wide launcher, the CSR universe

TIERS_DENSE = ("fast", "fast_hd", "general", "big_lds", "big_hbm", "big_wave")
TIERS_WIDE = ("dn64", "dn128", "wide", "general", "big_lds", "big_hbm", "big_wave")
TIERS_CSR = ("sp", "sp_general", "big_lds", "big_hbm", "big_wave")


def tier(A, L, R, sparse=False):
    """The kernel that joins the records L and R of one object, by the rule of
    launch_orswot_merge / launch_orswot_merge_sparse and the kernels' limits:
    dense, A <= 64 (orswot_join5_kernel<6, 32> / <5, 64>): "fast" / "fast_hd"
      (with deferred clocks): records <= 2 KB, <= 64 members and dots a side,
      <= 32 deferred clocks a side, a union of <= 64 members;
    dense, 65 <= A <= 1024: "dn64" / "dn128": the DN mask join (pair <= 6 KB,
      <= 64 members and <= 128 dots a side, union of <= 64 members) with a
      union of <= 64 / <= 128 present actors; "wide": orswot_dense_wide_kernel
      (pair <= 16 KB, same limits, <= 128 present actors);
    dense, A > 1024: join5<5, 64> takes no object (A > its 64 mask bits);
    CSR: "sp": the sparse mask join (pair <= 7 KB, <= 64 clock entries and
      members and <= 128 dots a side, unions of <= 64 actors and members);
    everything else the general kernel of its form ("general" /
    "sp_general"), which hands objects past 128 union positions or its 8 KB
    stage to orswot_big_kernel: "big_lds" (records <= 32 KB staged), "big_hbm"
    (<= 262 144 positions), "big_wave" (one wave)."""
    (szl, cl, ml, dl, fl), (szr, cr, mr, dr, fr) = struct.unpack_from("<5I", L), struct.unpack_from("<5I", R)
    U = Uc = 0
    if ml <= 64 and mr <= 64:  # (else the headers decide: a big record is not decoded)
        x, y = records.decode(L), records.decode(R)
        U = len(set(x["entries"]) | set(y["entries"]))
        Uc = len(set(x["clock"]) | set(y["clock"]))

    def past():
        if not (ml + mr > BIG_MIN_POS or szl > GEN_STAGE or szr > GEN_STAGE):
            return "sp_general" if sparse else "general"
        if ml + mr > BIG_HBM_POS:
            return "big_wave"
        return "big_lds" if szl <= BIG_STAGE and szr <= BIG_STAGE and ml + mr <= BIG_STAGED_POS else "big_hbm"

    side = ml <= 64 and mr <= 64 and fl <= MAX_DEFERRED and fr <= MAX_DEFERRED and U <= 64
    if sparse:
        ok = side and szl + szr <= CSR_PAIR and A <= TABLE_ACTORS and cl <= 64 and cr <= 64 and dl <= 128 and dr <= 128
        return "sp" if ok and Uc <= 64 else past()
    if 64 < A <= TABLE_ACTORS:
        ok = side and dl <= 128 and dr <= 128
        if ok and szl + szr <= DN_PAIR and Uc <= 128:
            return "dn64" if Uc <= 64 else "dn128"
        return "wide" if ok and szl + szr <= WIDE_PAIR and Uc <= 128 else past()
    ok = side and A <= 64 and szl <= FAST_STAGE and szr <= FAST_STAGE and dl <= 64 and dr <= 64
    if ok:
        return "fast_hd" if fl | fr else "fast"
    return past()


def tiers(A, Ls, Rs, sparse=False):
    out = {}
    for l, r in zip(Ls, Rs):
        t = tier(A, l, r, sparse)
        out[t] = out.get(t, 0) + 1
    return out


# ------------------------------------------------------------------ object pairs at the limits
def _until(make, ok, tries=500):
    for _ in range(tries):
        p = make()
        if ok(p):
            return p
    raise AssertionError("no object of the wanted shape in %d draws" % tries)


def _n(state, A, sparse=False):
    return len(records.encode(*state, A, sparse))


def _union(p):
    return len(set(p[0][1]) | set(p[1][1]))


def _fits_masks(p, dots=64):
    return all(len(s[1]) <= 64 and sum(len(d) for d in s[1].values()) <= dots and len(s[2]) <= MAX_DEFERRED
               for s in p) and _union(p) <= 64


def member_union(rng, A, U, sparse=False, n_act=None):
    """A pair whose sides hold <= 64 members and dots each and exactly U between them."""
    return _until(lambda: pair(rng, A, n_act=n_act or rng.randint(2, 8), n_keys=U, n_def=(0, rng.randint(0, 1)),
                               dots=1, sides=(0.2, 0.4)),
                  lambda p: _union(p) == U and _fits_masks((p[0], p[0])) and _fits_masks((p[1], p[1])))


def sized(rng, A, size=None, pair_size=None, sparse=False, n_act=None, n_keys=30):
    """A pair within the mask joins' counts whose self record is grown, by
    members of its last deferred clock's set, to `size` bytes, or until both
    records together hold `pair_size` bytes."""
    p = _until(lambda: pair(rng, A, n_act=n_act, n_keys=n_keys, n_def=(1, 3), dots=2),
               lambda p: p[0][2] and _fits_masks(p, 128 if A > 64 or sparse else 64)
               and _n(p[0], A, sparse) <= (size or pair_size - _n(p[1], A, sparse))
               and (size is None or _n(p[1], A, sparse) <= size))
    return grow(p[0], A, size or pair_size - _n(p[1], A, sparse), sparse), p[1]


def many_deferred(rng, A, nd):
    """A pair whose self side holds nd deferred clocks; the last of them in
    CLOCK ORDER (the top bit of the join's deferred mask at nd = 32) is the
    one that kills a present member's dot."""
    def make():
        L, R = pair(rng, A, n_act=rng.randint(3, 8), n_keys=8)
        M = {a: max(L[0].get(a, 0), R[0].get(a, 0)) for a in set(L[0]) | set(R[0])}
        acts = sorted(M)
        a0 = acts[0]
        hits = [(m, a, v) for e in (L[1], R[1]) for m, d in e.items() for a, v in d.items() if a > a0]
        if len(acts) < 3 or M[a0] > 2**64 - 2 - nd or not hits:
            return None
        keys = sorted(set(L[1]) | set(R[1]))
        deferred = {((a0, M[a0] + 1 + t),): {rng.choice(keys) if t % 2 else rng.getrandbits(64)} for t in range(nd - 1)}
        m, a1, v = rng.choice(hits)
        a2 = rng.choice([a for a in acts[1:] if a != a1 and up(M[a])] or [None])
        if a2 is None:
            return None
        deferred[tuple(sorted({a1: v, a2: up(M[a2])}.items()))] = {m}
        return (L[0], L[1], deferred), R
    return _until(make, lambda p: p is not None)


def heavy(rng, A, n, sparse=False, n_def=(4, 12)):
    """A pair of about 0.75 n members a side (1.5 n union positions), edge counters and keys 0 and 2^64 - 1."""
    L, R = pair(rng, A, n_act=min(A, 16), n_keys=n, n_def=n_def, dots=2)
    for s, m in ((L, 0), (R, M64)):
        if s[0]:
            a, c = max(s[0].items())
            s[1].setdefault(m, {a: c})
    return L, R


def heavy_wave(seed, A, n, n_def=4):
    """A pair of about 0.75 n one-dot members a side for orswot_big_kernel's
    one-wave path (> 262 144 union positions), built straight from numpy
    draws as tests/test_gpu_orswot.py::_synth_heavy_pair is: half the keys on
    both sides (half of those with the same dot on both), a quarter on either
    side alone, keys 0 and 2^64 - 2 on self only and 1 and 2^64 - 1 on other
    only; per actor the top counters are an edge pair and every dot is aimed at
    the other side's top counter (_dot's choices)."""
    rng, g = random.Random(seed), np.random.default_rng(seed)
    while True:
        Lc, Rc = {}, {}
        for a in range(A):
            l, r = _clock_pair(rng)
            Lc.update({a: l} if l else {})
            Rc.update({a: r} if r else {})
        both = sorted(set(Lc) & set(Rc))
        if len(both) >= 2 and len(Lc) >= 2 and len(Rc) >= 2:
            break
    special = np.array([0, M64 - 1, 1, M64], np.uint64)
    pool = np.setdiff1d(np.unique(g.integers(0, 2**64, size=n + n // 8, dtype=np.uint64, endpoint=False)), special)
    g.shuffle(pool)
    shared, only = pool[:n // 2], (np.concatenate([pool[n // 2:3 * n // 4], special[:2]]),
                                   np.concatenate([pool[3 * n // 4:n], special[2:]]))

    def dots(keys, acts, own, oth):
        """One dot a key: a random actor of `acts`, a counter from _dot's aims at oth's top counter."""
        act = g.choice(np.array(acts, np.uint32), size=len(keys))
        ctr = np.zeros(len(keys), np.uint64)
        for a in acts:
            aim = [c for c in (oth.get(a, 0), down(oth.get(a, 0)), up(oth.get(a, 0)) or 0, own[a], own[a])
                   if 0 < c <= own[a]]
            at = act == a
            ctr[at] = g.choice(np.array(aim, np.uint64), size=int(at.sum()))
        return act, ctr

    low = {a: min(Lc[a], Rc[a]) for a in both}
    ca, cc = dots(shared[:len(shared) // 2], both, low, low)  # the same dot on both sides
    sides = []
    for own, oth, mine in ((Lc, Rc, only[0]), (Rc, Lc, only[1])):
        keys = np.concatenate([shared[len(shared) // 2:], mine])
        a, c = dots(keys, sorted(own), own, oth)
        keys, a, c = np.concatenate([shared[:len(shared) // 2], keys]), np.concatenate([ca, a]), np.concatenate([cc, c])
        sides.append([own, {m: {x: y} for m, x, y in zip(keys.tolist(), a.tolist(), c.tolist())}, {}])
    M = {a: max(Lc.get(a, 0), Rc.get(a, 0)) for a in range(A) if a in Lc or a in Rc}
    some = [{int(m): s[1][int(m)] for m in shared[:40]} for s in sides]  # the members the deferred clocks may name
    for s in sides:
        for _ in range(n_def):
            D = _deferred(rng, s[0], M, some, sorted(some[0]))
            if D:
                s[2].setdefault(D[0], set()).update(D[1])
    return tuple(sides[0]), tuple(sides[1])


# ------------------------------------------------------------------ merge batches
# label -> the tiers an object of that label must take (tier())
LABEL_TIERS = {
    "forced": None, "plain": ("fast",), "deferred": ("fast_hd", "fast"),
    "union64": ("fast", "fast_hd"), "union65": ("general",),
    "size2048": ("fast_hd",), "size2064": ("general",),
    "ndef31": ("fast_hd",), "ndef32": ("fast_hd",), "ndef33": ("general",),
    "over_stage": ("big_lds",),
    "big150": ("big_lds",), "big700": ("big_lds",), "big1000": ("big_lds",), "big3000": ("big_hbm",),
    "big20000": ("big_hbm",), "big180000": ("big_wave",),
    "u64": ("dn64", "wide"), "u65": ("dn128", "wide"), "u128": ("dn128", "wide"), "u129": ("general",),
    "pair6144": ("dn64", "dn128"), "pair6160": ("wide",), "pair16384": ("wide",), "pair16400": ("big_lds",),
    "sp": ("sp",), "sp_deferred": ("sp",), "sp_u64": ("sp",), "sp_u65": ("sp_general",), "sp_m64": ("sp",),
    "sp_m65": ("sp_general",), "sp_pair7168": ("sp",), "sp_pair7184": ("sp_general",), "sp_big150": ("big_lds",),
}


def _recipe(A, kind):
    P, D = ("plain", 0.6, lambda r: pair(r, A)), ("deferred", 0.4, lambda r: pair(r, A, n_def=(1, 3)))
    if kind == "basic":  # join5<6, 32> / <5, 64>: plain and deferred-remove objects
        return [P, D]
    if kind == "over":  # every record past every stage of its launcher
        return [("over_stage", 0.6, P[2]), ("over_stage", 0.4, D[2])]
    if kind == "limits":
        f = [("union64", lambda r: member_union(r, A, 64)), ("union65", lambda r: member_union(r, A, 65)),
             ("size2048", lambda r: sized(r, A, 2048)), ("size2064", lambda r: sized(r, A, 2064)),
             ("ndef31", lambda r: many_deferred(r, A, 31)), ("ndef32", lambda r: many_deferred(r, A, 32)),
             ("ndef33", lambda r: many_deferred(r, A, 33))]
        return [("plain", 0.3, P[2]), ("deferred", 0.2, D[2])] + [(n, 0.5 / len(f), g) for n, g in f]
    if kind == "big":
        return [P, D]
    if kind == "wide":
        us = [u for u in (64, 65, 128, 129) if u <= A]
        f = [("u%d" % u, lambda r, u=u: pair(r, A, n_act=u, n_def=(0, r.randint(0, 2)))) for u in us]
        f += [("pair%d" % s, lambda r, s=s: sized(r, A, pair_size=s, n_act=r.choice([u for u in us if u <= 128])))
              for s in (6144, 6160, 16384, 16400)]
        return [(n, 1.0 / len(f), g) for n, g in f]
    if kind == "csr":
        f = [("sp", P[2]), ("sp_deferred", D[2]), ("sp_u64", lambda r: pair(r, A, n_act=64, n_def=(0, 1))),
             ("sp_u65", lambda r: pair(r, A, n_act=65, n_def=(0, 1))),
             ("sp_m64", lambda r: member_union(r, A, 64, True)), ("sp_m65", lambda r: member_union(r, A, 65, True)),
             ("sp_pair7168", lambda r: sized(r, A, pair_size=7168, sparse=True)),
             ("sp_pair7184", lambda r: sized(r, A, pair_size=7184, sparse=True))]
        return [(n, 1.0 / len(f), g) for n, g in f]
    raise ValueError(kind)


# name -> (A, sparse, objects after the forced ones, recipe, big pairs' member counts)
MERGE_SHAPES = {
    "A1": (1, False, 632, "basic", ()), "A16": (16, False, 632, "basic", ()), "A32": (32, False, 632, "basic", ()),
    "A16_limits": (16, False, 560, "limits", ()),
    "A33": (33, False, 632, "basic", ()), "A64": (64, False, 632, "basic", ()),
    "A65": (65, False, 320, "wide", ()), "A128": (128, False, 400, "wide", ()), "A160": (160, False, 480, "wide", ()),
    "A1024": (1024, False, 200, "over", ()), "A1025": (1025, False, 200, "over", ()),
    # (the member counts of test_big_kernel_paths; 1000 for its 1200 keeps a pair of two-dot members inside the
    # big kernel's 32 KB stage, and 180000 for its 150000 gives 0.75 n members a side: 270 000 union positions)
    "A16_big": (16, False, 240, "big", (150, 700, 1000, 3000, 20000, 180000)),
    "csr": (1024, True, 640, "csr", (150,)),
}


# the tiers every shape must hold, both sides of each boundary -> the fewest objects of each
SHAPE_TIERS = {
    **{n: {"fast": 300, "fast_hd": 200} for n in ("A1", "A16", "A32", "A33", "A64")},
    "A16_limits": {"fast": 150, "fast_hd": 150, "general": 100},
    "A65": {"dn64": 50, "dn128": 50, "wide": 50, "big_lds": 30},
    "A128": {"dn64": 50, "dn128": 50, "wide": 50, "big_lds": 30},
    "A160": {"dn64": 50, "dn128": 50, "wide": 50, "general": 50, "big_lds": 30},
    "A1024": {"big_lds": 200}, "A1025": {"big_lds": 200},
    "A16_big": {"fast": 100, "fast_hd": 50, "big_lds": 3, "big_hbm": 2, "big_wave": 1},
    "csr": {"sp": 300, "sp_general": 200, "big_lds": 1},
}


WAVE_MEMBERS = 100_000  # member counts past which a big pair is built by heavy_wave (numpy), not pair()


def merge_batch(name):
    """-> (A, sparse, [(L, R) states], labels): the forced objects, then the
    shape's recipe in shuffled order with its big pairs spread among them."""
    A, sparse, n, kind, bigs = MERGE_SHAPES[name]
    rng = random.Random("orswot-edges-" + name)
    objs = [("forced", p) for p in forced(rng, A)]
    rest = []
    for label, share, make in _recipe(A, kind):
        rest += [(label, make(rng)) for _ in range(max(1, round(share * n)))]
    rng.shuffle(rest)
    for k, m in enumerate(bigs):
        big = heavy_wave(m, A, m) if m > WAVE_MEMBERS else heavy(rng, A, m, sparse, (4 + 8 * (k % 2),) * 2)
        rest.insert(5 * k + 1, (("sp_big%d" if sparse else "big%d") % m, big))
    objs += rest
    return A, sparse, [p for _, p in objs], [l for l, _ in objs]


def check_tiers(A, sparse, Ls, Rs, labels):
    """Every labelled object takes a tier its label allows -> counts per (label, tier)."""
    counts = {}
    for l, r, lab in zip(Ls, Rs, labels):
        for x, y in ((l, r), (r, l)):
            t = tier(A, x, y, sparse)
            assert LABEL_TIERS[lab] is None or t in LABEL_TIERS[lab], (lab, t, struct.unpack_from("<8I", x),
                                                                      struct.unpack_from("<8I", y))
            counts[lab, t] = counts.get((lab, t), 0) + (x is l)  # counted in the first orientation
    return counts


# ------------------------------------------------------------------ truncate and apply inputs
def truncating_clock(rng, state, A):
    """A truncating clock on the edges of the state it meets: per actor the
    state's top counter, a dot's or a deferred clock's counter for it, one
    edge step below or above, or any edge counter."""
    clock, entries, deferred = state
    seen = {}
    for d in entries.values():
        for a, c in d.items():
            seen.setdefault(a, []).append(c)
    for dk in deferred:
        for a, c in dk:
            seen.setdefault(a, []).append(c)
    T = {}
    for a in sorted(set(clock) | set(seen) | {rng.choice(hot(A))}):
        if rng.random() < 0.25:
            continue
        base = rng.choice(seen.get(a, []) + [clock.get(a, 0)] * 2) or rng.choice(EDGE)
        T[a] = rng.choice([base, base, down(base) or base, up(base) or base, rng.choice(EDGE)])
    # a member left with an EMPTY clock: one of its dots lies above T and is
    # killed by a deferred clock, the others are cut by T at exactly their counters
    hits = [(m, a) for dk, ms in sorted(deferred.items()) for m in sorted(ms) if m in entries
            for a, c in dk if c >= entries[m].get(a, M64 + 1)]
    if hits and rng.random() < 0.3:
        m, a = rng.choice(hits)
        T.update(entries[m])
        T[a] = down(entries[m][a])
        if not T[a]:
            del T[a]
    return T


def truncate_form(A, rec, sparse=False):
    """The form crdt_orswot_truncate takes for a record (csrc/truncate.hip):
    "fast" the streaming form (dense, A <= 32, <= 2 KB, <= 64 members, dots,
    deferred dots and deferred members, <= 8 deferred clocks); "lds1" / "lds2"
    the single-pass (no deferred clock, <= 64 members of <= 4 dots) and the
    two-pass LDS form (dense, A <= 32, <= 4 KB, <= 8 deferred clocks, <= 170
    members); "hbm" the rest."""
    size, _, n_mem, n_dot, n_def, n_def_dot, n_def_mem, _ = struct.unpack_from("<8I", rec)
    if sparse or A > 32 or size > 4096 or n_def > 8 or n_mem > 4096 // 24:
        return "hbm"
    if size <= 2048 and max(n_mem, n_dot, n_def_dot, n_def_mem) <= 64:
        return "fast"
    most = max((len(d) for d in records.decode(rec)["entries"].values()), default=0)
    return "lds1" if n_def == 0 and n_mem <= 64 and most <= 4 else "lds2"


def ops_for(rng, state, A, n_ops):
    """An op list on the edges of the state it meets: Adds at exactly the top
    counter (stale), one edge step above it (fresh) and at 2^64 - 1, of
    present members and of the keys next to them (0, 2^64 - 1 included);
    removes whose context is the member's clock, or one step past it in one
    counter; a future-context remove left deferred, then the Add at exactly
    that counter that releases it."""
    clock = dict(state[0])
    entries = {m: dict(d) for m, d in state[1].items()}
    H = hot(A)
    ops = []

    def actor():
        return rng.choice(sorted(clock)) if clock and rng.random() < 0.7 else rng.choice(H)

    def member():
        if entries and rng.random() < 0.7:
            m = rng.choice(sorted(entries))
            u = rng.random()
            return m if u < 0.6 else (m + 1) & M64 if u < 0.8 else (m - 1) & M64
        return rng.choice(KEYS) if rng.random() < 0.6 else rng.getrandbits(64)

    def add(a, c, m):
        ops.append(("add", a, c, m))
        if c > clock.get(a, 0):
            clock[a] = c
            entries.setdefault(m, {})[a] = c

    while len(ops) < n_ops:
        u = rng.random()
        a = actor()
        top = clock.get(a, 0)
        if u < 0.15 and top:
            add(a, top, member())  # stale: exactly the top counter
        elif u < 0.4:
            c = up(top)
            if c:
                add(a, c, member())
        elif u < 0.45:
            add(a, M64, member())
        elif u < 0.65 and entries:
            m = rng.choice(sorted(entries))
            ctx = dict(entries[m])
            if rng.random() < 0.5 and ctx:  # one step past the member's clock in one counter
                b = rng.choice(sorted(ctx))
                ctx[b] = up(ctx[b]) or ctx[b]
            if ctx:
                ops.append(("rm", m, sorted(ctx.items())))
        elif u < 0.85:  # future context: deferred, then released by the Add at exactly that counter
            c = up(top)
            if not c:
                continue
            ctx = dict(clock)
            ctx[a] = c
            ops.append(("rm", member(), sorted(ctx.items())))
            if rng.random() < 0.6:
                add(a, c, member())
        else:
            ops.append(("rm", member(), sorted((b, v) for b, v in clock.items() if rng.random() < 0.7) or [(a, 1)]))
    return ops[:n_ops]


# name -> (A, sparse, objects after the forced ones, [(share, state maker)])
def _tstate(A, **kw):
    return lambda r: pair(r, A, **kw)[0]


def _long_run(rng, A):
    """A state whose actors are the hot ones and some from 64 up, and a
    truncating clock that also holds every actor below 64: a run of more than
    64 entries, the ones that decide what is cut past its first 64."""
    S = pair(rng, A, acts=set(hot(A)) | set(rng.sample(range(64, A), rng.randint(8, 30))), n_keys=10, n_def=(1, 4))[0]
    T = truncating_clock(rng, S, A)
    for a in range(64):
        T.setdefault(a, rng.choice(EDGE))
    return S, T


TRUNCATE_SHAPES = {
    **{"fast_A%d" % A: (A, False, 600, [(0.7, _tstate(A, n_def=(1, 8))), (0.1, _tstate(A)),
                                        (0.1, _tstate(A, n_def=(10, 14))),
                                        (0.1, _tstate(A, n_keys=140, dots=1))]) for A in (8, 16, 32)},
    "lds_A16": (16, False, 400, [(0.4, _tstate(16, n_act=12, n_keys=40, dots=4, sides=(0.0, 1.0))),
                                 (0.3, _tstate(16, n_act=16, n_keys=30, dots=9, sides=(0.3, 0.7), n_def=(1, 4))),
                                 (0.3, _tstate(16, n_keys=110, dots=1, sides=(0.3, 0.7), n_def=(1, 4)))]),
    "hbm_A40": (40, False, 400, [(0.5, _tstate(40, n_def=(0, 3))), (0.25, _tstate(40, n_def=(10, 14))),
                                 (0.25, _tstate(40, n_keys=300, n_def=(0, 2)))]),
    "csr": (1024, True, 400, [(0.7, _tstate(1024, n_def=(0, 4))), (0.3, _tstate(1024, n_act=70))]),
    "long_run_A128": (128, False, 200, [(1.0, None)]),
}
# the forms (truncate_form) every shape must hold -> the fewest records of each
TRUNCATE_FORMS = {
    **{"fast_A%d" % A: {"fast": 400, "hbm": 20, "lds2": 40} for A in (8, 16, 32)},
    "lds_A16": {"lds1": 100, "lds2": 100}, "hbm_A40": {"hbm": 400}, "csr": {"hbm": 400}, "long_run_A128": {"hbm": 200},
}


def truncate_batch(name):
    """-> (A, sparse, states, truncating clocks): the forced states, then the shape's recipe shuffled."""
    A, sparse, n, recipe = TRUNCATE_SHAPES[name]
    rng = random.Random("orswot-truncate-" + name)
    states = [f[0] for f in forced(rng, A)]
    clocks = [truncating_clock(rng, S, A) for S in states]
    rest = []
    for share, make in recipe:
        for _ in range(round(share * n)):
            if make is None:
                rest.append(_long_run(rng, A))
            else:
                S = make(rng)
                rest.append((S, truncating_clock(rng, S, A)))
    rng.shuffle(rest)
    return A, sparse, states + [S for S, _ in rest], clocks + [T for _, T in rest]


# name -> (A, sparse, objects, most ops an object, [(share, state maker)])
APPLY_SHAPES = {
    "A16": (16, False, 500, 12, [(0.5, _tstate(16, n_def=(0, 2))), (0.2, _tstate(16, n_keys=110, dots=1, sides=(0.2, 0.8))),
                                 (0.15, _tstate(16, n_keys=60, dots=1, sides=(0.0, 1.0))),
                                 (0.15, _tstate(16, n_def=(24, 30)))]),
    "A64": (64, False, 300, 10, [(1.0, _tstate(64, n_def=(0, 2)))]),
    "csr": (1024, True, 400, 10, [(0.7, _tstate(1024, n_def=(0, 2))), (0.3, _tstate(1024, n_keys=90, dots=1))]),
}


def apply_batch(name):
    """-> (A, sparse, states, op lists). Object 0 holds key 1 and is given key
    0, object 1 holds key 2^64 - 2 and is given key 2^64 - 1; object 2 has no ops."""
    A, sparse, n, max_ops, recipe = APPLY_SHAPES[name]
    rng = random.Random("orswot-apply-" + name)
    states = [({0: 2**32}, {1: {0: 2**32}}, {}), ({0: 2**63}, {M64 - 1: {0: 2**63 - 1}}, {}),
              pair(rng, A, n_def=(1, 2))[0]] + [f[0] for f in forced(rng, A)]
    ops = [[("add", 0, 2**32, 0), ("add", 0, 2**32 + 1, 0), ("rm", 1, [(0, 2**32)]), ("add", A - 1, M64, 0)],
           [("add", 0, 2**63, M64), ("add", 0, 2**63 + 1, M64), ("rm", M64 - 1, [(0, 2**63 - 1)]),
            ("rm", M64, [(0, 2**63 + 1), (A - 1, 1)]), ("add", A - 1, 1, M64 - 1), ("add", 0, M64 - 1, M64)], []]
    for share, make in recipe:
        states += [make(rng) for _ in range(round(share * n))]
    ops += [ops_for(rng, S, A, rng.randint(0, max_ops)) for S in states[len(ops):]]
    return A, sparse, states, ops
