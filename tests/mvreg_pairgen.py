"""Test helper: structured register pairs for MVReg<u64, A>::merge
(src/mvreg.rs:121-153) and row pairs for VClock::partial_cmp
(src/vclock.rs:59-71), in the slab layout of tests/mvreg_opgen.py::slab.

I.i.d. random rows are all concurrent once A is large, so a merge of them only
copies both sides. Here every used slot of a pair is a variant of one of a few
base rows (the row, one slot +1, one nonzero slot -1, one slot +1 and another
-1), so dominance in both directions, equal clocks across the sides and
duplicates inside a side all occur at every A; counters come from the edges of
u64 and the touched slots from the ends of the lane mappings.

classify() counts the outcome classes by brute force, merge_np() is a numpy
restatement of the merge whose knobs turn it into deliberately wrong merges
(MUTANTS), and cmp_np() the same for partial_cmp (CMP_MUTANTS): what the
generated inputs must tell apart."""
import random

import numpy as np

EDGE = (1, 2, 3, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 2)
# the counter pairs one differing slot of a partial_cmp pair holds (smaller, larger)
CMP_PAIRS = ((2**32 - 1, 2**32), (2**63 - 1, 2**63), (2**64 - 2, 2**64 - 1), (0, 1), (0, 2**63))
VAL0 = 2**63
BASE_NONZERO = 6
# base rows per object: (ns + no) / 3, at most 24; 8 for registers of hundreds of slots, where with more
# base rows at a few actors nearly every row of the small side is dominated and equal kept clocks die out
POOL_MAX, POOL_MAX_WIDE, WIDE = 24, 8, 512
CLASSES = ("self_kept", "self_dom", "other_kept", "other_dom", "other_eq_self", "other_eq_other")


def hot(A):
    """The slot indices at the ends of the lane mappings."""
    return sorted({0, A // 2, min(A - 1, 63), min(A - 1, 64), A - 1})


def _slot(rng, A, H):
    return rng.choice(H) if rng.random() < 0.5 else rng.randrange(A)


def _variant(rng, base, A, H, touched, wide=False):
    """base: {slot: counter} -> a variant of it; the touched slots are counted.
    The row itself 40 %, the other three 20 % each; in a wide register 10 % and
    50 % "+1" (there every base row meets a "+1" of itself on the other side
    and is dominated: the clocks that are kept and equal are the "+1" rows)."""
    row = dict(base)
    u = rng.random()
    if wide:
        u = 0.4 * u / 0.1 if u < 0.1 else 0.4 + 0.2 * (u - 0.1) / 0.5 if u < 0.6 else 0.6 + (u - 0.6)
    if u < 0.4:
        return row
    x = _slot(rng, A, H)

    def bump(s, d):
        row[s] = row.get(s, 0) + d
        if not row[s]:
            del row[s]
        touched[s] = touched.get(s, 0) + 1

    def nonzero(avoid):
        """The slot to decrement: x when it may be and is nonzero, else a hot nonzero slot half the time."""
        if avoid is None and x in row:
            return x
        nz = [s for s in row if s != avoid]
        hz = [s for s in nz if s in H]
        if not nz:
            return None
        return rng.choice(hz) if hz and rng.random() < 0.5 else rng.choice(nz)

    if u < 0.6:  # one slot +1
        bump(x, 1)
    elif u < 0.8:  # one nonzero slot -1
        bump(nonzero(None), -1)
    else:  # one slot +1 and another -1: concurrent with the base row (only the +1 when there is no other slot)
        y = nonzero(x)
        bump(x, 1)
        if y is not None:
            bump(y, -1)
    return row


def gen(seed, n, A, scap, ocap, info=None):
    """-> (sn, sclk, sval), (on, oclk, oval): n register pairs. Objects 0..3
    are: both sides full, ns = 0, no = 0, both 0. Values are 2^63 + the global
    slot index (self's slots, then other's). `info`, a dict, receives
    `touched`: how often each slot index was the +1 / -1 slot."""
    rng = random.Random(seed)
    H = hot(A)
    sn, on = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    sclk, oclk = np.zeros((n, scap, A), np.uint64), np.zeros((n, ocap, A), np.uint64)
    sval, oval = np.zeros((n, scap), np.uint64), np.zeros((n, ocap), np.uint64)
    touched = {}
    forced = {0: (scap, ocap), 1: (0, ocap), 2: (scap, 0), 3: (0, 0)}
    for i in range(n):
        ns = scap if rng.random() < 0.4 else rng.randint(0, scap)
        no = ocap if rng.random() < 0.4 else rng.randint(0, ocap)
        ns, no = forced.get(i, (ns, no))
        sn[i], on[i] = ns, no
        pool = []
        for _ in range(min(POOL_MAX_WIDE if ns + no > WIDE else POOL_MAX, max(1, round((ns + no) / 3)))):
            slots = {_slot(rng, A, H) for _ in range(BASE_NONZERO)} if A > BASE_NONZERO else range(A)
            pool.append({s: rng.choice(EDGE) for s in slots})
        for cnt, clk, val, cap, g0 in ((ns, sclk, sval, scap, 0), (no, oclk, oval, ocap, n * scap)):
            for k in range(cnt):
                for s, c in _variant(rng, rng.choice(pool), A, H, touched, ns + no > WIDE).items():
                    clk[i, k, s] = c
                val[i, k] = VAL0 + g0 + i * cap + k
    if info is not None:
        info["touched"] = touched
    return (sn, sclk, sval), (on, oclk, oval)


def tile(S, O, n):
    """The pair batch repeated to n objects; values stay globally unique
    (2^63 + the global slot index of the tiled batch)."""
    (sn, sclk, sval), (on, oclk, oval) = S, O
    m, scap, ocap = len(sn), sval.shape[1], oval.shape[1]
    idx = np.arange(n) % m
    gs = VAL0 + (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(scap) + np.arange(scap, dtype=np.uint64))
    go = VAL0 + np.uint64(n * scap) + (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(ocap)
                                      + np.arange(ocap, dtype=np.uint64))
    used = lambda cnt, cap: np.arange(cap)[None, :] < cnt[idx][:, None]  # noqa: E731
    return ((sn[idx], sclk[idx], np.where(used(sn, scap), gs, 0).astype(np.uint64)),
            (on[idx], oclk[idx], np.where(used(on, ocap), go, 0).astype(np.uint64)))


# ------------------------------------------------------------ merge in numpy
def _keyed(clk, key):
    """The rows as a wrong compare sees them (None: as they are)."""
    if key is None:
        return clk
    if key == "int64":
        return clk.view(np.int64)
    if key == "low32":
        return clk & np.uint64(0xFFFFFFFF)
    if key == "drop_last":
        return clk[..., :-1]
    if key == "drop_ge64":
        return clk[..., :64]
    raise ValueError(key)


def _flags(X, Y):
    """X [n][p][A], Y [n][q][A] -> (gt, lt) bool [n][p][q]: some X > Y, some X < Y."""
    n, p, q = X.shape[0], X.shape[1], Y.shape[1]
    gt, lt = np.zeros((n, p, q), bool), np.zeros((n, p, q), bool)
    step = max(1, (1 << 23) // max(1, p * q * max(1, X.shape[2])))
    for a in range(0, n, step):
        x, y = X[a:a + step, :, None, :], Y[a:a + step, None, :, :]
        gt[a:a + step] = (x > y).any(axis=-1)
        lt[a:a + step] = (x < y).any(axis=-1)
    return gt, lt


def relations(S, O, key=None):
    """The pairwise clock relations of a batch under the compare `key`."""
    (sn, sclk, _), (on, oclk, _) = S, O
    us = np.arange(sclk.shape[1])[None, :] < sn[:, None]
    uo = np.arange(oclk.shape[1])[None, :] < on[:, None]
    ks, ko = _keyed(sclk, key), _keyed(oclk, key)
    gso, lso = _flags(ks, ko)  # self i vs other j
    goo, loo = _flags(ko, ko)
    pair = us[:, :, None] & uo[:, None, :]
    return dict(us=us, uo=uo, s_lt_o=pair & lso & ~gso, s_gt_o=pair & gso & ~lso, s_eq_o=pair & ~gso & ~lso,
                o_eq_o=uo[:, :, None] & uo[:, None, :] & ~goo & ~loo)


def merge_np(S, O, out_cap, key=None, eq_dominates=False, dedupe_other=True, dedupe_self=True, other_first=False,
             val_from_other=False, rel=None):
    """MVReg::merge over slabs in numpy -> (n, clk, val), unused slots zero.
    With the defaults it restates src/mvreg.rs:121-153; every knob makes it
    wrong in one way (MUTANTS)."""
    (sn, sclk, sval), (on, oclk, oval) = S, O
    n, scap, ocap, A = len(sn), sval.shape[1], oval.shape[1], sclk.shape[2]
    r = rel if rel is not None else relations(S, O, key)
    dom_s = r["s_lt_o"] | (r["s_eq_o"] if eq_dominates else False)
    dom_o = r["s_gt_o"] | (r["s_eq_o"] if eq_dominates else False)
    keep_s = r["us"] & ~dom_s.any(axis=2)
    keep_o = r["uo"] & ~dom_o.any(axis=1)
    eq_kept = (r["s_eq_o"] & keep_s[:, :, None])  # [n][i][j]: other j equals kept self i
    if dedupe_self:
        keep_o &= ~eq_kept.any(axis=1)
    if dedupe_other:
        earlier = np.tril(np.ones((ocap, ocap), bool), -1)  # [j][jj]: jj < j
        keep_o &= ~(r["o_eq_o"] & earlier[None]).any(axis=2)
    sval = sval.copy()
    if val_from_other:  # the value of an equal clock taken from the other side
        i_idx = np.argmax(eq_kept, axis=2)  # the first equal other slot
        has = eq_kept.any(axis=2)
        sval[has] = np.take_along_axis(oval, i_idx, axis=1)[has]
    outn = (keep_s.sum(axis=1) + keep_o.sum(axis=1)).astype(np.uint32)
    assert int(outn.max(initial=0)) <= out_cap
    outc, outv = np.zeros((n, out_cap, A), np.uint64), np.zeros((n, out_cap), np.uint64)
    rs = np.cumsum(keep_s, axis=1) - 1
    ro = np.cumsum(keep_o, axis=1) - 1
    if other_first:
        rs += keep_o.sum(axis=1)[:, None]
    else:
        ro += keep_s.sum(axis=1)[:, None]
    for keep, rank, clk, val in ((keep_s, rs, sclk, sval), (keep_o, ro, oclk, oval)):
        obj, slot = np.nonzero(keep)
        outc[obj, rank[obj, slot]] = clk[obj, slot]
        outv[obj, rank[obj, slot]] = val[obj, slot]
    return outn, outc, outv


# name -> (knobs, can it differ at actor count A?)
MUTANTS = {
    "int64_compare": (dict(key="int64"), lambda A: True),
    "low32_compare": (dict(key="low32"), lambda A: True),
    "ignores_last_slot": (dict(key="drop_last"), lambda A: True),  # (at A = 1 every row compares equal)
    "ignores_slots_from_64": (dict(key="drop_ge64"), lambda A: A > 64),
    "equal_is_dominated": (dict(eq_dominates=True), lambda A: True),
    "no_dedupe_against_other": (dict(dedupe_other=False), lambda A: True),
    "no_dedupe_against_self": (dict(dedupe_self=False), lambda A: True),
    "other_before_self": (dict(other_first=True), lambda A: A > 1),  # (one actor: a total order, one side survives)
    "equal_clock_val_from_other": (dict(val_from_other=True), lambda A: True),
}


def classify(S, O):
    """Counts of the outcome classes of every used slot, by brute force from
    the rule itself (src/mvreg.rs:121-153) -> (dict, per-object output counts).
    self_kept / self_dom: no / some other clock is strictly greater.
    other_dom: some self clock is strictly greater; else other_eq_self: equal
    to a kept self clock; else other_eq_other: equal to an earlier other clock
    (which is kept, or this one would have been dropped with it); else
    other_kept. dup_in_self: self slots equal to an earlier self slot."""
    (sn, sclk, _), (on, oclk, _) = S, O
    c = dict.fromkeys(CLASSES + ("dup_in_self",), 0)
    outn = np.zeros(len(sn), np.uint32)
    for i in range(len(sn)):
        s, o = sclk[i, :sn[i]], oclk[i, :on[i]]
        le = (s[:, None, :] <= o[None, :, :]).all(axis=2)  # [i][j]: s_i <= o_j
        ge = (s[:, None, :] >= o[None, :, :]).all(axis=2)
        kept_s = ~(le & ~ge).any(axis=1)
        c["self_kept"] += int(kept_s.sum())
        c["self_dom"] += int((~kept_s).sum())
        for k in range(1, len(s)):
            c["dup_in_self"] += int((s[:k] == s[k]).all(axis=1).any())
        for j in range(len(o)):
            if (ge[:, j] & ~le[:, j]).any():
                c["other_dom"] += 1
            elif (ge[:, j] & le[:, j] & kept_s).any():
                c["other_eq_self"] += 1
            elif j and (o[:j] == o[j]).all(axis=1).any():
                c["other_eq_other"] += 1
            else:
                c["other_kept"] += 1
                outn[i] += 1
        outn[i] += int(kept_s.sum())
    return c, outn


# ------------------------------------------------------------- partial_cmp
def cmp_rows(seed, A):
    """-> (a, b) u64 [n][A]: for every slot x four pairs over one base row of
    edge counters (equal; a > b at x only; a < b at x only; a > b at x and
    a < b at another slot), the differing counters from CMP_PAIRS; then one
    more pair and three more, so that n is no multiple of the pairs per wave."""
    rng = random.Random(seed)
    a, b = np.zeros((4 * A + 4, A), np.uint64), np.zeros((4 * A + 4, A), np.uint64)

    def base():
        return np.array([rng.choice(EDGE) if rng.random() < 0.75 else 0 for _ in range(A)], np.uint64)

    for x in range(A):
        for t in range(4):
            a[4 * x + t] = b[4 * x + t] = base()
        lo, hi = rng.choice(CMP_PAIRS)
        a[4 * x + 1, x], b[4 * x + 1, x] = hi, lo
        lo, hi = rng.choice(CMP_PAIRS)
        a[4 * x + 2, x], b[4 * x + 2, x] = lo, hi
        lo, hi = rng.choice(CMP_PAIRS)
        a[4 * x + 3, x], b[4 * x + 3, x] = hi, lo
        if A > 1:
            y = rng.choice([s for s in {0, A // 2, A - 1, (x + 1) % A, rng.randrange(A)} if s != x])
            lo, hi = rng.choice(CMP_PAIRS)
            a[4 * x + 3, y], b[4 * x + 3, y] = lo, hi
    for t in range(4):  # the tail: pairs at the last slot again
        a[4 * A + t] = b[4 * A + t] = base()
    lo, hi = CMP_PAIRS[1]
    a[4 * A + 1, A - 1], b[4 * A + 1, A - 1] = hi, lo
    a[4 * A + 2, A - 1], b[4 * A + 2, A - 1] = lo, hi
    a[4 * A + 3, A - 1], b[4 * A + 3, A - 1] = hi, lo
    if A > 1:
        a[4 * A + 3, 0], b[4 * A + 3, 0] = lo, hi
    return a[:4 * A + 3], b[:4 * A + 3]  # 4A + 3 pairs: odd


def cmp_np(a, b, key=None):
    """partial_cmp of dense rows in numpy: 0 Equal, 1 Greater, -1 Less, 2 None."""
    a, b = _keyed(a, key), _keyed(b, key)
    gt, lt = (a > b).any(axis=1), (a < b).any(axis=1)
    return np.where(gt & lt, 2, np.where(gt, 1, np.where(lt, -1, 0))).astype(np.int8)


CMP_MUTANTS = {name: MUTANTS[name] for name in ("int64_compare", "low32_compare", "ignores_last_slot",
                                                 "ignores_slots_from_64")}


# ------------------------------------------------ shapes and launch tiers
LDS_BYTES = 60 * 1024


def per_wave_bytes(A, scap, ocap, out_cap=None):
    """A wave's LDS in the fast kernel (out_cap defaults to the capacities' sum)."""
    out_cap = scap + ocap if out_cap is None else out_cap
    return (8 * (scap + ocap) * A + scap * ocap + ocap * ocap + out_cap + 15) & ~15


def tier(A, scap, ocap, out_cap=None):
    """The kernel and waves per block crdt_mvreg_merge takes by the rule of its
    header (include/crdts_hip.h): "big", or "W4" / "W3" / "W2" / "W1"."""
    per_wave = per_wave_bytes(A, scap, ocap, out_cap)
    if per_wave > LDS_BYTES or scap > 64 or ocap > 64:
        return "big"
    return "W{}".format(max(W for W in (1, 2, 3, 4) if W == 1 or W * per_wave <= LDS_BYTES))


# (A, self_cap, other_cap, n, tier at out_cap = self_cap + other_cap)
SHAPES = (
    # fast kernel, 4 waves per block, actor widths around the lane mappings
    [(A, s, o, 1000, "W4") for A, s, o in ((1, 4, 4), (2, 3, 5), (3, 1, 7), (5, 16, 7), (31, 4, 4), (32, 4, 4),
                                           (33, 4, 4), (63, 3, 3), (64, 3, 3), (65, 2, 6), (100, 3, 3), (127, 2, 2),
                                           (128, 2, 2), (129, 2, 2))]
    # fast kernel, 3 / 2 / 1 waves per block: 64 A + 40 bytes per wave, rounded up to 16
    + [(300, 4, 4, 1000, "W3"), (400, 4, 4, 1000, "W2"), (600, 4, 4, 1000, "W1")]
    # the 64-slot boundary and the 60 KB boundary (61,424 and 61,504 bytes per wave)
    + [(8, 64, 64, 200, "W3"), (8, 65, 64, 200, "big"), (8, 64, 65, 200, "big")]
    + [(767, 5, 5, 300, "W1"), (768, 5, 5, 300, "big")]
    # the one-wave kernel ((8, 100, 70) at 100 objects: the Python restatement of it is slow; 1,024 slots at 8)
    + [(2, 65, 8, 1000, "big"), (8, 100, 70, 100, "big"), (4, 1024, 8, 8, "big"), (512, 16, 16, 1000, "big")]
)
# the shapes of the grid-stride, small-n, out_cap and status tests
EXTRA_SHAPES = [(8, 4, 4, 1000, "W4"), (8, 70, 70, 100, "big")]


def shape_id(s):
    return "A{}-s{}-o{}".format(*s[:3])
