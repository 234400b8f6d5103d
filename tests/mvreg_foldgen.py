"""Test helper: R replicas' register slabs for the MVReg fold (crdt_mvreg_fold:
reps[0].merge(reps[1]).merge(reps[2])..., src/mvreg.rs:121-153), in the slab
layout of tests/mvreg_pairgen.py.

Every used slot of a register, in whichever replica, is a variant of one of a
few base rows shared by the whole register (mvreg_pairgen's pool and
_variant), so dominance and equality occur across and inside replicas at every
A, with u64 edge counters at the hot lane slots. A replica built this way is
often malformed (a slot dominated or repeated inside its own replica): the
chain keeps such slots as merge keeps them, and the fold must too. Every slot
past a count holds a poison row (all 2^64 - 1, which would dominate
everything) and a poison value: a fold that reads them gives another answer.

fold_np() is the one-pass rule of the header in numpy, with knobs that turn it
into deliberately wrong folds (MUTANTS); chain_np() chains
mvreg_pairgen.merge_np; classify() is a brute-force census of what the batch
holds, from a slot-by-slot simulation of the chain."""
import random

import numpy as np

import mvreg_pairgen as pg

POISON = 2**64 - 1
P_EMPTY_MIDDLE = 0.15
PLANT_EVERY = 8  # registers 5, 13, 21, ... hold a planted "equal to an earlier replica's clock, dominated by its own"
CLASSES = ("kept", "dom_earlier", "dom_later", "own_dom_kept", "chain3", "dup_in_rep0", "eq_own_earlier",
           "eq_kept_earlier", "eq_earlier_own_dom")


def gen(seed, n, A, caps, info=None):
    """-> R slabs (n, clk, val). Registers 0..3 are: all replicas full, only
    the last replica non-empty, only replica 0 non-empty, all empty; a middle
    replica is empty with probability P_EMPTY_MIDDLE. Every PLANT_EVERY-th
    register (in a batch of fewer than 2 PLANT_EVERY registers: every one
    but 1..3, so that five hold it) gets one row that no other row of the register is derived from,
    in replica r - 1 and again in replica r beside the row + 1 (r: the last
    replica of two or more slots): the case in which the chain keeps a clock
    equal to an earlier replica's, which wide registers never produce by
    chance. Values are 2^63 + the global slot index (replica by replica)."""
    rng = random.Random(seed)
    H, R = pg.hot(A), len(caps)
    reps = [(np.zeros(n, np.uint32), np.full((n, cap, A), POISON, np.uint64), np.full((n, cap), POISON, np.uint64))
            for cap in caps]
    g0 = np.concatenate([[0], np.cumsum(caps)]) * n
    touched = {}
    for i in range(n):
        cnt = [cap if rng.random() < 0.4 else rng.randint(0, cap) for cap in caps]
        for r in range(1, R - 1):
            if rng.random() < P_EMPTY_MIDDLE:
                cnt[r] = 0
        cnt = {0: list(caps), 1: [0] * (R - 1) + [caps[-1]], 2: [caps[0]] + [0] * (R - 1), 3: [0] * R}.get(i, cnt)
        # (a batch of a few registers: every register but the three forced degenerate ones)
        planted = i % PLANT_EVERY == 5 or (n < 2 * PLANT_EVERY and i not in (1, 2, 3))
        plant = max((r for r in range(1, R) if caps[r] >= 2), default=None) if planted else None
        if plant is not None:
            cnt[plant], cnt[plant - 1] = max(cnt[plant], 2), max(cnt[plant - 1], 1)
        total = sum(cnt)
        wide = total > pg.WIDE
        pool = []
        for _ in range(min(pg.POOL_MAX_WIDE if wide else pg.POOL_MAX, max(1, round(total / 3)))):
            slots = {pg._slot(rng, A, H) for _ in range(pg.BASE_NONZERO)} if A > pg.BASE_NONZERO else range(A)
            pool.append({s: rng.choice(pg.EDGE) for s in slots})
        for r, (cn, clk, val) in enumerate(reps):
            cn[i] = cnt[r]
            for k in range(cnt[r]):
                clk[i, k] = 0
                for s, c in pg._variant(rng, rng.choice(pool), A, H, touched, wide).items():
                    clk[i, k, s] = c
                val[i, k] = pg.VAL0 + int(g0[r]) + i * caps[r] + k
        if plant is not None:  # a fresh base row: last used slot of replica r - 1, and (row, row + 1) at the end of r
            slots = sorted({pg._slot(rng, A, H) for _ in range(pg.BASE_NONZERO)} if A > pg.BASE_NONZERO else range(A))
            row = np.zeros(A, np.uint64)
            row[slots] = [rng.choice(pg.EDGE) for _ in slots]
            row[slots[:2]] = pg.EDGE[-1]  # (so that hardly any row of the pool is above it)
            up = row.copy()
            up[rng.choice(slots)] += np.uint64(1)
            reps[plant - 1][1][i, cnt[plant - 1] - 1] = row
            reps[plant][1][i, cnt[plant] - 2], reps[plant][1][i, cnt[plant] - 1] = row, up
    if info is not None:
        info["touched"] = touched
    return reps


def tile(reps, n):
    """The batch repeated to n registers; values stay globally unique and the
    unused slots poisoned."""
    m = len(reps[0][0])
    idx = np.arange(n) % m
    out, g0 = [], 0
    for cn, clk, val in reps:
        cap = val.shape[1]
        g = pg.VAL0 + np.uint64(g0) + (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(cap)
                                       + np.arange(cap, dtype=np.uint64))
        used = np.arange(cap)[None, :] < cn[idx][:, None]
        out.append((cn[idx], clk[idx], np.where(used, g, np.uint64(POISON)).astype(np.uint64)))
        g0 += n * cap
    return out


# ----------------------------------------------------------- the fold in numpy
def _stack(reps):
    """-> used [n][T], clk [n][T][A], val [n][T], rep [T]: the capacity slots of all replicas in (r, k) order."""
    used = np.concatenate([np.arange(v.shape[1])[None, :] < cn[:, None] for cn, _, v in reps], axis=1)
    rep = np.concatenate([np.full(v.shape[1], r) for r, (_, _, v) in enumerate(reps)])
    return used, np.concatenate([c for _, c, _ in reps], axis=1), np.concatenate([v for _, _, v in reps], axis=1), rep


def relations(reps, key=None):
    """(gt, lt) bool [n][c][u]: some counter of slot c is > / < slot u's, under the compare `key`."""
    _, clk, _, _ = _stack(reps)
    k = pg._keyed(clk, key)
    return pg._flags(k, k)


def _emit(keep, order, clk, val, out_cap):
    n, A = clk.shape[0], clk.shape[2]
    outn = keep.sum(axis=1).astype(np.uint32)
    assert int(outn.max(initial=0)) <= out_cap
    outc, outv = np.zeros((n, out_cap, A), np.uint64), np.zeros((n, out_cap), np.uint64)
    ko = keep[:, order]
    rank = np.cumsum(ko, axis=1) - 1
    obj, j = np.nonzero(ko)
    outc[obj, rank[obj, j]] = clk[obj, order[j]]
    outv[obj, rank[obj, j]] = val[obj, order[j]]
    return outn, outc, outv


def fold_np(reps, out_cap, key=None, eq_dominates=False, dom_inside=False, simple_dedupe=False, dedupe_rep0=False,
            dedupe_inside=True, later_first=False, val_from_later=False, ignore_last=False, adjacent_only=False,
            cap_for_count=False, rel=None):
    """The fold's one-pass rule (include/crdts_hip.h) over slabs in numpy ->
    (n, clk, val), unused slots zero. Every knob makes it wrong in one way."""
    used, clk, val, rep = _stack(reps)
    R, T = len(reps), len(rep)
    if cap_for_count:
        used = np.ones_like(used)
    if ignore_last and R > 1:
        used = used & (rep != R - 1)[None, :]
    gt, lt = rel if rel is not None else relations(reps, key)
    pair = used[:, :, None] & used[:, None, :] & ~np.eye(T, dtype=bool)[None]
    less, eq = pair & lt & ~gt, pair & ~lt & ~gt  # [c][u]: slot c is strictly less than / equal to slot u
    same = (rep[:, None] == rep[None, :])[None]
    near = (np.abs(rep[:, None] - rep[None, :]) <= 1)[None] if adjacent_only else True
    earlier_rep = (rep[None, :] < rep[:, None])[None]        # u's replica is before c's
    earlier_own = same & np.tril(np.ones((T, T), bool), -1)[None]
    domo = ((less | (eq if eq_dominates else False)) & ~same & near).any(axis=2)
    domw = (less & same).any(axis=2)
    eqw = (eq & earlier_own).any(axis=2)
    eqe = (eq & earlier_rep & near).any(axis=2)
    dup = (eqw if dedupe_inside else False) | (eqe if simple_dedupe else eqe & ~domw)
    first = (rep == 0)[None, :]
    keep = used & ~domo & np.where(first, ~eqw if dedupe_rep0 else True, ~dup)
    if dom_inside:
        keep &= ~domw
    if val_from_later:  # the value of an equal clock taken from the last later replica that holds it
        later = eq & (rep[None, :] > rep[:, None])[None]
        last = T - 1 - np.argmax(later[:, :, ::-1], axis=2)
        val = np.where(later.any(axis=2), np.take_along_axis(val, last, axis=1), val)
    order = np.lexsort((np.arange(T), -rep)) if later_first else np.arange(T)
    return _emit(keep, order, clk, val, out_cap)


def _fit(slab, out_cap):
    n, clk, val = slab
    assert int(n.max(initial=0)) <= out_cap
    oc, ov = np.zeros((len(n), out_cap, clk.shape[2]), np.uint64), np.zeros((len(n), out_cap), np.uint64)
    m = min(out_cap, val.shape[1])
    oc[:, :m], ov[:, :m] = clk[:, :m], val[:, :m]
    return n.copy(), oc, ov


def chain(reps, out_cap, merge):
    """The R - 1 merges in rank order through merge(S, O, A, cap), every
    intermediate at the running sum of the capacities; then cut to out_cap."""
    cn, clk, val = reps[0]
    use = np.arange(val.shape[1])[None, :] < cn[:, None]
    acc = (cn.copy(), np.where(use[:, :, None], clk, np.uint64(0)), np.where(use, val, np.uint64(0)))
    for O in reps[1:]:
        acc = merge(acc, O, clk.shape[2], acc[2].shape[1] + O[2].shape[1])
    return _fit(acc, out_cap)


def chain_np(reps, out_cap):
    return chain(reps, out_cap, lambda S, O, A, cap: pg.merge_np(S, O, cap))


def chain_oracle(reps, out_cap):
    import oracle_ffi

    return chain(reps, out_cap, lambda S, O, A, cap: oracle_ffi.mvreg_merge(*S, *O, A, cap))


# name -> (knobs, can it differ for (A, caps)?)
def _two(caps):
    return max(caps) >= 2


MUTANTS = {
    "int64_compare": (dict(key="int64"), lambda A, caps: len(caps) > 1),
    "low32_compare": (dict(key="low32"), lambda A, caps: len(caps) > 1),
    "ignores_last_slot": (dict(key="drop_last"), lambda A, caps: len(caps) > 1),
    "ignores_slots_from_64": (dict(key="drop_ge64"), lambda A, caps: len(caps) > 1 and A > 64),
    "equal_is_dominated": (dict(eq_dominates=True), lambda A, caps: len(caps) > 1),
    "dominance_inside_a_replica": (dict(dom_inside=True), lambda A, caps: _two(caps)),
    "simple_dedupe": (dict(simple_dedupe=True), lambda A, caps: len(caps) > 1 and _two(caps[1:])),
    "dedupe_in_replica_0": (dict(dedupe_rep0=True), lambda A, caps: caps[0] >= 2),
    "no_dedupe_inside_a_replica": (dict(dedupe_inside=False), lambda A, caps: len(caps) > 1 and _two(caps[1:])),
    # (one actor: a total order, and then every survivor comes from one replica)
    "later_replicas_first": (dict(later_first=True), lambda A, caps: len(caps) > 1 and A > 1),
    "value_from_later_equal_clock": (dict(val_from_later=True), lambda A, caps: len(caps) > 1),
    "last_replica_ignored": (dict(ignore_last=True), lambda A, caps: len(caps) > 1),
    "adjacent_replicas_only": (dict(adjacent_only=True), lambda A, caps: len(caps) > 2),
    "capacity_for_count": (dict(cap_for_count=True), lambda A, caps: True),
}


# ------------------------------------------------------------------- census
def classify(reps):
    """-> (registers per class, the chain's output counts), by brute force:
    each register's chain is simulated slot by slot (which (r, k) is in the
    state after every merge), each class read off the definitions.
      kept                a slot that is in the output
      dom_earlier / dom_later    a clock of an earlier / later replica is > it
      own_dom_kept        only clocks of its own replica are > it; it is kept
      chain3              v < d < d' in three different replicas (d is dropped)
      dup_in_rep0         equal to an earlier slot of replica 0, and kept
      eq_own_earlier      r >= 1, equal to an earlier slot of replica r, no
                          other replica dominates it: dropped
      eq_kept_earlier     r >= 1, equal to a kept slot of an earlier replica: dropped
      eq_earlier_own_dom  r >= 1, equal to a slot of an earlier replica, a
                          clock of replica r is > both: kept"""
    used, clk, _, rep = _stack(reps)
    c = dict.fromkeys(CLASSES, 0)
    outn = np.zeros(len(used), np.uint32)
    R = len(reps)
    for i in range(len(used)):
        ix = np.nonzero(used[i])[0]
        rows, rp = clk[i, ix], rep[ix]
        le = (rows[:, None, :] <= rows[None, :, :]).all(axis=2)
        less, eq = le & ~le.T, le & le.T  # [a][b]: a < b, a == b
        state = np.nonzero(rp == 0)[0]
        for r in range(1, R):
            oth = np.nonzero(rp == r)[0]
            ks = ~less[np.ix_(state, oth)].any(axis=1) if len(oth) else np.ones(len(state), bool)
            ko = np.ones(len(oth), bool)
            for j, b in enumerate(oth):
                ko[j] = not (less[b, state].any() or eq[b, state[ks]].any() or eq[b, oth[:j]].any())
            state = np.concatenate([state[ks], oth[ko]])
        kept = np.zeros(len(ix), bool)
        kept[state] = True
        outn[i] = len(state)
        other, own = rp[:, None] != rp[None, :], rp[:, None] == rp[None, :]
        before = np.tril(np.ones((len(ix), len(ix)), bool), -1)  # [a][b]: b is before a
        dom_e = (less & (rp[None, :] < rp[:, None])).any(axis=1)
        dom_l = (less & (rp[None, :] > rp[:, None])).any(axis=1)
        dom_o, dom_w = (less & other).any(axis=1), (less & own).any(axis=1)
        eq_e = eq & (rp[None, :] < rp[:, None])
        three = False
        for d in np.nonzero(dom_o)[0]:
            below = np.nonzero(less[:, d] & other[:, d])[0]
            above = np.nonzero(less[d] & other[d])[0]
            three = three or any(rp[v] != rp[a] for v in below for a in above)
        has = {
            "kept": kept.any(), "dom_earlier": dom_e.any(), "dom_later": dom_l.any(),
            "own_dom_kept": (dom_w & ~dom_o & kept).any(), "chain3": three,
            "dup_in_rep0": ((eq & own & before).any(axis=1) & (rp == 0) & kept).any(),
            "eq_own_earlier": ((eq & own & before).any(axis=1) & (rp > 0) & ~dom_o & ~kept).any(),
            "eq_kept_earlier": ((eq_e & kept[None, :]).any(axis=1) & ~dom_o & ~kept).any(),
            "eq_earlier_own_dom": (eq_e.any(axis=1) & dom_w & kept).any(),
        }
        for k, v in has.items():
            c[k] += int(v)
    return c, outn


def possible(cls, caps):
    """Can the class occur with these capacities at all? The classes that need
    two slots in one replica cannot where that replica has one; chain3 needs
    three replicas, the classes across replicas two."""
    R = len(caps)
    return {"kept": True, "dom_earlier": R > 1, "dom_later": R > 1, "own_dom_kept": max(caps) >= 2, "chain3": R > 2,
            "dup_in_rep0": caps[0] >= 2, "eq_own_earlier": R > 1 and max(caps[1:]) >= 2, "eq_kept_earlier": R > 1,
            "eq_earlier_own_dom": R > 1 and max(caps[1:]) >= 2}[cls]


# ------------------------------------------------ shapes and launch tiers
LDS_BYTES = 60 * 1024


def per_wave_bytes(A, caps):
    """A wave's LDS in the fast kernel: the rows, two 64-bit relation sets per slot, two T-byte tables."""
    T = sum(caps)
    return (8 * T * A + 18 * T + 15) & ~15


def tier(A, caps, out_cap=None):
    """The kernel and waves per block crdt_mvreg_fold takes by the rule of its
    header (include/crdts_hip.h): "big", or "W4" / "W3" / "W2" / "W1". out_cap
    has no part in it."""
    per_wave = per_wave_bytes(A, caps)
    if per_wave > LDS_BYTES or sum(caps) > 64:
        return "big"
    return "W{}".format(max(W for W in (1, 2, 3, 4) if W == 1 or W * per_wave <= LDS_BYTES))


# (A, caps, n, tier)
SHAPES = (
    # fast kernel, 4 waves per block
    [(8, (4, 4, 4), 500, "W4"), (2, (3, 5, 2, 4), 500, "W4"), (1, (4,) * 5, 500, "W4"), (33, (1,) * 32, 300, "W4"),
     (64, (3, 3, 3), 400, "W4"), (65, (2, 6, 3), 400, "W4"), (129, (2, 2, 2), 400, "W4"),
     (5, (16, 7, 3, 9, 2, 4, 4, 4), 300, "W4")]
    # 3 / 2 / 1 waves per block: 96 A + 216 bytes per wave, rounded up to 16
    + [(200, (4, 4, 4), 300, "W3"), (300, (4, 4, 4), 300, "W2"), (600, (4, 4, 4), 300, "W1")]
    # the 64-slot boundary, as two and as eight replicas
    + [(8, (32, 32), 300, "W4"), (8, (32, 33), 300, "big"), (8, (8,) * 8, 300, "W4"), (8, (8,) * 7 + (9,), 300, "big")]
    # the 60 KB boundary: 61,376 and 61,472 bytes per wave
    + [(637, (4, 4, 4), 300, "W1"), (638, (4, 4, 4), 300, "big")]
    # the one-wave kernel
    + [(2, (65, 8, 8), 300, "big"), (8, (100, 70, 30), 100, "big"), (4, (1024, 1024), 8, "big"),
       (4, (64,) * 32, 8, "big"), (512, (16, 16, 16), 300, "big")]
)
FAST, BIG = SHAPES[0], (8, (40, 30, 20), 100, "big")
EXTRA_SHAPES = [BIG]  # the big kernel's shape of the grid-stride, small-n, out_cap and status tests


def shape_id(s):
    return "A{}-{}".format(s[0], "x".join(map(str, s[1])) if len(s[1]) < 6 or len(set(s[1])) > 1
                           else "{}r{}".format(s[1][0], len(s[1])))


def seed_of(shape):
    A, caps, n, _ = shape
    return 0xF01D + 7 * A + 3 * len(caps) + sum((k + 1) * c for k, c in enumerate(caps)) + SEED_BUMP.get(shape[:2], 0)


# seeds moved off the default where a class of the census fell short
SEED_BUMP = {(4, (1024, 1024)): 1}  # (at the default one planted row met a larger row of the other replica)
