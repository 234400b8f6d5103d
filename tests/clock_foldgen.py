"""Test helper: R replicas' runs for the clock fold (crdt_clock_csr_fold,
rust-crdt_amd/csrc/clock_fold.hip). Runs are built directly, not drawn, over
clock_rungen's universe (actors astride 2^31) with its counter PAIRS (one apart
across 2^32, 2^63 and up to 2^64 - 1) on every actor that two replicas share:
R in REPS, per-replica lengths from LENGTHS and a few hundred, the lengths' sum
on both sides of 64 and of the LDS tier's limit (`stage`, which the tests read
from the package), a shared actor held by every replica / only the first /
only the last / only the first and the last, its largest counter in the first,
a middle or the last holder or tied, shared actors at index 0, 63, 64 and last
of a run, empty first / middle / last replicas, all replicas empty, unions of
exactly 64 and 65 actors.

An object is a tuple of R runs, a run a tuple of (actor, counter). fold_dict is
the plain reference; ref_fold restates the kernel's walk (an entry's place is
the sum of its actor's ranks in the R runs; the first holder owns the actor and
carries the largest counter; the tier caps what a wave can hold) with knobs
that make it wrong in one way each (MUTANTS). census() says which case is
present how often. Every batch is made once and is read-only by convention."""
import bisect
import functools
import random

import clock_rungen as cr

REPS = (1, 2, 3, 8, 32)
LENGTHS = (0, 1, 63, 64, 65)
REGS = 64  # the register tier holds this many entries


def fold_dict(reps):
    d = {}
    for run in reps:
        for a, c in run:
            if c > d.get(a, 0):
                d[a] = c
    return sorted(d.items())


def tier(reps, stage):
    T = sum(len(r) for r in reps)
    return "regs" if T <= REGS else "lds" if T <= stage else "mem"


# ------------------------------------------------------------------ building
def _window(rng, width, region):
    """A slice of universe indices `width` wide: below 2^31, astride it, at and above it."""
    U = cr.universe()
    m = bisect.bisect_left(U, 2**31)
    lo = (rng.randrange(0, max(1, m - width)), max(0, m - width // 2), rng.randrange(m, max(m + 1, len(U) - width)))[region]
    return list(range(lo, min(len(U), lo + width)))


def _with_counters(rng, idx_runs, mode=None):
    """Counters for runs of universe indices: an actor that several replicas
    hold takes a PAIRS pair, the larger counter at the holder `mode` names
    (first / middle / last), at two holders (tied), or nowhere (equal)."""
    U = cr.universe()
    holders = {}
    for r, run in enumerate(idx_runs):
        for k in run:
            holders.setdefault(k, []).append(r)
    ctr = [dict() for _ in idx_runs]
    for k, hs in holders.items():
        if len(hs) == 1:
            ctr[hs[0]][k] = cr._counter(rng)
            continue
        lo, hi = rng.choice(cr.PAIRS)
        md = mode or rng.choice(("first", "middle", "last", "tied", "equal"))
        top = {"first": hs[:1], "middle": hs[len(hs) // 2:len(hs) // 2 + 1], "last": hs[-1:],
               "tied": [hs[0], hs[-1]] if len(hs) < 3 else rng.sample(hs, 2), "equal": []}[md]
        for r in hs:
            ctr[r][k] = hi if r in top else lo
    return tuple(tuple((U[k], ctr[r][k]) for k in run) for r, run in enumerate(idx_runs))


def _sampled(rng, lens, region, shared=None, holders=(), mode=None):
    """Runs of the given lengths sampled from one window (so that replicas
    share actors by chance); the index `shared` of the window is held by the
    replicas `holders` alone."""
    win = _window(rng, max(2 * max(lens + [1]), 80), region)
    x = None if shared is None else win[shared % len(win)]
    pool = [k for k in win if k != x]
    runs = []
    for r, n in enumerate(lens):
        hold = x is not None and r in holders and n >= 1
        run = rng.sample(pool, n - hold) + ([x] if hold else [])
        runs.append(sorted(run))
    return _with_counters(rng, runs, mode)


def _anchored(rng, lens, region):
    """clock_rungen's anchors: the runs share the actors at index 0, 63, 64 and last whenever they reach them."""
    U = cr.universe()
    m = bisect.bisect_left(U, 2**31)
    i0 = (0, m - 40, m)[region] + rng.randrange(0, 4)
    i63 = i0 + 1 + rng.randrange(130, 260)
    ilast = len(U) - 1 - rng.randrange(0, 3)
    return _with_counters(rng, [cr._side(rng, n, i0, i63, ilast) for n in lens])


def _split(rng, total, R, how):
    """`total` entries over R replicas: even, all in the first / a middle / the last, or a random composition."""
    if how == "even":
        return [total // R + (r < total % R) for r in range(R)]
    if how in ("first", "middle", "last"):
        at = {"first": 0, "middle": R // 2, "last": R - 1}[how]
        return [total if r == at else 0 for r in range(R)]
    cuts = sorted(rng.randrange(0, total + 1) for _ in range(R - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def _union_of(rng, size, R, region):
    """R runs whose union has exactly `size` actors."""
    win = _window(rng, size, region)
    runs = [sorted(rng.sample(win, rng.randrange(size // 4, size // 2 + 1))) for _ in range(R)]
    at = rng.randrange(R)  # this replica holds what no other does
    others = set().union(*[r for q, r in enumerate(runs) if q != at])
    runs[at] = sorted(set(runs[at]) | (set(win) - others))
    return _with_counters(rng, runs)


@functools.lru_cache(maxsize=None)
def batch(R, stage, seed=0xF01D):
    """The objects of one fold of R replicas -> a tuple of objects."""
    rng = random.Random(seed * 64 + R)
    objs = []
    big = (200, 300, 700)
    n_reg = 0
    for rep in range(40):  # anchored runs: lengths from LENGTHS and a few hundred
        if R <= 3:
            lens = [rng.choice(LENGTHS + (300,)) for _ in range(R)]
        else:  # a few long runs among short ones
            lens = [rng.choice(LENGTHS + (300,)) if rng.random() < 4 / R else rng.choice((0, 1, 1, 2)) for _ in range(R)]
        objs.append(_anchored(rng, lens, rep % 3))
    for total in (63, 64, 65, stage - 1, stage, stage + 1):  # the tier boundaries
        for how in ("even", "first", "middle", "last", "random"):
            for _ in range(2):
                lens = _split(rng, total, R, how)
                objs.append(_sampled(rng, lens, n_reg % 3, shared=n_reg, holders=range(R)))
                n_reg += 1
    for size in (64, 65):  # the union's size
        for _ in range(6):
            objs.append(_union_of(rng, size, R, n_reg % 3))
            n_reg += 1
    for _ in range(5):  # empty replicas
        objs.append(tuple(() for _ in range(R)))
        for at in (0, R // 2, R - 1):
            lens = [0 if r == at else rng.choice((1, 5, 40, 64, 65)) for r in range(R)]
            objs.append(_sampled(rng, lens, n_reg % 3))
            n_reg += 1
    pats = {"every": range(R), "first": (0,), "last": (R - 1,), "first_last": (0, R - 1)}
    for pat, holders in pats.items():  # who holds the shared actor, and where its largest counter sits
        for mode in ("first", "middle", "last", "tied", "equal"):
            for per in (64 // R or 1, max(2, (stage - 40) // R), stage // R + 30):  # one object per tier
                lens = [max(1, per + rng.randrange(-1, 2)) for _ in range(R)]
                objs.append(_sampled(rng, lens, n_reg % 3, shared=n_reg * 7, holders=holders, mode=mode))
                n_reg += 1
    for _ in range(6):  # long runs
        lens = [rng.choice(big) if r in (0, R // 2, R - 1) else rng.choice((0, 1, 40)) for r in range(R)]
        objs.append(_sampled(rng, lens, n_reg % 3, shared=n_reg, holders=(0, R - 1)))
        n_reg += 1
    if len(objs) % 64 == 0:  # the last chunk of a launch is partial
        objs.append(_sampled(rng, [3] * R, 1))
    return tuple(objs)


# ------------------------------------------- the kernel's walk, with wrong knobs
def ref_fold(reps, stage, last_counter=False, counter_compare=None, actor_order_signed=False, keep_first_dup=False,
             skip=None, regs_max=REGS, stage_max=None):
    """The union the walk of clock_fold.hip gives: each entry's place is the sum
    of its actor's ranks in the runs; the first holder owns the actor with the
    holders' largest counter; owners come out by place. A tier holds REGS /
    `stage` entries of the runs laid end to end, whatever the boundary says."""
    ck, ak = cr._ckey(counter_compare), cr._akey(actor_order_signed)
    stage_max = stage if stage_max is None else stage_max
    runs = [list(r) for q, r in enumerate(reps) if q != skip]
    T = sum(len(r) for r in runs)
    cap = REGS if T <= regs_max else stage if T <= stage_max else T
    held, room = [], cap
    for r in runs:  # what the tier's lanes / stage can hold
        held.append(r[:room])
        room -= len(held[-1])
    keys = [[ak(a) for a, _ in r] for r in held]
    out = []
    for r, run in enumerate(held):
        for k, (a, c) in enumerate(run):
            p, cm, first = 0, c, True
            for q, other in enumerate(held):
                b = k if q == r else bisect.bisect_left(keys[q], ak(a))
                p += b
                if b < len(other) and other[b][0] == a:
                    if last_counter:
                        cm = other[b][1]
                    elif ck(other[b][1]) > ck(cm):
                        cm = other[b][1]
                    if q < r and not (keep_first_dup and q == 0):
                        first = False
            if first:
                out.append((p, a, cm))
    return [(a, c) for _, a, c in sorted(out)]


def mutants(R, stage):
    """name -> knobs; `skip` names a replica of this R."""
    return {"last_counter": dict(last_counter=True), "counter_compare_low32": dict(counter_compare="low32"),
            "actor_order_signed": dict(actor_order_signed=True), "keep_first_dup": dict(keep_first_dup=True),
            "skip_replica": dict(skip=R // 2), "regs_boundary_off_by_one": dict(regs_max=REGS + 1),
            "stage_boundary_off_by_one": dict(stage_max=stage + 1)}


MUTANTS = tuple(mutants(2, 0))


def differs(objs, stage, knobs):
    """Does the walk with the knobs give another union on some object of the batch?"""
    return any(ref_fold(o, stage, **knobs) != fold_dict(o) for o in objs)


# ------------------------------------------------------------------- census
def census(objs, stage):
    """How many objects hold each case (the cases of the module docstring)."""
    c = dict(regs=0, lds=0, mem=0, sum63=0, sum64=0, sum65=0, sum_stage_m1=0, sum_stage=0, sum_stage_p1=0,
             held_by_every=0, held_by_first_only=0, held_by_last_only=0, held_by_first_and_last_only=0,
             max_in_first=0, max_in_middle=0, max_in_last=0, max_tied=0, shared_idx0=0, shared_idx63=0,
             shared_idx64=0, shared_last=0, empty_first=0, empty_middle=0, empty_last=0, all_empty=0, union64=0,
             union65=0, len0=0, len1=0, len63=0, len64=0, len65=0, len_hundreds=0, astride_2_31=0)
    for reps in objs:
        R = len(reps)
        lens = [len(r) for r in reps]
        T = sum(lens)
        c[tier(reps, stage)] += 1
        for name, v in (("sum63", 63), ("sum64", 64), ("sum65", 65), ("sum_stage_m1", stage - 1), ("sum_stage", stage),
                        ("sum_stage_p1", stage + 1)):
            c[name] += T == v
        for n in LENGTHS:
            c[f"len{n}"] += n in lens
        c["len_hundreds"] += any(n >= 200 for n in lens)
        holders = {}
        for r, run in enumerate(reps):
            for k, (a, v) in enumerate(run):
                holders.setdefault(a, []).append((r, k, v))
        pats = set()
        for a, hs in holders.items():
            rs = [r for r, _, _ in hs]
            if R >= 2 and len(rs) == R:
                pats.add("held_by_every")
            if R >= 2 and rs == [0]:
                pats.add("held_by_first_only")
            if R >= 2 and rs == [R - 1]:
                pats.add("held_by_last_only")
            if R >= 3 and rs == [0, R - 1]:
                pats.add("held_by_first_and_last_only")
            if len(hs) < 2:
                continue
            top = max(v for _, _, v in hs)
            at = [j for j, (_, _, v) in enumerate(hs) if v == top]
            if len(at) >= 2:
                pats.add("max_tied")
            elif at[0] == 0:
                pats.add("max_in_first")
            elif at[0] == len(hs) - 1:
                pats.add("max_in_last")
            else:
                pats.add("max_in_middle")
            for r, k, _ in hs:
                for name, idx in (("shared_idx0", 0), ("shared_idx63", 63), ("shared_idx64", 64),
                                  ("shared_last", lens[r] - 1)):
                    if k == idx:
                        pats.add(name)
        for p in pats:
            c[p] += 1
        if T == 0:
            c["all_empty"] += 1
        elif R >= 2:
            c["empty_first"] += lens[0] == 0
            c["empty_last"] += lens[-1] == 0
            c["empty_middle"] += R >= 3 and any(n == 0 for n in lens[1:-1])
        c["union64"] += len(holders) == 64
        c["union65"] += len(holders) == 65
        c["astride_2_31"] += bool(holders) and min(holders) < 2**31 <= max(holders)
    return c


# ----------------------------------------------------------------- CSR form
def csr(runs):
    """Packed numpy CSR (off u64, len u32, act u32, ctr u64) of one replica's runs."""
    import numpy as np

    ln = np.array([len(r) for r in runs], np.uint32)
    off = (np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
    act = np.array([a for r in runs for a, _ in r], np.uint32)
    ctr = np.array([c for r in runs for _, c in r], np.uint64)
    return off, ln, act, ctr


def replicas(objs):
    """The batch by replica: R lists of runs."""
    return [[o[r] for o in objs] for r in range(len(objs[0]))]
