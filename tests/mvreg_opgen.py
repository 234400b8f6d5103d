"""Test helper: MVReg<u64, A> op lists (Op::Put, src/mvreg.rs:51-59) — a seeded
generator, the rendering of oracle/crdts_ref.py::MVReg to the zero-filled slab
of crdt_mvreg_merge / crdt_mvreg_apply, and the runner of the KAT
scripts (tests/golden/kat_mvreg_ops.json) over a backend.

A register is a crdts_ref.MVReg; an op is (clock_pairs, val) with clock_pairs
= [(actor, counter), ...] in actor order; actors are dense ids below A."""
import json
import os
import random

import numpy as np

import crdts_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_mvreg_ops.json")
CLASSES = ("add", "add_drop", "skip", "skip_drop", "empty")


# ------------------------------------------------------------------ slabs
def slab(regs, cap, A):
    """MVRegs -> (n u32[n], clk u64[n][cap][A], val u64[n][cap]), unused slots zero."""
    n = len(regs)
    cnt = np.zeros(n, np.uint32)
    clk = np.zeros((n, cap, A), np.uint64)
    val = np.zeros((n, cap), np.uint64)
    for i, r in enumerate(regs):
        assert len(r.vals) <= cap, (i, len(r.vals), cap)
        cnt[i] = len(r.vals)
        for k, (c, v) in enumerate(r.vals):
            for a, x in c.dots.items():
                clk[i, k, a] = x
            val[i, k] = v
    return cnt, clk, val


def regs_of(cnt, clk, val):
    """The slab's registers, rows taken as given (an all-zero row is an empty clock)."""
    out = []
    for i in range(len(cnt)):
        r = crdts_ref.MVReg()
        for k in range(int(cnt[i])):
            nz = np.nonzero(clk[i, k])[0]
            r.vals.append((crdts_ref.VClock([(int(a), int(clk[i, k, a])) for a in nz]), int(val[i, k])))
        out.append(r)
    return out


def setlike(cnt, clk, val):
    """Per object the sorted (row, val) list: the reference's PartialEq (src/mvreg.rs:74-96)."""
    return [sorted((tuple(int(x) for x in clk[i, k]), int(val[i, k])) for k in range(int(cnt[i])))
            for i in range(len(cnt))]


def pairs_of(clock):
    return sorted(clock.dots.items())


def fold(reg):
    """read().add_clock (src/mvreg.rs:201-222)."""
    c = crdts_ref.VClock()
    for vc, _ in reg.vals:
        c.merge(vc)
    return c


def classify(reg, clock):
    """The outcome class of Put{clock} on reg (src/mvreg.rs:158-186)."""
    if clock.is_empty():
        return "empty"
    drop = any(c <= clock for c, _ in reg.vals)
    add = not any(c > clock for c, _ in reg.vals if not (c <= clock))
    return ("add" if add else "skip") + ("_drop" if drop else "")


# -------------------------------------------------------------- generator
def random_reg(rng, A, cap, hi, val0=0):
    """0..cap slots of random rows with counters below hi (rows as given: an
    all-zero row may occur)."""
    r = crdts_ref.MVReg()
    for k in range(rng.randint(0, cap)):
        r.vals.append((crdts_ref.VClock([(a, c) for a in range(A) for c in [rng.randrange(hi)] if c]), val0 + k))
    return r


def random_clock(rng, A, hi):
    c = crdts_ref.VClock([(a, rng.randint(1, hi)) for a in range(A) if rng.random() < 0.5])
    if c.is_empty():
        c = crdts_ref.VClock([(rng.randrange(A), rng.randint(1, hi))])
    return c


def gen_op(rng, reg, A, hi):
    """5 % empty, 30 % read-derived (fold + inc), 15 % replay of a stored clock,
    10 % one step below a stored clock, the rest random sparse clocks up to hi."""
    u = rng.random()
    if u < 0.05:
        return crdts_ref.VClock()
    if u < 0.35:
        c = fold(reg)
        c.apply(c.inc(rng.randrange(A)))
        return c
    stored = [c for c, _ in reg.vals if not c.is_empty()]
    if u < 0.50 and stored:
        return rng.choice(stored).clone()
    if u < 0.60 and stored:
        c = rng.choice(stored).clone()
        a = rng.choice(sorted(c.dots))
        if c.dots[a] > 1:
            c.dots[a] -= 1
        elif len(c.dots) > 1:
            del c.dots[a]
        return c
    return random_clock(rng, A, hi)


def gen_batch(seed, n, A, cap, hi, min_ops=0, max_ops=8):
    """-> dict(regs0, ops, regs, classes, peak): the initial registers, the op
    lists [(pairs, val), ...], the registers after them (by the restatement),
    the outcome-class counts and the largest slot count any object reached."""
    rng = random.Random(seed)
    regs0, ops, regs, classes, peak = [], [], [], dict.fromkeys(CLASSES, 0), 0
    for i in range(n):
        r0 = random_reg(rng, A, cap, hi, val0=1000 * i)
        r = r0.clone()
        lst = []
        for t in range(rng.randint(min_ops, max_ops)):
            c = gen_op(rng, r, A, hi)
            classes[classify(r, c)] += 1
            v = 1000 * i + 500 + t
            r.apply_put(c, v)
            peak = max(peak, len(r.vals))
            lst.append((pairs_of(c), v))
        regs0.append(r0)
        ops.append(lst)
        regs.append(r)
    return dict(regs0=regs0, ops=ops, regs=regs, classes=classes, peak=peak)


def apply_ref(regs, ops):
    out = []
    for r, lst in zip(regs, ops):
        r = r.clone()
        for pairs, v in lst:
            r.apply_put(crdts_ref.VClock(pairs), v)
        out.append(r)
    return out


# ------------------------------------------------------------ KAT scripts
def load_kats():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


class PyBackend:
    """Registers are crdts_ref.MVRegs."""

    def new(self):
        return crdts_ref.MVReg()

    def apply(self, reg, op):
        reg.apply_put(crdts_ref.VClock(op[0]), op[1])

    def merge(self, reg, other):
        reg.merge(other)

    def read(self, reg):
        """(vals in order, add_clock pairs)."""
        return reg.read(), pairs_of(fold(reg))

    def setlike(self, reg):
        return sorted((pairs_of(c), v) for c, v in reg.vals)


def run_kat(case, be):
    """Runs one script; the reference's asserts are the script's assert steps.
    Steps: ["new", r] | ["set", op, r, actor, val] (reg.set(val,
    reg.read().derive_add_ctx(actor)): the register is not changed) |
    ["put", op, pairs, val] | ["apply", r, op] | ["merge", r1, r2] (r1.merge(&r2))
    | ["assert_read", r, vals, pairs] | ["assert_read_any", r, [vals, ...]] (the
    values read are one of the lists) | ["assert_eq", r1, r2] | ["assert_new", r].
    Returns the applies made."""
    regs, ops, applies = {}, {}, 0
    for st in case["steps"]:
        k = st[0]
        if k == "new":
            regs[st[1]] = be.new()
        elif k == "set":
            _, (clock) = be.read(regs[st[2]])
            c = crdts_ref.VClock([tuple(p) for p in clock])
            c.apply(c.inc(st[3]))  # derive_add_ctx, src/ctx.rs:45-53
            ops[st[1]] = (pairs_of(c), st[4])
        elif k == "put":
            ops[st[1]] = ([tuple(p) for p in st[2]], st[3])
        elif k == "apply":
            be.apply(regs[st[1]], ops[st[2]])
            applies += 1
        elif k == "merge":
            be.merge(regs[st[1]], regs[st[2]])
        elif k == "assert_read_any":
            vals, _ = be.read(regs[st[1]])
            assert list(vals) in st[2], (case["name"], st, vals)
        elif k == "assert_read":
            vals, clock = be.read(regs[st[1]])
            assert list(vals) == st[2], (case["name"], st, vals)
            assert [list(p) for p in clock] == st[3], (case["name"], st, clock)
        elif k == "assert_eq":
            assert be.setlike(regs[st[1]]) == be.setlike(regs[st[2]]), (case["name"], st)
        elif k == "assert_new":
            assert be.setlike(regs[st[1]]) == [], (case["name"], st)
        else:
            raise ValueError(f"unknown step {st!r}")
    return applies
