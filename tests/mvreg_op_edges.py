"""Test helper: edge inputs for the MVReg<u64, A> op path — crdt_mvreg_apply
(Op::Put, src/mvreg.rs:158-186), crdt_mvreg_truncate (:100-113) and
crdt_mvreg_read_clock (:201-222), rust-crdt_amd/csrc/mvreg_apply.hip.

The op-simulated inputs of tests/mvreg_opgen.py keep every counter below 5. Here
a batch is a register pair of tests/mvreg_pairgen.py: its self side is the
stored register, the rows of its other side, in slot order, are the Put
clocks. Every row is a variant of a few base rows with counters on the u64
edges, so every Put meets stored clocks below it, equal to it, above it and
concurrent with it, one apart across 2^32 and 2^63. Named extra Puts, the
structure batches (dominating chains of up to 130 Puts, registers that fill
to out_cap with holes below) and poison in the unused input slots are added.

apply_ref / truncate_ref / read_clock_ref restate the three calls per object;
their knobs turn them into the deliberately wrong kernels of APPLY_MUTANTS,
TRUNCATE_MUTANTS and READ_MUTANTS that the batches must tell apart. tier() and
truncate_form() restate the launch rules; layout() walks the physical slots
the way the kernels do and counts compactions, header reloads and unstaged ops.
Every batch is made once (batch()) and is read-only."""
import functools
import random

import numpy as np

import mvreg_pairgen as pg
from mvreg_opgen import CLASSES

M64 = 2**64 - 1
POISON = np.uint64(0xFFFF_FFFF_DEAD_BEEF)  # the unused input slots: above every counter but 2^64 - 1, nonzero low word
XVAL0 = 2**63 + 2**40  # the values of the extra Puts
LDS_BYTES = 60 * 1024
EXTRAS = ("empty", "stored_row", "read_clock", "read_lower", "actor_first", "actor_last", "zero_row")
KW = 64


# ------------------------------------------------------------ launch rules
def per_wave_bytes(A, out_cap):
    """A wave's LDS in the fast kernel: the block, the op row, the values (8 bytes each), the slot table."""
    return (8 * (out_cap * A + A + out_cap) + out_cap + 15) & ~15


def tier(A, out_cap):
    """The kernel and waves per block crdt_mvreg_apply takes: "general", or "W4" / "W3" / "W2" / "W1"."""
    pw = per_wave_bytes(A, out_cap)
    if out_cap > 64 or pw > LDS_BYTES:
        return "general"
    W = 4
    while W > 1 and W * pw > LDS_BYTES:
        W -= 1
    return f"W{W}"


def truncate_form(ns, A):
    """The form crdt_mvreg_truncate takes for a register of ns used slots."""
    return "lane_element" if ns <= KW and A <= 65536 else "lane_slot"


def tier_edges_by_A(out_cap, A_max=4096):
    """[(A, tier(A), A + 1, tier(A + 1))] wherever the tier changes."""
    return [(A, tier(A, out_cap), A + 1, tier(A + 1, out_cap)) for A in range(1, A_max)
            if tier(A, out_cap) != tier(A + 1, out_cap)]


def tier_edges_by_cap(A, cap_max=80):
    return [(c, tier(A, c), c + 1, tier(A, c + 1)) for c in range(1, cap_max) if tier(A, c) != tier(A, c + 1)]


def fast_grid_waves(cus):
    """Waves of the fast kernel's largest grid: cus * (256 / W) blocks of W waves."""
    return cus * 256


# ------------------------------------------------------------- references
def _key(x, compare):
    """The counters as a wrong compare sees them."""
    if compare is None:
        return x
    if compare == "low32":
        return x & np.uint64(0xFFFFFFFF)
    if compare == "high32":
        return x >> np.uint64(32)
    if compare == "signed":
        return x.view(np.int64)
    raise ValueError(compare)


def apply_ref(rows, vals, puts, compare=None, drop_strict=False, skip_on_concurrent=False, unnamed_actor_blind=False,
              ignores_last_actor=False, empty_put_appends=False, append_before_drop=False, out_cap=None, trace=None):
    """MVReg::apply of the Puts [(dense clock row, val), ...] in order on the
    register (rows u64 [k][A] as given, vals) -> (rows, vals), or None when
    out_cap is given and a Put would leave more slots than that (the kernels
    latch CRDT_ECAPACITY). With no knob this is src/mvreg.rs:158-186: an empty
    clock changes nothing; else the values whose clock is <= the Put's go, and
    the Put is appended unless a remaining clock is strictly greater. `trace`
    receives (class, kept mask over the slots before the Put, appended?)."""
    R = np.array(rows, np.uint64)
    V = [int(v) for v in vals]
    for c, v in puts:
        c = np.asarray(c, np.uint64)
        if R.ndim != 2:
            R = R.reshape(0, len(c))
        if not c.any():
            if empty_put_appends:
                R = np.vstack([R, c[None]])
                V.append(int(v))
            if trace is not None:
                trace.append(("empty", np.ones(len(V) - bool(empty_put_appends), bool), bool(empty_put_appends)))
            continue
        Rk, ck = _key(R, compare), _key(c, compare)
        if ignores_last_actor:
            Rk, ck = Rk[:, :-1], ck[:-1]
        if unnamed_actor_blind:
            named = (c != 0)[:ck.shape[0]]
            Rk, ck = Rk[:, named], ck[named]
        gt, lt = (Rk > ck).any(axis=1), (Rk < ck).any(axis=1)
        keep = gt | ~lt if drop_strict else gt  # not <= the Put clock
        dom = keep if skip_on_concurrent else gt & ~lt
        add = not dom.any()
        if out_cap is not None and (len(V) if append_before_drop else int(keep.sum())) + add > out_cap:
            return None
        if trace is not None:
            trace.append((("add" if add else "skip") + ("" if keep.all() else "_drop"), keep, add))
        if not keep.all():
            R = R[keep]
            V = [x for x, k in zip(V, keep) if k]
        if add:
            R = np.vstack([R, c[None]])
            V.append(int(v))
    return R, V


def truncate_ref(rows, vals, T, compare=None, subtract_strict=False, keeps_emptied_value=False):
    """Causal::truncate (src/mvreg.rs:100-113): a counter <= the truncating
    clock's goes (VClock::subtract), a value whose clock empties is dropped."""
    R = np.array(rows, np.uint64)
    T = np.asarray(T, np.uint64)
    Rk, Tk = _key(R, compare), _key(T, compare)
    stay = (Rk >= Tk if subtract_strict else Rk > Tk) & (R != 0)
    R = np.where(stay, R, np.uint64(0))
    keep = np.ones(len(R), bool) if keeps_emptied_value else stay.any(axis=1)
    return R[keep], [int(v) for v, k in zip(vals, keep) if k]


def read_clock_ref(clk, ns, compare=None, max_per_half=False, ignores_last_used_slot=False,
                   reads_unused_slots=False):
    """read().add_clock (src/mvreg.rs:201-222) of a register given as its
    whole input block clk u64 [cap][A] with ns used slots: the pointwise max."""
    R = np.asarray(clk, np.uint64)
    R = R if reads_unused_slots else R[:max(0, ns - 1) if ignores_last_used_slot else ns]
    m = np.zeros(R.shape[1], np.uint64)
    if max_per_half:
        if len(R):
            m = ((R >> np.uint64(32)).max(axis=0) << np.uint64(32)) | (R & np.uint64(0xFFFFFFFF)).max(axis=0)
        return m
    for r in R:
        m = np.where(_key(r, compare) > _key(m, compare), r, m)
    return m


_CMP = {f"counter_compare_{k}": dict(compare=k) for k in ("low32", "high32", "signed")}
APPLY_MUTANTS = dict(_CMP, drop_strict=dict(drop_strict=True), skip_on_concurrent=dict(skip_on_concurrent=True),
                     unnamed_actor_blind=dict(unnamed_actor_blind=True),
                     ignores_last_actor=dict(ignores_last_actor=True), empty_put_appends=dict(empty_put_appends=True),
                     append_before_drop=dict(append_before_drop=True))
TRUNCATE_MUTANTS = dict(_CMP, subtract_strict=dict(subtract_strict=True),
                        keeps_emptied_value=dict(keeps_emptied_value=True))
READ_MUTANTS = dict(_CMP, max_per_half=dict(max_per_half=True),
                    ignores_last_used_slot=dict(ignores_last_used_slot=True),
                    reads_unused_slots=dict(reads_unused_slots=True))


def layout(ns, trace, out_cap, shrink):
    """The physical slots as the kernels keep them: a drop leaves a hole, the
    append goes past the highest slot in use (`shrink`, the fast kernel) or
    past the high-water mark (the general kernel), and the kept rows move down
    only when that runs into out_cap; the general kernel closes the holes once
    more at the end. -> (compactions mid-list, at the end, most slots in use)."""
    phys, hw, mid, peak = list(range(ns)), ns, 0, ns
    for _, keep, add in trace:
        phys = [p for p, k in zip(phys, keep) if k]
        if shrink:
            hw = phys[-1] + 1 if phys else 0
        if add:
            if hw == out_cap:
                mid += 1
                phys = list(range(len(phys)))
                hw = len(phys)
            phys.append(hw)
            hw += 1
        peak = max(peak, len(phys))
    return mid, int(not shrink and len(phys) != hw), peak


def staging(pairs_per_put):
    """Of one object's op list: (header reloads, staged Puts, Puts whose pairs
    are read from memory). The fast kernel loads 64 op headers and the first
    64 clock pairs after the chunk's start at a time; a non-empty Put is
    staged when its pairs end within those 64."""
    reloads, staged, unstaged = max(0, (len(pairs_per_put) - 1) // KW), 0, 0
    for t, np_ in enumerate(pairs_per_put):
        if np_:
            if sum(pairs_per_put[t - t % KW:t + 1]) <= KW:
                staged += 1
            else:
                unstaged += 1
    return reloads, staged, unstaged


# ---------------------------------------------------------------- batches
def _slab(objs, cap, A, poison=False):
    n = len(objs)
    cnt = np.array([len(v) for _, v in objs], np.uint32)
    clk = np.full((n, cap, A), POISON if poison else 0, np.uint64)
    val = np.full((n, cap), POISON if poison else 0, np.uint64)
    for i, (R, V) in enumerate(objs):
        assert len(V) <= cap, (i, len(V), cap)
        if len(V):
            clk[i, :len(V)] = R
            val[i, :len(V)] = np.array(V, np.uint64)
    return cnt, clk, val


def _extra_put(rng, kind, R, A, H):
    """The extra Put clock of `kind` against the register's rows R at that point of the list."""
    c = np.zeros(A, np.uint64)
    rc = R.max(axis=0) if len(R) else c
    if kind == "empty":
        return c
    if kind == "stored_row" and len(R):
        return R[rng.randrange(len(R))].copy()
    if kind in ("read_clock", "read_lower", "stored_row"):  # (no stored row: the read clock, which is empty too)
        c = rc.copy()
        if kind == "read_lower":
            nz = [int(x) for x in np.nonzero(c)[0]]
            hz = [x for x in nz if x in H]
            if nz:
                c[rng.choice(hz or nz)] -= np.uint64(1)
        return c
    x = 0 if kind == "actor_first" else A - 1
    top = int(rc[x])
    c[x] = rng.choice([top or 1, min(top + 1, M64), max(top - 1, 1), rng.choice(pg.EDGE), M64])
    return c


def _finish(name, A, scap, out_cap, objs, puts, extras, pcap):
    """Objects (rows, vals) and Put lists -> the batch dict, its answers and census."""
    n, t = len(objs), tier(A, out_cap)
    ends, classes = [], dict.fromkeys(CLASSES, 0)
    cen = dict(reloads=0, staged=0, unstaged=0, compact_mid=0, compact_end=0, compact_objs=0, peak=0, full_puts=0,
               longest=0, over_64_used=0)
    for (R, V), lst in zip(objs, puts):
        trace = []
        out = apply_ref(R, V, lst, out_cap=out_cap, trace=trace)
        assert out is not None
        ends.append(out)
        for cls, _, _ in trace:
            classes[cls] += 1
        mid, end, peak = layout(len(V), trace, out_cap, shrink=t != "general")
        r, s, u = staging([int(np.count_nonzero(c)) for c, _ in lst])
        cen["reloads"] += r
        cen["staged"] += s
        cen["unstaged"] += u
        cen["compact_mid"] += mid
        cen["compact_end"] += end
        cen["compact_objs"] += bool(mid)
        cen["peak"] = max(cen["peak"], peak)
        cen["full_puts"] += peak == out_cap
        cen["longest"] = max(cen["longest"], len(lst))
        cen["over_64_used"] += peak > KW
    S = _slab(objs, scap, A, poison=True)
    P = _slab([(np.array([c for c, _ in lst], np.uint64).reshape(-1, A), [v for _, v in lst]) for lst in puts], pcap, A)
    E = _slab(ends, out_cap, A)
    b = dict(name=name, A=A, scap=scap, out_cap=out_cap, n=n, tier=t, S=S, P=P, E=E, classes=classes, census=cen,
             extras={k: sum(k in e for e in extras) for k in EXTRAS})
    for x in (*S, *P, *E):
        x.flags.writeable = False
    return b


def pair_batch(name, A, scap, ogen, out_cap, n, extras=True, cut=()):
    """The register pairs of mvreg_pairgen.gen as registers and Put lists,
    two extras per object; a list that would pass out_cap loses Puts from its
    end (the extras last). `cut`: slot counts that the registers of objects
    5, 6, .. of every ten are cut down to (around truncate's 64-slot test)."""
    seed = 0xE000 + 131 * A + 17 * scap + 5 * ogen + out_cap
    (sn, sclk, sval), (on, oclk, oval) = pg.gen(seed, n, A, scap, ogen)
    rng, H = random.Random(seed + 1), pg.hot(A)
    objs, puts, marks = [], [], []
    for i in range(n):
        ns = int(sn[i])
        if cut and 5 <= i % 10 < 5 + len(cut):
            ns = min(ns, cut[i % 10 - 5])
        R, V = sclk[i, :ns].copy(), [int(v) for v in sval[i, :ns]]
        lst = [(oclk[i, k].copy(), int(oval[i, k]), None) for k in range(int(on[i]))]
        kinds = [EXTRAS[i % 7], EXTRAS[(i + 3) % 7]] if extras else []
        if "zero_row" in kinds and len(V):
            R[rng.randrange(len(V))] = 0
        at = sorted((len(lst) if k == "empty" and i % 21 >= 7 else rng.randint(0, len(lst)), k)
                    for k in kinds if k != "zero_row")
        for j, (pos, kind) in enumerate(at):
            pos += j
            state = apply_ref(R, V, [(c, v) for c, v, _ in lst[:pos]])
            lst.insert(pos, (_extra_put(rng, kind, state[0].reshape(-1, A), A, H), XVAL0 + 4 * i + j, kind))
        while apply_ref(R, V, [(c, v) for c, v, _ in lst], out_cap=out_cap) is None:
            plain = [k for k, p in enumerate(lst) if p[2] is None]
            lst.pop(plain[-1] if plain else -1)
        objs.append((R, V))
        puts.append([(c, v) for c, v, _ in lst])
        marks.append({p[2] for p in lst if p[2]} | ({"zero_row"} if "zero_row" in kinds and len(V) else set()))
    return _finish(name, A, scap, out_cap, objs, puts, marks, ogen + 2)


CHAIN_LENGTHS = (63, 64, 65, 130)
CHAIN_STARTS = (2**32 - 1, 2**63 - 1, 2**64 - 2, 40)


def chain_batch(name, A, n, out_cap=8, scap=4):
    """Lists in which each Put dominates the one before. Object i: a list of
    CHAIN_LENGTHS[i % 4] Puts of 1..6 clock pairs; the chain actor's counter
    climbs one at a time through 2^32, 2^63 or up to 2^64 - 1 at a random place
    of the list; replays, stale Puts, empty Puts and concurrent forks are mixed
    in. The stored register holds a row above the chain's first steps, a row
    below them and rows at other actors."""
    rng, H = random.Random(0xC4A1 + A), pg.hot(A)
    objs, puts = [], []
    for i in range(n):
        L = CHAIN_LENGTHS[i % 4]
        npairs = min(A, 1 + (i // 4) % 6)
        slots = rng.sample(H, min(len(H), npairs))
        slots += rng.sample([s for s in range(A) if s not in slots], npairs - len(slots))
        if i % 5 == 1:  # the chain actor is the last one
            slots = [A - 1] + [s for s in slots if s != A - 1][:npairs - 1]
        x, ys = slots[0], slots[1:]
        cross = CHAIN_STARTS[(i // 24) % 4]
        c0 = min(cross - rng.randrange(2, L), M64 - L // 2) if cross > 2 * L else cross
        cur = np.zeros(A, np.uint64)
        cur[x] = c0
        for y in ys:
            cur[y] = rng.choice(pg.EDGE)
        R, V = [], []
        if i % 3 == 0:  # a row above the first steps and a row below them
            hi_, lo_ = cur.copy(), cur.copy()
            hi_[x] += np.uint64(rng.randint(2, 6))
            lo_[x] -= np.uint64(1)
            R, V = [lo_, hi_], [pg.VAL0 + 8 * i, pg.VAL0 + 8 * i + 1]
        others = [s for s in range(A) if s not in slots]
        w, h = rng.choice(others or [0]), rng.choice([0, 1, 2**31 - 1, 2**31])
        for k in range(rng.randint(0, 2) if others else 0):  # rows at an actor no Put of the chain names;
            z = np.zeros(A, np.uint64)  # two of them: the larger has the smaller low word
            z[w] = ((h + 1) << 32 | 3) if k else (h << 32 | 0xFFFFFFF0)
            R.append(z)
            V.append(pg.VAL0 + 8 * i + 2 + k)
        lst = []
        for t in range(L):
            u = rng.random()
            c = cur.copy()
            if u < 0.05:
                c[:] = 0
            elif u < 0.15:
                pass  # a replay of the clock before
            elif u < 0.23:
                c[x] -= np.uint64(1)  # stale
            elif u < 0.30 and ys:  # a fork: the chain actor one lower, another one higher; the chain joins it
                y = rng.choice(ys)
                if int(cur[y]) < M64:
                    c[x] -= np.uint64(1)
                    c[y] += np.uint64(1)
                    cur[y] += np.uint64(1)
            elif int(cur[x]) < M64:
                cur[x] += np.uint64(1)
                c = cur.copy()
            if t == L - 1 and i % 5 == 2:
                c[:] = 0  # the list ends with an empty Put
            if t == L - 1 and i % 5 == 1:
                c = cur.copy()
                c[x] -= np.uint64(2)  # the list ends with a stale Put that differs at the last actor only
            lst.append((c, XVAL0 + 256 * i + t))
        objs.append((np.array(R, np.uint64).reshape(-1, A), V))
        puts.append(lst)
    return _finish(name, A, scap, out_cap, objs, puts, [set()] * n, max(CHAIN_LENGTHS))


def compact_batch(name, A, out_cap, n, nputs=7):
    """Registers that are full or one short of it, of mutually concurrent rows
    ({x: base + k, y: base + out_cap - k}, the counters astride 2^32 or 2^63).
    Two Puts in three are greater than two neighbouring rows and concurrent
    with the rest: they leave holes below and are appended at out_cap. The rest
    are empty, stale (below one row), or concurrent with every row (a third
    actor). Every sixth register holds a row below its neighbour, and its first
    Put lies between the two."""
    rng, H = random.Random(0xC0AC + A + out_cap), pg.hot(A)
    objs, puts = [], []
    for i in range(n):
        x, y = rng.sample(H, 2) if rng.random() < 0.7 else rng.sample(range(A), 2)
        z = rng.choice([s for s in range(A) if s not in (x, y)])
        base = max(1, rng.choice([2**32, 2**63, M64 - out_cap, 5]) - (out_cap // 2 if i % 2 else 0))
        ns = out_cap - (i % 3 == 2)
        R = np.zeros((ns, A), np.uint64)
        for k in range(ns):
            R[k, x], R[k, y] = base + k, base + out_cap - k
        V = [pg.VAL0 + 128 * i + k for k in range(ns)]
        lst = []
        for t in range(nputs):
            c = np.zeros(A, np.uint64)
            u = rng.random()
            j = rng.randrange(1, ns) if t or i % 4 else ns - 1  # (i % 4 == 0: the first Put drops the top row)
            if t == 0 and i % 6 == 2:
                R[0, y] -= np.uint64(3)  # row 0 < row 1
                c[x], c[y] = base, base + out_cap - 2  # row 0 <= the Put < row 1
            elif t == 1 and i % 4 == 3 or 0.35 <= u < 0.45:
                c[x], c[y] = base + j, base + out_cap - j  # row j again, if it is still there
            elif u < 0.10:
                pass
            elif u < 0.22:
                c[x], c[y] = base + j, base + out_cap - j - 1  # below row j, above none
            elif u < 0.35:
                c[z] = rng.choice(pg.EDGE)
            else:
                c[x], c[y] = base + j, base + out_cap - j + 1
            lst.append((c, XVAL0 + 16 * i + t))
        while apply_ref(R, V, lst, out_cap=out_cap) is None:
            lst.pop()
        if i % 4 == 1 and lst:
            lst[-1] = (np.zeros(A, np.uint64), lst[-1][1])  # the list ends with an empty Put
        objs.append((R, V))
        puts.append(lst)
    return _finish(name, A, out_cap, out_cap, objs, puts, [set()] * n, nputs)


def _n(A, out_cap):
    return 300 if out_cap * A <= 4000 else 120


def _specs():
    """name -> (maker, args). The tier shapes are found from tier() itself:
    both sides of every change of tier along A at out_cap 64 and along out_cap
    at A = 100."""
    s = {}
    for lo, _, hi, _ in tier_edges_by_A(64):
        for A in (lo, hi):
            s[f"A{A}-cap64"] = (pair_batch, (A, 24, 10, 64, _n(A, 64)))
    for lo, _, hi, _ in tier_edges_by_cap(100):
        for c in (lo, hi):
            s[f"A100-cap{c}"] = (pair_batch, (100, min(8, c - 6), 4 if c < 17 else 6, c, _n(100, c)))
    for A in (1, 5, 16, 33, 63, 64, 65):
        s[f"A{A}-cap16"] = (pair_batch, (A, 8, 6, 16, 300))
    s["A16-cap64"] = (pair_batch, (16, 24, 10, 64, 300))
    s["A16-cap65"] = (pair_batch, (16, 24, 10, 65, 300))
    s["A8-cap100"] = (pair_batch, (8, 80, 18, 100, 300, True, (63, 64, 65, 66)))
    s["A2048-cap3"] = (pair_batch, (2048, 2, 1, 3, 300))
    s["chain-A16"] = (chain_batch, (16, 160))
    s["chain-A100"] = (chain_batch, (100, 160))
    for A in (5, 64, 100):
        s[f"compact-A{A}-cap64"] = (compact_batch, (A, 64, 120))
    s["compact-A5-cap70"] = (compact_batch, (5, 70, 120))
    s["compact-A200-cap40"] = (compact_batch, (200, 40, 120))
    return s


SPECS = _specs()
NAMES = tuple(SPECS)
TILED = "A5-cap16"  # the batch tiled over the fast kernel's whole grid


@functools.lru_cache(maxsize=None)
def batch(name):
    maker, args = SPECS[name]
    return maker(name, *args)


def puts_of(b, i):
    pn, pclk, pval = b["P"]
    return [(pclk[i, k], int(pval[i, k])) for k in range(int(pn[i]))]


def reg_of(b, i):
    sn, sclk, sval = b["S"]
    return sclk[i, :sn[i]], [int(v) for v in sval[i, :sn[i]]]


def op_arrays(P):
    """The dense Put slab (pn, pclk [n][P][A], pval) -> the five arrays of crdt_mvreg_ops."""
    pn, pclk, pval = P
    used = np.arange(pclk.shape[1])[None, :] < pn[:, None]
    nz = (pclk != 0) & used[:, :, None]
    act = np.nonzero(nz)[2].astype(np.uint32)
    return (np.cumsum(pn, dtype=np.uint64), pval[used], np.cumsum(nz.sum(axis=2)[used], dtype=np.uint64), act,
            pclk[nz])


def tile(b, n):
    """The batch repeated to n objects -> (S, P, E); round r of the tiling adds
    r * 2^41 to every value in use."""
    idx, rnd = np.arange(n) % b["n"], (np.arange(n, dtype=np.uint64) // np.uint64(b["n"])) << np.uint64(41)

    def rep(slab):
        cnt, clk, val = slab
        used = np.arange(val.shape[1])[None, :] < cnt[idx][:, None]
        return cnt[idx], clk[idx], np.where(used, val[idx] + rnd[:, None], val[idx])

    return rep(b["S"]), rep(b["P"]), rep(b["E"])


# ------------------------------------------------- truncate and read clock
TRUNC_KINDS = ("read_clock", "stored_row", "row_hot_up", "row_hot_down", "zero")


@functools.lru_cache(maxsize=None)
def truncate_batch(name):
    """-> (T u64 [n][A], E at the batch's scap): the truncating clocks, built
    from each register's own rows, and the truncated registers."""
    b = batch(name)
    A, n = b["A"], b["n"]
    rng, H = random.Random(0x7E00 + A + b["scap"]), pg.hot(A)
    T, out = np.zeros((n, A), np.uint64), []
    for i in range(n):
        R, V = reg_of(b, i)
        kind = TRUNC_KINDS[i % 5]
        if len(R) and kind != "zero":
            t = R.max(axis=0) if kind == "read_clock" else R[rng.randrange(len(R))].copy()
            if kind.startswith("row_hot"):
                nz = [int(x) for x in np.nonzero(t)[0]]
                x = rng.choice([s for s in nz if s in H] or nz or H)
                t[x] = min(int(t[x]) + 1, M64) if kind == "row_hot_up" else max(int(t[x]) - 1, 0)
            T[i] = t
        out.append(truncate_ref(R, V, T[i]))
    E = _slab(out, b["scap"], A)
    for x in (T, *E):
        x.flags.writeable = False
    return T, E


@functools.lru_cache(maxsize=None)
def read_batch(name):
    b = batch(name)
    sn, sclk, _ = b["S"]
    E = np.array([read_clock_ref(sclk[i], int(sn[i])) for i in range(b["n"])], np.uint64).reshape(b["n"], b["A"])
    E.flags.writeable = False
    return E


# ------------------------------------------------------ what a mutant changes
def _same(a, b):
    if a is None or b is None or list(a[1]) != list(b[1]):
        return False
    return not len(a[1]) or np.array_equal(np.asarray(a[0]).reshape(len(a[1]), -1), np.asarray(b[0]))


def answer_of(E, i):
    en, eclk, eval_ = E
    return eclk[i, :en[i]], [int(v) for v in eval_[i, :en[i]]]


def apply_differs(b, **knobs):
    """Objects of the batch on which apply_ref with the knobs gives another register (or an error)."""
    return sum(not _same(apply_ref(*reg_of(b, i), puts_of(b, i), out_cap=b["out_cap"], **knobs), answer_of(b["E"], i))
               for i in range(b["n"]))


def truncate_differs(b, **knobs):
    T, E = truncate_batch(b["name"])
    return sum(not _same(truncate_ref(*reg_of(b, i), T[i], **knobs), answer_of(E, i)) for i in range(b["n"]))


def read_differs(b, **knobs):
    sn, sclk, _ = b["S"]
    E = read_batch(b["name"])
    return sum(not np.array_equal(read_clock_ref(sclk[i], int(sn[i]), **knobs), E[i]) for i in range(b["n"]))
