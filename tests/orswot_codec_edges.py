"""Test helper: structured inputs for the Orswot state codec
(rust-crdt_amd/csrc/bincode.hip; crdt_orswot_from_bincode /
crdt_orswot_to_bincode), its contract and its walk restated in plain Python.

The generators behind tests/test_gpu_bincode.py draw counters below 2^40
(generate_orswot / generate_replicas) or below 20 (extreme_state), keys below
2^40, dense batches of 16 actors and member counts that sit on none of the
codec's launch tiers. Here every comparison the codec makes is put on an edge:
counters from orswot_pairgen.EDGE in top clocks, dots and deferred clocks;
deferred clocks in pairs that differ in one counter (orswot_pairgen.PAIRS), in
the last counter only, by a strict prefix, or in one actor across 2^31; member
keys and deferred-set elements from KEYS with partners that differ only in the
high word, the low word or the top bit; and every count the launch rule
branches on sits on both sides of its boundary (tier batches).

accepts() restates the header's contract (include/crdts_hip.h, "Ingest /
egest") on top of bincode_ref.decode / canonical. ingest_ref() / egest_ref()
restate the kernels' walk — rank by compare, scan, scatter; fields OR-ed into
a window of dwords — with every comparison point a knob; MUTANTS names wrong
settings of them: what the batches must tell apart. tier() recomputes, from
the launch rule, the path every object of a call takes; census() counts them.
Nothing here calls into the library."""
import bisect
import collections
import functools
import random
import struct

import bincode_ref as BC
import orswot_pairgen as pg
import records

FLOOR = 20  # orswot_edge_cases.FLOOR: the fewest objects of a batch that must show each property
M32, M64 = pg.M32, pg.M64
ENONCANON, ECAPACITY = -2, -4
WIDTHS = ((1, 1), (1, 8), (2, 2), (4, 4), (8, 1), (8, 8))
A_WIDE = 2**32 - 1  # the sparse batches' actor universe: actors on both sides of 2^31

# the kernels' limits (bincode.hip)
STAGE = 4096          # kBcStage: the LDS window of one wave
XS_MEM, XS_DEF = 256, 64        # the LDS scratch: members, deferred clocks
XB_MEM, XB_DEF = 16384, 1024    # the large-object kernel's HBM scratch
WAVE = 64
BLOCK_OBJS = 256      # objects per block the decode grid is sized by (bc_resident_blocks)
SPLIT_DYN, SPLIT_SF = 20, 5     # GuidedSplit<20, 5> (sched.h)


def signed(x):
    return x - 2**64 if x >= 2**63 else x


def signed32(x):
    x &= M32
    return x - 2**32 if x >= 2**31 else x


# ------------------------------------------------------------------ states and expected bytes
# A state is bincode_ref's: dict(clock={a: c}, entries={m: [(a, c)]}, deferred=[([(a, c)], [m])]).
def state(clock, entries, deferred=()):
    return dict(clock=dict(clock), entries={m: sorted(d.items() if isinstance(d, dict) else d)
                                            for m, d in entries.items()},
                deferred=sorted((sorted(c), sorted(ms)) for c, ms in deferred))


def rec_of(st, A, sparse=False):
    """The canonical record of a state (tests/records.py)."""
    return records.encode(st["clock"], {m: dict(d) for m, d in st["entries"].items()},
                          {tuple(c): set(ms) for c, ms in st["deferred"]}, A, sparse)


def pad16(b):
    return bytes(b) + bytes(-len(b) % 16)


def blob_len(st, wa, wm):
    sa = wa + 8
    return (24 + len(st["clock"]) * sa + sum(wm + 8 + len(d) * sa for d in st["entries"].values())
            + sum(16 + len(c) * sa + len(ms) * wm for c, ms in st["deferred"]))


# ------------------------------------------------------------------ the contract
def _structure(blob, wa, wm, A, ln):
    """The walk over a blob's length words in blob order, as every walk of
    bincode.hip makes it (bc_walk, lane_walk, bc_lane_walk_window): -> (code,
    None) at the first word it refuses, or (0, (n_clk, [(key pos, dots)],
    [(clock pos, dots, set pos, elements)])). `ln` reads a length word."""
    n, sa = len(blob), wa + 8
    if n < 24 or n >= 2**31:
        return ENONCANON, None
    nclk = ln(0)
    if nclk > A or nclk * sa > n - 24:
        return ENONCANON, None
    p = 8 + nclk * sa
    nent = ln(p)
    p += 8
    if nent > XB_MEM:
        return ECAPACITY, None
    mem = []
    for _ in range(nent):
        if p + wm + 8 > n:
            return ENONCANON, None
        l = ln(p + wm)
        if l == 0 or l > A or l * sa > n - (p + wm + 8):
            return ENONCANON, None
        mem.append((p, l))
        p += wm + 8 + l * sa
    if p + 8 > n:
        return ENONCANON, None
    ndef = ln(p)
    p += 8
    if ndef > XB_DEF:
        return ECAPACITY, None
    dfs = []
    for _ in range(ndef):
        if p + 8 > n:
            return ENONCANON, None
        lc = ln(p)
        if lc == 0 or lc > A or lc * sa > n - (p + 8):
            return ENONCANON, None
        q = p + 8 + lc * sa
        if q + 8 > n:
            return ENONCANON, None
        ls = ln(q)
        if ls == 0 or ls > n or ls * wm > n - (q + 8):
            return ENONCANON, None
        dfs.append((p, lc, q, ls))
        p = q + 8 + ls * wm
    if p != n:
        return ENONCANON, None
    return 0, (nclk, mem, dfs)


def accepts(blob, wa, wm, A, sparse=False):
    """The contract of crdt_orswot_from_bincode for one blob -> 0,
    CRDT_ENONCANON or CRDT_ECAPACITY. The header names both codes and no
    precedence; the one taken here (and written into the header with this
    suite): the length words are read front to back before any content is
    looked at, and the first one that cannot be taken decides — a count of
    members above 16 384 or of deferred clocks above 1 024 is CRDT_ECAPACITY
    where it is read, whatever the clocks before it hold or the bytes after it
    lack; every other refusal is CRDT_ENONCANON."""
    blob = bytes(blob)
    code, _ = _structure(blob, wa, wm, A, lambda p: int.from_bytes(blob[p:p + 8], "little"))
    if code:
        return code
    try:
        st = BC.decode(blob, wa, wm)
    except BC.FormatError:
        return ENONCANON
    acts = list(st["clock"]) + [a for d in st["entries"].values() for a, _ in d] + \
        [a for c, _ in st["deferred"] for a, _ in c]
    return 0 if BC.canonical(st) and all(a < A for a in acts) else ENONCANON


def size_by_counts(blob, wa, wm, A, sparse=False):
    """What crdt_orswot_bincode_record_sizes answers: 0 for a blob whose
    length words are refused, else the record bytes of the counts they give —
    also for a blob that is bad only in what its fields hold (a zero counter,
    an actor >= n_actors or out of order, duplicates), which only
    crdt_orswot_from_bincode looks at."""
    blob = bytes(blob)
    code, S = _structure(blob, wa, wm, A, lambda p: int.from_bytes(blob[p:p + 8], "little"))
    if code:
        return 0
    nclk, mem, dfs = S
    return records.record_bytes(nclk if sparse else A, len(mem), sum(l for _, l in mem), len(dfs),
                                sum(d[1] for d in dfs), sum(d[3] for d in dfs), sparse)


# ------------------------------------------------------------------ the walk, restated
def _pack(top, mems, defs, A, sparse):
    """A record from sections in the order given (records.encode sorts; this
    does not): top = [(a, c)], mems = [(key, [(a, c)])], defs = [([(a, c)], [m])]."""
    n_mem, n_dot = len(mems), sum(len(d) for _, d in mems)
    n_def, n_fd, n_fm = len(defs), sum(len(c) for c, _ in defs), sum(len(ms) for _, ms in defs)
    n_clk = len(top) if sparse else A
    size = records.record_bytes(n_clk, n_mem, n_dot, n_def, n_fd, n_fm, sparse)
    out = bytearray(size)
    struct.pack_into("<8I", out, 0, size, n_clk, n_mem, n_dot, n_def, n_fd, n_fm, 1 if sparse else 0)
    o = 32
    if sparse:
        struct.pack_into(f"<{n_clk}Q", out, o, *[c for _, c in top])
        struct.pack_into(f"<{n_clk}I", out, o + 8 * n_clk, *[a & M32 for a, _ in top])
        o += (12 * n_clk + 7) // 8 * 8
    else:
        for a, c in top:
            struct.pack_into("<Q", out, o + 8 * a, c)
        o += 8 * A
    dots = [x for _, d in mems for x in d]
    struct.pack_into(f"<{n_mem}Q", out, o, *[k for k, _ in mems])
    o += 8 * n_mem
    struct.pack_into(f"<{n_dot}Q", out, o, *[c for _, c in dots])
    o += 8 * n_dot
    struct.pack_into(f"<{n_dot}I", out, o, *[a & M32 for a, _ in dots])
    o += 4 * n_dot
    e, ends = 0, []
    for _, d in mems:
        e += len(d)
        ends.append(e)
    struct.pack_into(f"<{n_mem}I", out, o, *ends)
    o = (o + 4 * n_mem + 7) // 8 * 8
    fd = [x for c, _ in defs for x in c]
    struct.pack_into(f"<{n_fd}Q", out, o, *[c for _, c in fd])
    o += 8 * n_fd
    struct.pack_into(f"<{n_fm}Q", out, o, *[m for _, ms in defs for m in ms])
    o += 8 * n_fm
    struct.pack_into(f"<{n_fd}I", out, o, *[a & M32 for a, _ in fd])
    o += 4 * n_fd
    de, me, dd, mm = [], [], 0, 0
    for c, ms in defs:
        dd += len(c)
        mm += len(ms)
        de.append(dd)
        me.append(mm)
    struct.pack_into(f"<{n_def}I", out, o, *de)
    struct.pack_into(f"<{n_def}I", out, o + 4 * n_def, *me)
    return bytes(out)


def _ranks(keys, order, equal, small):
    """Rank by compare as bc_write_record does: rank = the number of keys
    below under `order`; duplicates by the rank sum (`small`: all keys in one
    register) or by counting the keys equal under `equal` -> (ranks, bad)."""
    ks = sorted(order(k) for k in keys)
    ranks = [bisect.bisect_left(ks, order(k)) for k in keys]
    n = len(keys)
    if small:
        return ranks, sum(ranks) != n * (n - 1) // 2
    return ranks, max(collections.Counter(equal(k) for k in keys).values(), default=1) != 1


def _scatter(ranks, items):
    out = [None] * len(items)
    for r, x in zip(ranks, items):
        out[r] = x
    return out


def ingest_ref(blob, wa, wm, A, sparse=False, **K):
    """bc_walk + bc_write_record on one blob -> the record, CRDT_ENONCANON /
    CRDT_ECAPACITY, or ("unplaced", ...) where a wrong compare leaves a slot
    of the record unwritten. K: the knobs of MUTANTS."""
    blob = bytes(blob)
    sa = wa + 8

    def u(p, w):
        return int.from_bytes(blob[p:p + w], "little")

    def ln(p):
        return u(p, 8) & M32 if K.get("length_low32") else u(p, 8)

    code, S = _structure(blob, wa, wm, A, ln)
    if code:
        return code
    nclk, mem, dfs = S
    bad = False

    def clock(p, l, top=False):
        nonlocal bad
        out, prev = [], 0
        for i in range(l):
            x, c = u(p + i * sa, wa), u(p + i * sa + wa, 8)
            if K.get("actor_narrowed_to_u32"):
                x &= M32
            # the top clock is read 64 entries a round; lane 0's predecessor is the round's carry
            pv = 0 if top and K.get("top_clock_no_carry") and i % WAVE == 0 else prev
            if x >= A or (c == 0 and not K.get("zero_counter_accepted")) or (i and pv >= x):
                bad = True
            prev = x
            out.append((x, c))
        return out

    top = [(x, c) for x, c in clock(8, nclk, True) if x < A]
    if not sparse:
        top = sorted(dict(top).items())  # the dense scatter: slot x holds the last counter written to it
    # members: ranked by key
    korder = signed if K.get("member_order_signed") else (lambda k: k & M32) if K.get("member_order_low32") \
        else (lambda k: k)
    kequal = (lambda k: k & M32) if K.get("member_equal_on_low32") else (lambda k: k)
    keys = [u(p, wm) for p, _ in mem]
    ranks, dup = _ranks(keys, korder, kequal, len(keys) <= WAVE)
    bad = bad or dup
    mems = _scatter(ranks, [(k, clock(p + wm + 8, l)) for k, (p, l) in zip(keys, mem)])
    # deferred clocks: ranked in CLOCK ORDER ((actor, counter) lexicographic, a proper prefix first)
    aorder = signed32 if K.get("clock_order_actor_signed") else (lambda a: a)
    corder = signed if K.get("clock_order_counter_signed") else (lambda c: c & M32) \
        if K.get("clock_order_counter_low32") else (lambda c: c >> 32) if K.get("clock_order_counter_high32") \
        else (lambda c: c)

    def ckey(pairs):
        t = tuple((aorder(a), corder(c)) for a, c in pairs)
        if K.get("clock_order_longer_first"):  # a proper prefix after what it is a prefix of
            return tuple((0,) + p for p in t) + ((1,),)
        return t

    clocks = [[(u(p + 8 + i * sa, wa), u(p + 8 + i * sa + wa, 8)) for i in range(lc)] for p, lc, _, _ in dfs]
    dranks, dup = _ranks(clocks, ckey, ckey, False)
    bad = bad or dup
    sorder = signed if K.get("set_order_signed") else (lambda m: m)
    sequal = (lambda m: m & M32) if K.get("set_equal_on_low32") else (lambda m: m)
    dd = []
    for (p, lc, q, ls) in dfs:
        c = clock(p + 8, lc)
        ms = [u(q + 8 + j * wm, wm) for j in range(ls)]
        r, dup = _ranks(ms, sorder, sequal, False)
        bad = bad or dup
        dd.append((c, _scatter(r, ms)))
    defs = _scatter(dranks, dd)
    if bad:
        return ENONCANON
    if None in mems or None in defs or any(None in ms for _, ms in defs):
        return ("unplaced", tuple(ranks), tuple(dranks))
    return _pack(top, mems, defs, A, sparse)


class _Window:
    """Dst<true> of bincode.hip: a zeroed window of dwords; a field is OR-ed
    in as the aligned 32-bit pieces it covers."""

    def __init__(self, nbytes, spill=False):
        self.w, self.spill = [0] * (nbytes // 4 + 4), spill

    def put(self, pos, v, w):
        q, sh = pos >> 2, 8 * (pos & 3)
        W = self.w
        if w == 8:
            lo, hi = v & M32, v >> 32
            W[q] |= (lo << sh) & M32
            W[q + 1] |= (((hi << sh) | (lo >> (32 - sh))) & M32) if sh else hi
            if sh:
                W[q + 2] |= hi >> (32 - sh)
            elif self.spill:  # the third piece without its `if (sh)`: a shift by 32 leaves hi as it is
                W[q + 2] |= hi
        else:
            m = v & ((1 << (8 * w)) - 1)
            W[q] |= (m << sh) & M32
            if sh + 8 * w > 32:
                W[q + 1] |= m >> (32 - sh)

    def bytes(self, n):
        return struct.pack(f"<{len(self.w)}I", *self.w)[:n]


def egest_ref(rec, wa, wm, A, **K):
    """bc_emit on one record -> the blob zero-padded to 16 bytes, or
    CRDT_ENONCANON for a value wider than its field."""
    d = records.decode(rec)
    sparse = bool(d["flags"] & 1)
    sa = wa + 8
    amax, mmax = (1 << (8 * wa)) - 1, (1 << (8 * wm)) - 1
    if sparse or not K.get("egest_emits_zero_slots"):
        top = sorted(d["clock"].items())
    else:
        top = list(enumerate(struct.unpack_from(f"<{A}Q", rec, 32)))
    mems, defs = list(d["entries"].items()), d["deferred"]
    acts = [a for a, _ in top] + [a for _, dots in mems for a, _ in dots] + [a for c, _ in defs for a, _ in c]
    keys = [m for m, _ in mems] + [m for _, ms in defs for m in ms]
    if A - 1 > amax:
        return ENONCANON
    if not K.get("egest_width_check_skipped") and (any(a > amax for a in acts) or any(m > mmax for m in keys)):
        return ENONCANON
    n = 24 + len(top) * sa + sum(wm + 8 + len(dots) * sa for _, dots in mems) + \
        sum(16 + len(c) * sa + len(ms) * wm for c, ms in defs)
    padded = (n + 15) // 16 * 16
    T = _Window(padded, K.get("egest_or_spills_neighbour"))

    def clock(p, pairs):
        T.put(p, len(pairs), 8)
        for i, (a, c) in enumerate(pairs):
            T.put(p + 8 + i * sa, a, wa)
            T.put(p + 8 + i * sa + wa, c, 8)
        return p + 8 + len(pairs) * sa

    p = clock(0, top)
    T.put(p, len(mems), 8)
    p += 8
    for m, dots in mems:
        T.put(p, m, wm)
        p = clock(p + wm, dots)
    T.put(p, len(defs), 8)
    p += 8
    for c, ms in defs:
        p = clock(p, c)
        T.put(p, len(ms), 8)
        for j, m in enumerate(ms):
            T.put(p + 8 + j * wm, m, wm)
        p += 8 + len(ms) * wm
    assert p == n
    return T.bytes(padded)


# knob -> (what it is, the batches meant for it: objects it must change there)
MUTANTS = {
    "member_order_signed": dict(member_order_signed=True),
    "member_order_low32": dict(member_order_low32=True),
    "member_equal_on_low32": dict(member_equal_on_low32=True),
    "clock_order_counter_signed": dict(clock_order_counter_signed=True),
    "clock_order_counter_low32": dict(clock_order_counter_low32=True),
    "clock_order_counter_high32": dict(clock_order_counter_high32=True),
    "clock_order_actor_signed": dict(clock_order_actor_signed=True),
    "clock_order_longer_first": dict(clock_order_longer_first=True),
    "set_order_signed": dict(set_order_signed=True),
    "set_equal_on_low32": dict(set_equal_on_low32=True),
    "actor_narrowed_to_u32": dict(actor_narrowed_to_u32=True),
    "length_low32": dict(length_low32=True),
    "top_clock_no_carry": dict(top_clock_no_carry=True),
    "zero_counter_accepted": dict(zero_counter_accepted=True),
    "egest_emits_zero_slots": dict(egest_emits_zero_slots=True),
    "egest_width_check_skipped": dict(egest_width_check_skipped=True),
    "egest_or_spills_neighbour": dict(egest_or_spills_neighbour=True),
}
INGEST_MUTANTS = tuple(k for k in MUTANTS if not k.startswith("egest"))
EGEST_MUTANTS = tuple(k for k in MUTANTS if k.startswith("egest"))
COMPARE_MUTANTS = INGEST_MUTANTS[:10]


# ------------------------------------------------------------------ value batches
def _keys(rng, n, wm):
    """n distinct member keys of wm bytes: KEYS that fit, and draws with
    partners that differ only in the high half, only in the low half, or only
    in the top bit of the width (wm = 8: the high word, the low word, bit 63)."""
    bits = 8 * wm
    lim, half = 1 << bits, bits // 2
    ks = {k for k in pg.KEYS if k < lim and rng.random() < 0.5} | {lim - 1}
    n = min(n, lim)
    while len(ks) < n:
        r = rng.getrandbits(bits)
        ks.add(r)
        u = rng.random()
        if u < 0.3:
            ks.add(r ^ (1 << rng.randrange(half, bits)))
        elif u < 0.55:
            ks.add(r ^ (1 << rng.randrange(half)))
        elif u < 0.75:
            ks.add(r ^ (1 << (bits - 1)))
    ks = sorted(ks)
    rng.shuffle(ks)
    return ks[:n]


def _edge(rng):
    return rng.choice(pg.EDGE)


def _dots(rng, acts, k):
    return [(a, _edge(rng)) for a in sorted(rng.sample(acts, min(len(acts), rng.randint(1, k))))]


_CPAIRS = tuple(p for p in pg.PAIRS if p[0])


def _clock_pairs(rng, acts, wide):
    """Two deferred clocks that differ in one place only."""
    base = _dots(rng, acts, 4)
    i = rng.randrange(len(base))
    lo, hi = rng.choice(_CPAIRS)
    u = rng.random()
    if u < 0.35:  # one counter, anywhere
        x, y = list(base), list(base)
        x[i], y[i] = (base[i][0], lo), (base[i][0], hi)
    elif u < 0.55:  # the last counter only
        x, y = list(base), list(base)
        x[-1], y[-1] = (base[-1][0], lo), (base[-1][0], hi)
    elif u < 0.75 or not wide:  # a strict prefix: not a duplicate, and first in CLOCK ORDER
        x, y = list(base), list(base) + [(max(acts) + 1, _edge(rng))]
    else:  # one actor only, across 2^31
        a, b = rng.choice(((2**31 - 1, 2**31), (2**31 - 2, 2**31 + 1), (1, 2**31), (2**31 - 1, 2**32 - 2)))
        c, tail = _edge(rng), [(2**32 - 2 + 0, _edge(rng))] if rng.random() < 0.5 and b < 2**32 - 2 else []
        head = [(0, _edge(rng))] if a > 0 and rng.random() < 0.5 else []
        x, y = head + [(a, c)] + tail, head + [(b, c)] + tail
    return (x, y) if rng.random() < 0.5 else (y, x)


def _value_state(rng, A, wa, wm, wide):
    amax = min(A, 1 << (8 * wa)) - 2  # (one actor id kept free for the prefix pairs)
    if wide:
        pool = [0, 1, 2**31 - 2, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 3] + [rng.randrange(2**32 - 3) for _ in range(3)]
        acts = sorted(set(rng.sample(pool, rng.randint(1, 6))))
    else:
        acts = sorted(rng.sample(range(amax + 1), rng.randint(1, min(amax + 1, 8))))
    clock = {a: _edge(rng) for a in acts if rng.random() < 0.85}
    keys = _keys(rng, rng.choice((0, 1, 3, 8, 14)), wm)
    entries = {m: _dots(rng, acts, 3) for m in keys}
    deferred = {}
    for _ in range(rng.choice((0, 1, 1, 2, 3))):
        for c in _clock_pairs(rng, [a for a in acts if a <= max(acts)], wide):
            deferred[tuple(c)] = _keys(rng, rng.choice((1, 2, 5, 9)), wm)
    return state(clock, entries, [(list(c), ms) for c, ms in deferred.items()])


def _or_window_state(k):
    """(wa, wm) = (1, 1): counters of 2^64 - 1 and 0x8000000000000001 next to
    counters of 1, rotated through the 9-byte entries' four alignments, with
    the largest key, for the OR-assembled egest window."""
    big = (M64, 0x8000000000000001, 2**63, M64 - 1)
    ctr = lambda i: big[(i + k) % 4] if (i + k // 4) % 2 else 1  # noqa: E731
    n = 2 + k % 7
    clock = {a: ctr(a) for a in range(n)}
    entries = {255 - j: [(a, ctr(a + j)) for a in range(j % 2, n)] for j in range(1 + k % 4)}
    deferred = [([(a, ctr(a + 1)) for a in range(0, n, 2)], [255, k % 200]), ([(n - 1, ctr(k))], [254 - k % 100])]
    return state(clock, entries, deferred)


N_VALUE = 160


@functools.lru_cache(maxsize=None)
def value_batch(wa, wm, wide=False):
    """-> (A, sparse, states): dense with 16 actors, or (wide) sparse with
    2^32 - 1 actors on both sides of 2^31 (wa 4 and 8)."""
    rng = random.Random(f"orswot-codec-value-{wa}-{wm}-{wide}")
    A = A_WIDE if wide else 16
    sts = [state({}, {}), state({0: 1}, {}), state({A - 1 if wide else min(A, 1 << (8 * wa)) - 1: M64},
                                                    {(1 << (8 * wm)) - 1: [(0, M64)], 0: [(0, 1)]})]
    if (wa, wm) == (1, 1) and not wide:
        sts += [_or_window_state(k) for k in range(48)]
    sts += [_value_state(rng, A, wa, wm, wide) for _ in range(N_VALUE)]
    return A, wide, sts


VALUE_SHAPES = tuple((wa, wm, False) for wa, wm in WIDTHS) + ((4, 4, True), (8, 8, True), (8, 1, True))


# ------------------------------------------------------------------ tier batches
def _members_state(rng, n, wm, A=16, n_def=0):
    acts = sorted(rng.sample(range(A), min(A, 3)))
    keys = _keys(rng, n, wm)
    assert len(keys) == n
    ent = {m: [(rng.choice(acts), _edge(rng))] for m in keys}
    return state({a: _edge(rng) for a in acts}, ent, _def_clocks(rng, n_def, A, wm))


def _def_clocks(rng, n, A, wm, set_size=None):
    out = {}
    while len(out) < n:
        acts = sorted(rng.sample(range(A), rng.randint(1, min(A, 3))))
        c = tuple((a, max(1, min(M64, _edge(rng) + rng.choice((0, 0, -1, 1, 7))))) for a in acts)
        out.setdefault(c, _keys(rng, set_size or rng.choice((1, 1, 2, 4)), wm))
    return [(list(c), ms) for c, ms in out.items()]


MEMBER_TIERS = (0, 1, 63, 64, 65, 128, 129, 255, 256, 257)
MEMBER_TIERS_11 = (0, 1, 63, 64, 65, 128, 129, 222, 223, 225)  # 222: the most that leaves len + 32 <= 4096
MEMBER_TIERS_BIG = (16383, 16384)   # twice each; 16385: rejected (malformed_big)
DEFERRED_TIERS = (0, 1, 63, 64, 65)
DEFERRED_TIERS_BIG = (1023, 1024)
CLOCK_A = (15, 16, 17, 64, 65, 256, 257, 1024)
CLOCK_N = (0, 1, 63, 64, 65, 128, 129)
LEN_TIERS = (4063, 4064, 4065)
EGEST_SIZES = (4080, 4096, 4112)


def _sized11(rng, target):
    """A (1, 1) state of one-dot members whose blob is exactly `target` bytes:
    24 + 18 m, the rest made up by one deferred clock of one dot (25 + s)."""
    m = (target - 24 - 26) // 18
    s = target - 24 - 18 * m - 25
    assert 1 <= s <= 256 and m <= 256
    keys = _keys(rng, m, 1)
    st = state({}, {k: [(rng.randrange(16), _edge(rng))] for k in keys},
               [([(rng.randrange(16), _edge(rng))], _keys(rng, s, 1))])
    assert blob_len(st, 1, 1) == target, (blob_len(st, 1, 1), target)
    return st


@functools.lru_cache(maxsize=None)
def _egest_shape(wa, wm, rsz, padded):
    sa = wa + 8
    for d in range(1, 7):
        for m in range(0, 257 if wm == 1 else 200):
            for s in range(d, 128 * d + 1):
                r = records.record_bytes(16, m, m, d, d, s)
                b = (24 + 6 * sa + m * (wm + 8 + sa) + d * (16 + sa) + s * wm + 15) // 16 * 16  # (6: the top clock below)
                if (rsz is None or r == rsz) and (padded is None or b == padded):
                    return m, d, s
    return None


def _egest_sized(rng, wa, wm, rsz, padded):
    """A dense A = 16 state of m one-dot members and d one-dot deferred clocks
    with s set elements between them (at most 128 a set: the set ranking is one
    lane's loop) whose record is rsz bytes and / or whose padded blob is
    `padded` bytes (None: whatever comes), or None when no (m, d, s) gives it."""
    mds = _egest_shape(wa, wm, rsz, padded)
    if mds is None:
        return None
    m, d, s = mds
    clocks = set()
    while len(clocks) < d:
        clocks.add((rng.randrange(16), _edge(rng)))
    sets = [s // d + (i < s % d) for i in range(d)]
    return state({a: _edge(rng) for a in range(0, 16, 3)}, {k: [(rng.randrange(16), _edge(rng))] for k in _keys(rng, m, wm)},
                 [([c], _keys(rng, n, wm)) for c, n in zip(sorted(clocks), sets)])


@functools.lru_cache(maxsize=None)
def tier_batch(name):
    """-> (wa, wm, A, sparse, states, labels, placement): placement None
    (junk-separated, every off & 15) or explicit (offsets, buffer length)."""
    rng = random.Random("orswot-codec-tier-" + name)
    sts, labs, place = [], [], None
    wa, wm, A, sparse = 1, 8, 16, False
    if name == "members":  # u64 keys through the register | loop ranking and the LDS | listed scratch
        for n in MEMBER_TIERS:
            sts += [_members_state(rng, n, 8, n_def=rng.choice((0, 0, 2))) for _ in range(FLOOR)]
            labs += ["mem%d" % n] * FLOOR
        order = list(range(len(sts)))
        rng.shuffle(order)
        sts, labs = [sts[i] for i in order], [labs[i] for i in order]
    elif name == "members11":  # (1, 1): what one window holds
        wm = 1
        for n in MEMBER_TIERS_11:
            sts += [_members_state(rng, n, 1) for _ in range(FLOOR)]
            labs += ["mem%d" % n] * FLOOR
    elif name == "members_big":
        for n in MEMBER_TIERS_BIG:
            sts += [_members_state(rng, n, 8, n_def=2) for _ in range(2)]
            labs += ["mem%d" % n] * 2
        sts.insert(1, _members_state(rng, 3, 8))
        labs.insert(1, "mem3")
    elif name == "deferred":
        wa, wm = 2, 2
        for n in DEFERRED_TIERS:
            sts += [_members_state(rng, rng.choice((0, 2, 5)), 2, n_def=n) for _ in range(FLOOR)]
            labs += ["def%d" % n] * FLOOR
        order = list(range(len(sts)))
        rng.shuffle(order)
        sts, labs = [sts[i] for i in order], [labs[i] for i in order]
    elif name == "set2000":  # one lane ranks a deferred set: two objects, in different chunks of the call
        wa, wm = 2, 2
        sts = [_members_state(rng, rng.choice((0, 2, 5)), 2, n_def=rng.choice((0, 1, 2))) for _ in range(70)]
        labs = ["small"] * 70
        for at in (3, 60):
            sts[at] = state({1: 2**63}, {7: [(1, 2**63)]}, _def_clocks(rng, 1, 16, 2, set_size=2000))
            labs[at] = "set2000"
    elif name == "deferred_big":
        wa, wm = 2, 2
        for n in DEFERRED_TIERS_BIG:
            sts += [_members_state(rng, 4, 2, n_def=n) for _ in range(2)]
            labs += ["def%d" % n] * 2
        sts.insert(2, _members_state(rng, 3, 2))
        labs.insert(2, "def0")
    elif name.startswith("clock") or name.startswith("sparse"):
        wa, wm = 2, 8
        sparse = name.startswith("sparse")
        A = int(name[5:]) if not sparse else 1024
        for n in [n for n in CLOCK_N if n <= A] + ([A] if not sparse else [2, 1023]):
            for _ in range(10):
                acts = sorted(rng.sample(range(A), n))  # zeros between the nonzero slots
                mem = {m: [(a, _edge(rng)) for a in sorted(rng.sample(acts, min(n, 2)))] or [(0, 1)]
                       for m in _keys(rng, rng.choice((0, 1, 3)), 8)}
                sts.append(state({a: _edge(rng) for a in acts}, mem))
                labs.append("clk%d" % n)
        order = list(range(len(sts)))
        rng.shuffle(order)
        sts, labs = [sts[i] for i in order], [labs[i] for i in order]
        if A == 256 and not sparse:
            # a full clock and 256 members (the dense scatter shares its bytes with the ranking's arrays),
            # followed in the same wave by a small object
            full = _members_state(rng, 256, 8, A=256)
            full["clock"] = {a: _edge(rng) for a in range(256)}
            sts[:0] = [full, state({255: 1, 0: M64}, {5: [(255, 1)]})]
            labs[:0] = ["full256", "after_full"]
    elif name == "length":  # len + 32 on both sides of the window; groups ending on both sides of its edge
        wm = 1
        for t in LEN_TIERS:
            sts += [_sized11(rng, t) for _ in range(FLOOR)]
            labs += ["len%d" % t] * FLOOR
    elif name == "groups":
        wm = 1
        buf, offs = 0, []

        def tiny(k):
            return state({k % 16: _edge(rng)}, {m: [(k % 16, _edge(rng))] for m in _keys(rng, 2 + k % 3, 1)})

        # pairs in one window: the second blob ends at ga + reach - 16, reach = 4095, 4096 (fits), 4097 (does not)
        for reach in (4095, 4096, 4097) * (FLOOR + 4):
            a, b = tiny(len(sts)), tiny(len(sts) + 1)
            ga = (buf + 15) // 16 * 16 + 16
            o0 = ga + rng.randrange(16)
            o1 = ga + reach - 16 - blob_len(b, 1, 1)
            offs += [o0, o1]
            sts += [a, b]
            labs += ["first", "reach%d" % reach]
            buf = o1 + blob_len(b, 1, 1) + rng.randrange(8) + (4200 if reach == 4097 else 0)  # (b left alone)
        # 120 blobs back to back: ~30 to a window
        for k in range(120):
            sts.append(tiny(k))
            labs.append("row")
            offs.append(buf)
            buf += blob_len(sts[-1], 1, 1)
        # a group whose members are not consecutive lanes: a big blob's lane between two small ones
        for k in range(FLOOR + 8):
            a, big, b = tiny(k), _members_state(rng, 250, 1), tiny(k + 1)
            offs += [buf, buf + 256 + 8192, buf + 128]
            sts += [a, big, b]
            labs += ["split_a", "split_big", "split_b"]
            buf += 256 + 8192 + blob_len(big, 1, 1) + 3
        place = (tuple(offs), buf + 5)
    elif name.startswith("egest"):
        wa, wm = {"egest11": (1, 1), "egest18": (1, 8), "egest88": (8, 8)}[name]
        for r in EGEST_SIZES + (None,):
            for p in EGEST_SIZES + (None,):
                if r is None and p is None:
                    continue
                for _ in range(7):
                    st = _egest_sized(rng, wa, wm, r, p)
                    if st is not None:
                        sts.append(st)
                        labs.append("r%s_p%s" % (r, p))
    else:
        raise ValueError(name)
    return wa, wm, A, sparse, sts, labs, place


TIER_SHAPES = ("members", "members11", "members_big", "deferred", "set2000", "deferred_big", "length", "groups",
               "egest11", "egest18", "egest88", "sparse") + tuple("clock%d" % a for a in CLOCK_A)


# ------------------------------------------------------------------ placement
def place(blobs, rng=None, offsets=None):
    """-> (buffer, offsets, lengths): blobs at explicit offsets (the rest of
    the buffer junk), or one after another with junk between them so that
    blob i starts at off & 15 == i % 16."""
    rng = rng or random.Random(len(blobs))
    if offsets is not None:
        offs, total = offsets
        buf = bytearray(random.Random(total).randbytes(total))
        for o, b in zip(offs, blobs):
            buf[o:o + len(b)] = b
        return bytes(buf), list(offs), [len(b) for b in blobs]
    buf, offs = bytearray(), []
    for i, b in enumerate(blobs):
        buf += bytes([0xA5]) * ((i % 16 - len(buf)) % 16 + 16 * (i % 3 == 2))
        offs.append(len(buf))
        buf += b
    buf += b"\xa5" * 3
    return bytes(buf), offs, [len(b) for b in blobs]


# ------------------------------------------------------------------ the launch rule
def chunks(n):
    """The object ranges GuidedSplit<20, 5> (sched.h) hands to the decode
    waves of an n-object call whose grid is ceil(n / 256) blocks of 4 waves."""
    n_waves = 4 * ((n + BLOCK_OBJS - 1) // BLOCK_OBJS)
    s_total = n * SPLIT_SF // 8
    out = []
    if s_total:
        rounds = (s_total + n_waves * WAVE - 1) // (n_waves * WAVE)
        cs = (s_total + n_waves * rounds - 1) // (n_waves * rounds)
        out += [(b, min(b + cs, s_total)) for b in range(0, s_total, cs)]
    out += [(b, min(b + SPLIT_DYN, n)) for b in range(s_total, n, SPLIT_DYN)]
    return out


def peek(blob, wa, wm, A):
    """What the group walk's first pass reads of a blob: the entry count it
    reserves in the group's 256 entry slots (0 when the header is refused)."""
    n = len(blob)
    if n < 24:
        return 0
    nclk = int.from_bytes(blob[:8], "little")
    if nclk > A or nclk * (wa + 8) > n - 24:
        return 0
    ne = int.from_bytes(blob[8 + nclk * (wa + 8):16 + nclk * (wa + 8)], "little")
    return ne if ne <= XS_MEM else 0


def tier(n_obj, offs, lens, shapes, blob_bytes=None):
    """The ingest path of every object of one crdt_orswot_from_bincode call ->
    [dict(path, scratch, rank, group, reach, missed)]. shapes[i] = (the entry
    count peek() reads, n_mem, n_def) with n_mem = None for a refused blob.
    path: "group" (walked lane-parallel with the blobs that share its 4 KB
    window), "hbm" (len + 32 > 4096: walked from HBM), "fallback" (a group
    whose claimed entry counts pass 256: its blobs one by one from HBM), "out"
    (not inside the buffer); scratch: "lds" | "listed" (the large-object
    kernel); rank: "reg" (<= 64 members, ranked in registers) | "loop"."""
    assert n_obj <= 2048, "the grid rule below holds for uncapped grids only"
    out = [None] * n_obj
    gid = 0
    for cb, ce in chunks(n_obj):
        lanes = range(cb, ce)
        inb = {i for i in lanes if blob_bytes is None or (offs[i] <= blob_bytes and lens[i] <= blob_bytes - offs[i])}
        rem = sorted(i for i in inb if lens[i] + 32 <= STAGE)
        for i in lanes:
            out[i] = dict(path="hbm" if i in inb else "out", group=None, reach=None, missed=[], gsize=0)
        while rem:
            ga = offs[rem[0]] & ~15
            g = [i for i in rem if offs[i] >= ga and offs[i] + lens[i] + 16 <= ga + STAGE]
            for i in rem:
                if i not in g and offs[i] >= ga:
                    out[i]["missed"].append(offs[i] + lens[i] + 16 - ga)
            fits = sum(shapes[i][0] for i in g) <= XS_MEM
            for i in g:
                out[i].update(path="group" if fits else "fallback", group=gid, gsize=len(g),
                              reach=offs[i] + lens[i] + 16 - ga)
            gid += 1
            rem = [i for i in rem if i not in g]
    for i, o in enumerate(out):
        _, n_mem, n_def = shapes[i]
        if n_mem is None or o["path"] == "out":
            o.update(scratch=None, rank=None)
        else:
            o.update(scratch="listed" if n_mem > XS_MEM or n_def > XS_DEF else "lds",
                     rank="reg" if n_mem <= WAVE else "loop")
    return out


def egest_tier(rsz, blen):
    """The write path of one record of crdt_orswot_to_bincode: the record
    staged in the LDS window or read from HBM; the blob assembled in the
    second window or written to HBM byte by byte."""
    padded = (blen + 15) // 16 * 16
    return "hbm_hbm" if rsz > STAGE else "win_lds" if padded <= STAGE else "win_hbm"


def census(tiers, sts, lens, recs, wa, wm):
    """Counts of everything a tier batch is there for."""
    c = collections.Counter()
    for t, st, n, r in zip(tiers, sts, lens, recs):
        c["%s/%s/%s" % (t["path"], t["scratch"], t["rank"])] += 1
        c["mem%d" % len(st["entries"])] += 1
        c["def%d" % len(st["deferred"])] += 1
        c["clk%d" % len(st["clock"])] += 1
        c["clk_odd" if len(st["clock"]) & 1 else "clk_even"] += 1
        c["len+32%s4096" % ("<=" if n + 32 <= STAGE else ">")] += 1
        if n in LEN_TIERS:
            c["len%d" % n] += 1
        if t["reach"] in (4095, 4096) and t["gsize"] > 1:
            c["reach%d" % t["reach"]] += 1
        c["missed4097"] += 4097 in t["missed"]
        c["egest/" + egest_tier(len(r), n)] += 1
        if len(r) in EGEST_SIZES:
            c["rsz%d" % len(r)] += 1
        if (n + 15) // 16 * 16 in EGEST_SIZES:
            c["padded%d" % ((n + 15) // 16 * 16)] += 1
        c["set>=2000"] += any(len(ms) >= 2000 for _, ms in st["deferred"])
    groups = collections.Counter(t["group"] for t in tiers if t["group"] is not None)
    c["largest_group"] = max(groups.values(), default=0)
    c["groups>=25"] = sum(v >= 25 for v in groups.values())
    by = collections.defaultdict(list)
    for i, t in enumerate(tiers):
        if t["group"] is not None and t["path"] == "group":
            by[t["group"]].append(i)
    c["split_groups"] = sum(1 for g in by.values() if len(g) > 1 and g[-1] - g[0] + 1 != len(g))
    return +c


@functools.lru_cache(maxsize=None)
def case(kind, *key):
    """One batch ready for both tests -> dict(wa, wm, A, sparse, states,
    labels, blobs (shuffled HashMap / HashSet orders), buf / offs / lens (the
    upload), recs (expected records), canon (expected egest blobs, padded),
    tiers, census)."""
    if kind == "value":
        wa, wm, wide = key
        A, sparse, sts = value_batch(wa, wm, wide)
        labs, plc = ["value"] * len(sts), None
    else:
        wa, wm, A, sparse, sts, labs, plc = tier_batch(key[0])
    rng = random.Random("orswot-codec-case-%s-%s" % (kind, key))
    blobs = [BC.encode(s, wa, wm, rng=rng) for s in sts]
    buf, offs, lens = place(blobs, rng, plc)
    recs = [rec_of(s, A, sparse) for s in sts]
    canon = [pad16(BC.encode(s, wa, wm)) for s in sts]
    shapes = [(peek(b, wa, wm, A), len(s["entries"]), len(s["deferred"])) for b, s in zip(blobs, sts)]
    tiers = tier(len(sts), offs, lens, shapes, len(buf))
    return dict(wa=wa, wm=wm, A=A, sparse=sparse, states=sts, labels=labs, blobs=blobs, buf=buf, offs=offs, lens=lens,
                recs=recs, canon=canon, tiers=tiers, census=census(tiers, sts, lens, recs, wa, wm))


# the census every tier batch must show (both test files assert it): key -> the fewest objects
CENSUS = {
    "members": dict({"mem%d" % n: FLOOR for n in MEMBER_TIERS}, **{
        "group/lds/reg": 3 * FLOOR, "group/lds/loop": 2 * FLOOR, "hbm/lds/loop": 2 * FLOOR, "hbm/listed/loop": FLOOR}),
    "members11": dict({"mem%d" % n: FLOOR for n in MEMBER_TIERS_11}, **{
        "group/lds/reg": 4 * FLOOR, "group/lds/loop": 4 * FLOOR, "hbm/lds/loop": 2 * FLOOR}),
    "members_big": {"mem16383": 2, "mem16384": 2, "hbm/listed/loop": 4, "group/lds/reg": 1},
    "deferred": dict({"def%d" % n: FLOOR for n in DEFERRED_TIERS}, **{"group/listed/reg": FLOOR}),
    "set2000": {"set>=2000": 2, "hbm/lds/reg": 2},
    "deferred_big": {"def1023": 2, "def1024": 2, "hbm/listed/reg": 4},
    "length": dict({"len%d" % n: FLOOR for n in LEN_TIERS}, **{"len+32<=4096": 2 * FLOOR, "len+32>4096": FLOOR,
                                                                "group/lds/loop": 2 * FLOOR, "hbm/lds/loop": FLOOR}),
    "groups": {"reach4095": FLOOR, "reach4096": FLOOR, "missed4097": FLOOR, "groups>=25": 1, "largest_group": 28,
               "split_groups": FLOOR},
    "egest11": {"rsz4080": 7, "rsz4096": 7, "rsz4112": 7, "padded4080": 7, "padded4096": 7, "padded4112": 7,
                "egest/win_lds": 14, "egest/hbm_hbm": 14},
    # (a few objects cover the three write paths: each size in at least two of the (record, blob) combinations the
    # widths allow, 7 objects a combination)
    **{n: dict({"%s%d" % (k, v): 14 for k in ("rsz", "padded") for v in EGEST_SIZES},
               **{"egest/win_lds": 14, "egest/win_hbm": 14, "egest/hbm_hbm": 14}) for n in ("egest18", "egest88")},
    "sparse": dict({"clk%d" % n: 10 for n in CLOCK_N + (2, 1023)}, clk_odd=40, clk_even=40),
    **{"clock%d" % a: {"clk%d" % n: 10 for n in CLOCK_N + (a,) if n <= a} for a in CLOCK_A},
}


def assert_census(name):
    c = case("tier", name)["census"]
    want = CENSUS[name]
    assert all(c.get(k, 0) >= v for k, v in want.items()), (name, {k: (c.get(k, 0), v) for k, v in want.items()
                                                                   if c.get(k, 0) < v})
    return c


# ------------------------------------------------------------------ malformed input
def layout(st, wa, wm):
    """Byte positions of every field of BC.encode(st, wa, wm) (ascending
    orders): dict(nclk, clk=[(actor pos, counter pos)], nent, mem=[(key pos,
    count pos, [(actor pos, counter pos)])], ndef, defs=[(count pos, [(a, c)],
    set count pos, [element pos])], end)."""
    sa = wa + 8
    L = dict(nclk=0, clk=[(8 + i * sa, 8 + i * sa + wa) for i in range(len(st["clock"]))])
    p = 8 + len(st["clock"]) * sa
    L["nent"], L["mem"] = p, []
    p += 8
    for m in sorted(st["entries"]):
        d = st["entries"][m]
        L["mem"].append((p, p + wm, [(p + wm + 8 + i * sa, p + wm + 8 + i * sa + wa) for i in range(len(d))]))
        p += wm + 8 + len(d) * sa
    L["ndef"], L["defs"] = p, []
    p += 8
    for c, ms in sorted((sorted(c), sorted(ms)) for c, ms in st["deferred"]):
        q = p + 8 + len(c) * sa
        L["defs"].append((p, [(p + 8 + i * sa, p + 8 + i * sa + wa) for i in range(len(c))], q,
                          [q + 8 + j * wm for j in range(len(ms))]))
        p = q + 8 + len(ms) * wm
    L["end"] = p
    return L


def _patch(blob, pos, v, w):
    return blob[:pos] + int(v).to_bytes(w, "little") + blob[pos + w:]


MATRIX_W = (8, 8)  # the matrix' widths: 8-byte actors hold 1 + 2^32, 8-byte members more than 256 keys
VARIANTS = {"group": 3, "hbm": 200, "listed": 300}  # the bad blob's member count -> its path


def _matrix_base(n_mem, n_clk=3):
    clock = {a: 2**32 + a for a in range(1, n_clk + 1)}
    ent = {2**40 + 3 * m: [(1, 2**32 - m - 1), (2, 2**63 + m)] for m in range(n_mem)}
    return state(clock, ent, [([(1, 2**63), (3, 1)], [5, 2**63 + 6]), ([(2, M64)], [8])])


@functools.lru_cache(maxsize=None)
def matrix(variant):
    """-> [(name, A, good blob, bad blob, placed past the buffer?)]: every
    damage of the malformed matrix applied to a base blob of the variant's
    member count ("group": in a window with its neighbours, "hbm": past the
    window, "listed": the large-object kernel), widths MATRIX_W."""
    wa, wm = MATRIX_W
    n = VARIANTS[variant]
    st = _matrix_base(n)
    g = BC.encode(st, wa, wm)
    L = layout(st, wa, wm)
    good = BC.encode(_matrix_base(2), wa, wm)
    out = []

    def add(name, bad, A=16, past=False):
        out.append((name, A, good, bytes(bad), past))

    hi = 2**32 + 1
    for name, pos in (("clock", L["nclk"]), ("entries", L["nent"]), ("member_dots", L["mem"][1][1]),
                      ("deferred", L["ndef"]), ("deferred_clock", L["defs"][0][0]), ("deferred_set", L["defs"][0][2])):
        add("length_high_word:" + name, _patch(g, pos, hi, 8))
    add("len_23", bytes(23))
    add("len_24_zero_is_default", bytes(24))
    add("past_the_buffer", g, past=True)
    for name, pos in (("clock", L["clk"][1][1]), ("entries", L["mem"][1][2][0][1]), ("deferred", L["defs"][1][1][0][1])):
        add("one_byte_short_in:" + name, g[:pos] + g[pos + 1:])
    add("cut_by_one", g[:-1])
    add("trailing_byte", g + b"\0")
    for name, pos in (("clock", L["clk"][2][1]), ("member", L["mem"][n // 2][2][1][1]),
                      ("deferred", L["defs"][0][1][1][1])):
        add("zero_counter:" + name, _patch(g, pos, 0, 8))
    add("actor_eq_A", _patch(g, L["mem"][n - 1][2][1][0], 16, wa))
    add("actor_1_plus_2^32", _patch(g, L["mem"][0][2][0][0], 1 + 2**32, wa))
    add("equal_adjacent_actors", _patch(g, L["clk"][1][0], 1, wa))
    # actors out of order exactly between top-clock entries 63 and 64 (the second round's lane 0)
    st70 = _matrix_base(n, 70)
    L70, g70 = layout(st70, wa, wm), BC.encode(st70, wa, wm)
    add("actors_out_of_order_63|64", _patch(_patch(g70, L70["clk"][63][0], 65, wa), L70["clk"][64][0], 64, wa), A=128)
    add("duplicate_member", _patch(g, L["mem"][n - 1][0], 2**40 + 3 * (n // 2), wm))
    one = BC.encode(dict(clock={}, entries={}, deferred=[([(2, M64)], [8])]), wa, wm)[24:]  # (one deferred entry)
    add("duplicate_deferred_clock", g[:L["ndef"]] + (2).to_bytes(8, "little") + one + _patch(one, len(one) - wm, 9, wm))
    add("duplicate_set_element", _patch(g, L["defs"][0][3][1], 5, wm))
    empty_member = dict(st, entries={**st["entries"], 7: []})
    add("empty_member_clock", BC.encode(empty_member, wa, wm))
    add("empty_deferred_clock", BC.encode(dict(st, deferred=st["deferred"] + [([], [9])]), wa, wm))
    add("empty_deferred_set", BC.encode(dict(st, deferred=st["deferred"] + [([(3, 7)], [])]), wa, wm))
    if variant == "group":
        # claimed entry counts that overflow the group's 256 entry slots: 200 + 200 (and the good neighbours')
        add("claims_200_entries", (0).to_bytes(8, "little") + (200).to_bytes(8, "little") + bytes(40))
    return out


def matrix_upload(good, bad, past, twin=False):
    """good | bad | good (twin: good | bad | bad | good, for the group-slot
    overflow) -> (buffer, offsets, lengths)."""
    blobs = [good] + [bad] * (2 if twin else 1) + [good]
    buf, offs, lens = place(blobs, random.Random(len(bad)))
    if past:
        offs[1] = len(buf) - len(bad) + 1
    return buf, offs, lens


@functools.lru_cache(maxsize=None)
def reject_batch(kind):
    """-> (wa, wm, A, [(blob, code under the contract)]): at least FLOOR blobs
    that only one check refuses, each between valid ones, for the knobs that
    drop a check. "actor": an 8-byte actor whose low word alone is a valid,
    ordered actor; "length": a length word of 2^32 + n whose low word alone is
    the blob's true length; "carry": top-clock actors out of order exactly
    across a 64-entry round; "zero": one zero counter."""
    rng = random.Random("orswot-codec-reject-" + kind)
    wa, wm, A = (8, 8, 16) if kind != "carry" else (2, 8, 200)
    out = []
    for k in range(FLOOR + 4):
        st = _value_state(rng, A, wa, wm, False) if kind != "carry" else None
        while kind != "carry" and not (st["clock"] and st["entries"] and st["deferred"]):
            st = _value_state(rng, A, wa, wm, False)
        if kind == "carry":
            n = rng.choice((65, 70, 129, 140, 200))
            acts = sorted(rng.sample(range(A), n))
            st = state({a: _edge(rng) for a in acts}, {m: [(acts[0], 1)] for m in _keys(rng, k % 3, 8)})
        g, L = BC.encode(st, wa, wm), layout(st, wa, wm)
        out.append((g, 0))
        if kind == "actor":
            spots = [a for a, _ in L["clk"]] + [a for _, _, d in L["mem"] for a, _ in d] + \
                [a for _, c, _, _ in L["defs"] for a, _ in c]
            pos = spots[k % len(spots)]
            bad = _patch(g, pos, int.from_bytes(g[pos:pos + 8], "little") + (1 + k % 3) * 2**32, 8)
        elif kind == "length":
            spots = [L["nclk"], L["nent"], L["ndef"]] + [c for _, c, _ in L["mem"]] + \
                [x for c, _, s, _ in L["defs"] for x in (c, s)]
            pos = spots[(k * 7) % len(spots)] if k >= 6 else ([L["nclk"], L["nent"], L["mem"][0][1], L["ndef"],
                                                              L["defs"][0][0], L["defs"][0][2]][k])
            bad = _patch(g, pos, int.from_bytes(g[pos:pos + 8], "little") + 2**32, 8)
        elif kind == "carry":
            r = 64 if n < 129 or k % 2 else 128
            a, b = L["clk"][r - 1][0], L["clk"][r][0]
            bad = _patch(_patch(g, a, int.from_bytes(g[b:b + wa], "little"), wa), b, int.from_bytes(g[a:a + wa], "little"), wa)
        else:
            spots = [c for _, c in L["clk"]] + [c for _, _, d in L["mem"] for _, c in d] + \
                [c for _, cl, _, _ in L["defs"] for _, c in cl]
            pos = ([L["clk"][0][1], L["mem"][0][2][0][1], L["defs"][0][1][0][1]] + spots)[k % (3 + len(spots))]
            bad = _patch(g, pos, 0, 8)
        out.append((bad, accepts(bad, wa, wm, A)))
    out.append((out[0][0], 0))
    return wa, wm, A, out


REJECT_KINDS = {"actor": "actor_narrowed_to_u32", "length": "length_low32", "carry": "top_clock_no_carry",
                "zero": "zero_counter_accepted"}
