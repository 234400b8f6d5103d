"""Workload generators: the C ABI's host op-simulation generators
(crdt_orswot_generate*, crdt_dense_generate) as numpy arrays, the heavy-tail
batch assembly over them, and the sparse clock pairs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SPARSE_CLOCK, GenParams, RepParams, check, lib

# SURVEY.md §8(d) config 3 / BASELINE.json configs[2].
CONFIG3 = dict(n_actors=16, member_universe=64, ancestor_adds=32, min_div_ops=4, max_div_ops=16, pct_add=60,
               pct_future_rm=10, pct_deferred_obj=8, pct_shared_actor=5)
CONFIG3_SEED = 0xC0FFEE03
# SURVEY.md §8(d) config 5 / BASELINE.json configs[4]: 1024-actor universe, CSR top clocks, 8 replicas.
CONFIG5 = dict(universe=1024, pool_actors=48, own_actors=2, member_universe=64, ancestor_adds=48, min_div_ops=4,
               max_div_ops=16, pct_add=60, pct_future_rm=10, pct_deferred_obj=8)
CONFIG5_SEED = 0xC0FFEE05


def _params(p):
    if isinstance(p, GenParams):
        return p
    d = dict(CONFIG3)
    d.update(p or {})
    return GenParams(**{k: int(v) for k, v in d.items()})


def generate_orswot(n_obj, first_obj=0, seed=CONFIG3_SEED, params=None, threads=8):
    """Host op-simulation generator (see include/crdts_hip.h). Returns
    ((L_base, L_off), (R_base, R_off)) as numpy arrays (copies)."""
    P = _params(params)
    g = C.c_void_p()
    check(lib.crdt_orswot_generate(seed, first_obj, n_obj, C.byref(P), threads, C.byref(g)), "generate")
    try:
        sides = _copy_sides(g, 2, n_obj)
        return sides[0], sides[1]
    finally:
        lib.crdt_orswot_gen_free(g)


TAIL_SEED = 0xC0FFEE06
TAIL_SIZES = (100, 300, 1000)


def generate_orswot_tail(n_obj, frac=0.05, sizes=TAIL_SIZES, first_obj=0, seed=CONFIG3_SEED, threads=8):
    """Config 3 with a heavy tail (bench.py --workload orswot_tail): object i
    is heavy iff (first_obj + i) % round(1 / frac) == 0; heavy objects take
    the sizes in turn, an object of size m being op-simulated over a member
    universe of m keys with m ancestor adds and m/8..m/4 divergent ops per
    side (so ~m members per side: the reference's entries map is unbounded,
    src/orswot.rs:26-30); the others are config-3 objects. The same object
    index gets the same pair at any batch split. Returns ((L_base, L_off),
    (R_base, R_off)) as numpy arrays."""
    def base(n, first):
        return generate_orswot(n, first_obj=first, seed=seed, threads=threads)

    def heavy_gen(n, first, m, params):
        return generate_orswot(n, first_obj=first, seed=TAIL_SEED + m, threads=threads, params=params)

    return _tail_batch(n_obj, frac, sizes, first_obj, base, heavy_gen)


def generate_orswot_csr_tail(n_obj, frac=0.05, sizes=TAIL_SIZES, first_obj=0, seed=CONFIG5_SEED, threads=8):
    """Config 5's record form with a heavy tail (bench.py --workload
    orswot_csr_tail): replicas 0 and 1 of the config-5 replica generator (CSR
    top clocks over the 1 024-actor universe) as the self and other batches,
    object i heavy iff (first_obj + i) % round(1 / frac) == 0, heavy objects
    at the sizes in turn (member universe m, m ancestor adds, m/8..m/4
    divergent ops per replica: ~m members per side; the reference's entries
    map and clock are unbounded, src/orswot.rs:26-30, src/vclock.rs:54-57).
    Split-invariant like generate_orswot_tail. Returns ((L_base, L_off),
    (R_base, R_off)) as numpy arrays, every record with the sparse-clock flag."""
    def base(n, first):
        return tuple(generate_replicas(n, 2, first_obj=first, seed=seed, threads=threads))

    def heavy_gen(n, first, m, params):
        return tuple(generate_replicas(n, 2, first_obj=first, seed=TAIL_SEED + 0x5000 + m, threads=threads,
                                       params=params))

    return _tail_batch(n_obj, frac, sizes, first_obj, base, heavy_gen)


def _tail_batch(n_obj, frac, sizes, first_obj, base, heavy_gen):
    """The heavy-tail batch assembly shared by generate_orswot_tail and
    generate_orswot_csr_tail: base(n, first) -> the ordinary pairs of objects
    [first, first + n); heavy_gen(n, first, m, params) -> n heavy pairs of size
    m (pair index first..)."""
    step = max(1, int(round(1.0 / frac)))
    ids = np.arange(first_obj, first_obj + n_obj, dtype=np.int64)
    heavy = ids % step == 0
    kind = np.where(heavy, 1 + (ids // step) % len(sizes), 0)
    parts = []  # per kind: (positions, (lb, lo), (rb, ro))
    for k in range(len(sizes) + 1):
        pos = np.nonzero(kind == k)[0]
        if pos.size == 0:
            continue
        if k == 0:  # base pairs of the objects' own ids (the heavy ids' pairs generated and dropped)
            (lb, lo), (rb, ro) = base(n_obj, first_obj)
            sides = []
            for b, o in ((lb, lo), (rb, ro)):
                end = np.append(o[1:], np.uint64(b.nbytes))
                sides.append((b, o[pos], end[pos]))
        else:  # heavy object g of size m: pair index (g // step) // len(sizes) of the size-m generator
            m = sizes[k - 1]
            sides = heavy_gen(int(pos.size), int(ids[pos[0]] // step // len(sizes)), m,
                              {"member_universe": m, "ancestor_adds": m, "min_div_ops": max(4, m // 8),
                               "max_div_ops": max(8, m // 4)})
        parts.append((pos, sides))
    out = []
    for side in (0, 1):
        # gather every object's record (16-B units) into object order
        srcs, starts, counts, order = [], [], [], []
        base_units = 0
        for pos, sides in parts:
            b, o = sides[side][0], sides[side][1]
            end = sides[side][2] if len(sides[side]) == 3 else np.append(o[1:], np.uint64(b.nbytes))
            u = b.view(np.complex128) if b.nbytes % 16 == 0 else np.frombuffer(b.tobytes() + bytes(16 - b.nbytes % 16), np.complex128)
            sz = end.astype(np.int64) - o.astype(np.int64)
            srcs.append(u)
            starts.append(o.astype(np.int64) // 16 + base_units)
            counts.append(sz // 16)
            order.append(pos)
            base_units += u.size
        src = np.concatenate(srcs)
        pos_all = np.concatenate(order)
        st = np.empty(n_obj, np.int64)
        ct = np.empty(n_obj, np.int64)
        st[pos_all] = np.concatenate(starts)
        ct[pos_all] = np.concatenate(counts)
        off_units = np.concatenate(([0], np.cumsum(ct)[:-1]))
        idx = np.repeat(st - off_units, ct) + np.arange(int(ct.sum()), dtype=np.int64)
        out.append((src[idx].view(np.uint8).copy(), (off_units * 16).astype(np.uint64)))
    return out[0], out[1]


def _copy_sides(g, n_sides, n_obj):
    sides = []
    for s in range(n_sides):
        bp, op, nb = C.c_void_p(), C.c_void_p(), C.c_size_t()
        check(lib.crdt_orswot_gen_side(g, s, C.byref(bp), C.byref(op), C.byref(nb)), "gen_side")
        base = np.ctypeslib.as_array((C.c_uint8 * max(1, nb.value)).from_address(bp.value)).copy() \
            if nb.value else np.zeros(16, np.uint8)
        off = np.ctypeslib.as_array((C.c_uint64 * max(1, n_obj)).from_address(op.value)).copy()[:n_obj] \
            if n_obj else np.zeros(0, np.uint64)
        sides.append((base, off))
    return sides


def generate_replicas(n_obj, n_replicas=8, first_obj=0, seed=CONFIG5_SEED, params=None, sparse=True, threads=8,
                      keep=None):
    """Replica sets for anti-entropy (config 5, include/crdts_hip.h): a list of
    n_replicas (base, off) batches; replica r of object i is record i of batch r.
    keep=(first, count): only replicas [first, first + count) are returned
    (crdt_orswot_generate_replicas_subset; the same bytes)."""
    d = dict(CONFIG5)
    d.update(params or {})
    P = RepParams(**{k: int(v) for k, v in d.items()})
    g = C.c_void_p()
    fl = SPARSE_CLOCK if sparse else 0
    if keep is None:
        check(lib.crdt_orswot_generate_replicas(seed, first_obj, n_obj, C.byref(P), n_replicas, fl, threads,
                                                C.byref(g)), "generate_replicas")
        count = n_replicas
    else:
        count = int(keep[1])
        check(lib.crdt_orswot_generate_replicas_subset(seed, first_obj, n_obj, C.byref(P), n_replicas, int(keep[0]),
                                                       count, fl, threads, C.byref(g)), "generate_replicas_subset")
    try:
        return _copy_sides(g, count, n_obj)
    finally:
        lib.crdt_orswot_gen_free(g)


def generate_clocks_csr(n_obj, seed, universe=1024, slots=56, p_present=6 / 7, overlap=0.75, bits=40):
    """A pair of sparse clock batches (host numpy CSR: off u64, len u32, act
    u32, ctr u64) over an actor universe of `universe` ids: each clock draws
    from `slots` evenly spaced actor bands (one actor per band), each present
    with p_present (~48 of 56 by default); the other side picks the same actor
    in a band with probability `overlap` (replicas of one clock share most
    actors), counters U[1, 2^bits)."""
    rng = np.random.default_rng(seed)
    band = universe // slots
    js = rng.integers(0, band, (n_obj, slots), dtype=np.uint32)
    jo = np.where(rng.random((n_obj, slots)) < overlap, js, rng.integers(0, band, (n_obj, slots), dtype=np.uint32))
    base = (np.arange(slots, dtype=np.uint32) * band)[None, :]
    out = []
    for j in (js, jo):
        present = rng.random((n_obj, slots)) < p_present
        act = (base + j)[present].astype(np.uint32)
        ctr = rng.integers(1, 1 << bits, act.size, dtype=np.uint64)
        ln = present.sum(1).astype(np.uint32)
        off = np.zeros(n_obj, np.uint64)
        if n_obj:
            off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        out.append((off, ln, act, ctr))
    return out[0], out[1]


def generate_dense(n_obj, n_actors, seed, first_obj=0, bits=40, pct_zero=25, threads=8):
    rows = np.empty((n_obj, n_actors), dtype=np.uint64)
    check(lib.crdt_dense_generate(seed, first_obj, n_obj, n_actors, bits, pct_zero, threads,
                                  C.c_void_p(rows.ctypes.data)), "dense_generate")
    return rows
