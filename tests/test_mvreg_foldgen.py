"""The replica generator and the numpy fold of tests/mvreg_foldgen.py earn
their place without a GPU: on every batch the GPU tests of crdt_mvreg_fold use,
the one-pass rule (fold_np), the chained numpy merge and the chained C++ oracle
give identical slabs; a brute-force census finds every class of slot the rule
distinguishes; and every deliberately wrong fold differs from the chain
wherever it can. One test needs the library but no device: the entry point
rejects a null context."""
import ctypes as C
import functools

import numpy as np
import pytest

import mvreg_foldgen as fg
import mvreg_pairgen as pg
from test_mvreg_pairgen import batch as pair_batch

ALL = fg.SHAPES + fg.EXTRA_SHAPES
PAIR_SHAPES = [(8, 4, 4, 1000, "W4"), (8, 70, 70, 100, "big")]  # FAST and BIG of tests/test_gpu_mvreg_merge.py


def out_cap_of(shape):
    return min(sum(shape[1]), 2048)


@functools.lru_cache(maxsize=None)
def batch(shape):
    """-> (reps, info, the chained oracle's fold at out_cap = the capacities' sum): made once, read-only."""
    A, caps, n, _ = shape
    info = {}
    reps = fg.gen(fg.seed_of(shape), n, A, caps, info)
    E = fg.chain_oracle(reps, out_cap_of(shape))
    for x in (*[a for r in reps for a in r], *E):
        x.flags.writeable = False
    return reps, info, E


@functools.lru_cache(maxsize=2)
def _relations(shape):
    return fg.relations(batch(shape)[0])


def test_tiers_of_the_table():
    """Every launch tier is in the table: 4, 3, 2 and 1 waves per block, both
    sides of the 64-slot boundary (as two and as eight replicas) and of the
    60 KB boundary."""
    for A, caps, _, t in ALL:
        assert fg.tier(A, caps) == t, (A, caps)
    assert {s[3] for s in fg.SHAPES} == {"W4", "W3", "W2", "W1", "big"}
    assert [fg.per_wave_bytes(A, (4, 4, 4)) for A in (200, 300, 600)] == [(96 * A + 216 + 15) & ~15
                                                                          for A in (200, 300, 600)]
    assert fg.per_wave_bytes(637, (4, 4, 4)) == 61376 <= fg.LDS_BYTES < fg.per_wave_bytes(638, (4, 4, 4)) == 61472
    assert fg.tier(8, (32, 32)) == fg.tier(8, (8,) * 8) == "W4"
    assert fg.tier(8, (32, 33)) == fg.tier(8, (8,) * 7 + (9,)) == "big"


@pytest.mark.parametrize("shape", ALL, ids=fg.shape_id)
def test_references_agree(shape):
    """fold_np == chain_np == the chained oracle, whole slabs, order included;
    the output counts are the census's slot-by-slot chain's."""
    reps, _, E = batch(shape)
    cap = out_cap_of(shape)
    for name, e, f, c in zip(("n", "clk", "val"), E, fg.fold_np(reps, cap, rel=_relations(shape)),
                             fg.chain_np(reps, cap)):
        assert (e == f).all(), f"{name}: oracle chain vs the one-pass rule"
        assert (e == c).all(), f"{name}: oracle chain vs numpy chain"
    assert len(set(E[0].tolist())) >= min(3, cap)


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=pg.shape_id)
def test_two_replicas_are_the_merge(shape):
    """On the pair batches of the merge's tests, both orientations, the
    one-pass rule gives the oracle's merge."""
    import oracle_ffi

    A, scap, ocap = shape[:3]
    S, O, _, E = pair_batch(shape)
    for got, exp in ((fg.fold_np([S, O], scap + ocap), E),
                     (fg.fold_np([O, S], scap + ocap), oracle_ffi.mvreg_merge(*O, *S, A, scap + ocap))):
        for name, g, e in zip(("n", "clk", "val"), got, exp):
            assert (g == e).all(), name


@pytest.mark.parametrize("shape", ALL, ids=fg.shape_id)
def test_census(shape):
    """Each class of mvreg_foldgen.classify that the capacities allow at all
    (possible()) is held by at least 5 registers, on every batch. In the two
    batches of 8 registers those are exactly the five that are not forced
    degenerate; registers of hundreds of slots over 8 base rows are dominated
    from outside throughout, so there the classes that need a malformed
    replica to survive come from the row the generator plants in each of the
    five.

    Also: the forced registers, the poison in every unused slot, values that
    are unique with the high bit set, hot slots touched, counters >= 2^63."""
    A, caps, n, _ = shape
    reps, info, E = batch(shape)
    c, outn = fg.classify(reps)
    assert (outn == E[0]).all()
    for k in fg.CLASSES:
        if fg.possible(k, caps):
            assert c[k] >= 5, (k, c)
        else:
            assert c[k] == 0, (k, c)
    R = len(caps)
    head = [[int(cn[i]) for cn, _, _ in reps] for i in range(4)]
    assert head[0] == list(caps) and head[3] == [0] * R
    assert head[1] == [0] * (R - 1) + [caps[-1]] and head[2] == [caps[0]] + [0] * (R - 1)
    if R > 2:
        mid = np.stack([cn for cn, _, _ in reps[1:-1]], axis=1)
        assert ((mid == 0).any(axis=1) & (reps[0][0] > 0) & (reps[-1][0] > 0)).sum() >= 1
    vals, nz = [], []
    for cn, clk, val in reps:
        use = np.arange(val.shape[1])[None, :] < cn[:, None]
        assert (clk[~use] == np.uint64(fg.POISON)).all() and (val[~use] == np.uint64(fg.POISON)).all()
        vals.append(val[use])
        nz.append(clk[use][clk[use] > 0])
    assert (np.concatenate(nz) >= np.uint64(2**63)).mean() >= 0.05
    vals = np.concatenate(vals)
    assert len(np.unique(vals)) == len(vals) and (vals >= np.uint64(2**63)).all() and fg.POISON not in vals
    assert all(info["touched"].get(h, 0) >= 1 for h in pg.hot(A)), (pg.hot(A), info["touched"])


@pytest.mark.parametrize("mutant", sorted(fg.MUTANTS))
@pytest.mark.parametrize("shape", ALL, ids=fg.shape_id)
def test_wrong_folds_differ(shape, mutant):
    """A fold that is wrong in one way gives another slab than the chain on
    this very batch, wherever it can (MUTANTS says where it cannot, and there
    it must not). A wrong fold that keeps more than every slot's worth of
    survivors differs too."""
    A, caps, n, _ = shape
    knobs, can = fg.MUTANTS[mutant]
    reps, _, E = batch(shape)
    rel = _relations(shape) if "key" not in knobs else None
    got = fg.fold_np(reps, out_cap_of(shape), rel=rel, **knobs)
    differs = sum(int((g != e).reshape(n, -1).any(axis=1).sum()) for g, e in zip(got, E))
    if can(A, caps):
        assert differs >= 1, (mutant, differs)
    else:
        assert differs == 0, (mutant, differs)


@pytest.mark.parametrize("shape", [fg.SHAPES[0], fg.SHAPES[1], fg.SHAPES[7]], ids=fg.shape_id)
def test_surviving_clocks_under_a_permutation(shape):
    """The set of surviving clocks of a register does not depend on the order
    of the replicas (the order of the survivors and the values of equal clocks do)."""
    A, caps, n, _ = shape
    reps, _, E = batch(shape)
    perm = list(range(len(caps)))[::-1]
    perm = perm[1:] + perm[:1]
    P = fg.fold_np([reps[r] for r in perm], out_cap_of(shape))
    for i in range(n):
        assert {r.tobytes() for r in E[1][i, :E[0][i]]} == {r.tobytes() for r in P[1][i, :P[0][i]]}, i


def test_fold_rejects_a_null_context():
    """No device needed: the entry point exists and checks its arguments before any device work."""
    import crdts_hip
    from crdts_hip._lib import MVRegViewC, lib

    views = (MVRegViewC * 2)(MVRegViewC(0x1000, 0x2000, 0x3000, 4), MVRegViewC(0x4000, 0x5000, 0x6000, 4))
    out = [C.c_void_p(0x7000), C.c_void_p(0x8000), C.c_void_p(0x9000)]
    assert lib.crdt_mvreg_fold(None, views, 2, *out, 8, 4, 8, None) == crdts_hip.CRDT_EINVAL
    assert lib.crdt_mvreg_fold(None, views, 2, None, None, None, 8, 0, 8, None) == crdts_hip.CRDT_EINVAL
