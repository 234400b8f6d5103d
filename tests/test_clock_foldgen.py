"""The replica batches of the clock fold (tests/clock_foldgen.py) earn their
place without a GPU: on every batch the GPU tests of crdt_clock_csr_fold use,
the plain dict fold equals the chain of dict merges and the chained C++
oracle's vclock_csr_merge in offsets, lengths and entries; every deliberately
wrong walk differs from the truth somewhere; the census finds every case the
batches were built for. One test needs the library but no device: the two
entry points refuse their CRDT_EINVAL cases before any device work."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import clock_foldgen as fg
import oracle_ffi
from test_oracle_csr import dict_merge

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stage():
    import crdts_hip

    return crdts_hip.CLOCK_FOLD_STAGE_ENTRIES


@functools.lru_cache(maxsize=None)
def batch(R):
    """-> (objects, the dict fold of each): made once, read-only."""
    objs = fg.batch(R, stage())
    return objs, tuple(tuple(fg.fold_dict(o)) for o in objs)


def test_constants_mirror_the_header():
    import crdts_hip

    src = open(os.path.join(REPO, "include", "crdts_hip.h")).read()
    for name in ("CLOCK_FOLD_MAX_REPS", "CLOCK_FOLD_STAGE_ENTRIES"):
        assert int(re.search(rf"#define CRDT_{name} (\d+)", src).group(1)) == getattr(crdts_hip, name)
    assert max(fg.REPS) == crdts_hip.CLOCK_FOLD_MAX_REPS


@pytest.mark.parametrize("R", fg.REPS)
def test_dict_fold_is_the_chain_of_dict_merges(R):
    objs, exp = batch(R)
    assert len(objs) % 64 and 150 <= len(objs) <= 400
    for o, e in zip(objs, exp):
        acc = sorted(dict(o[0]).items())
        for run in o[1:]:
            acc = dict_merge(dict(acc), dict(run))
        assert acc == list(e)
        assert all(a < b for (a, _), (b, _) in zip(e, e[1:])) and all(c > 0 for _, c in e)


@pytest.mark.parametrize("R", fg.REPS)
def test_dict_fold_is_the_oracle_chain(R):
    """The chained oracle ends at the summed offsets with the union's lengths and entries."""
    objs, exp = batch(R)
    reps = [fg.csr(runs) for runs in fg.replicas(objs)]
    acc = reps[0]
    for r in reps[1:]:
        acc = oracle_ffi.vclock_csr_merge(acc, r)
    off, ln, act, ctr = acc
    assert (off == sum(r[0] for r in reps)).all()
    assert ln.tolist() == [len(e) for e in exp]
    for o, e in zip(off.tolist(), exp):
        assert act[o:o + len(e)].tolist() == [a for a, _ in e] and ctr[o:o + len(e)].tolist() == [c for _, c in e]


@pytest.mark.parametrize("R", fg.REPS)
def test_the_walk_is_the_fold_and_every_mutant_is_not(R):
    objs, exp = batch(R)
    assert all(fg.ref_fold(o, stage()) == list(e) for o, e in zip(objs, exp))
    muts = fg.mutants(R, stage())
    assert tuple(muts) == fg.MUTANTS
    for name, knobs in muts.items():
        if R == 1 and name in ("last_counter", "counter_compare_low32", "actor_order_signed", "keep_first_dup"):
            continue  # (one replica: nothing to compare with)
        assert fg.differs(objs, stage(), knobs), name


def test_census_is_full():
    """Every case by at least 5 objects over the batches; every tier by at least 5 at every R."""
    total = {}
    for R in fg.REPS:
        c = fg.census(batch(R)[0], stage())
        for t in ("regs", "lds", "mem"):
            assert c[t] >= 5, (R, t, c[t])
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
        if R >= 3:  # every case at every R that has a middle replica
            assert all(v >= 5 for v in c.values()), (R, {k: v for k, v in c.items() if v < 5})
    assert all(v >= 5 for v in total.values()), {k: v for k, v in total.items() if v < 5}
    assert set(total) >= {"held_by_every", "held_by_first_only", "held_by_last_only", "held_by_first_and_last_only",
                          "max_in_first", "max_in_middle", "max_in_last", "max_tied", "shared_idx0", "shared_idx63",
                          "shared_idx64", "shared_last", "empty_first", "empty_middle", "empty_last", "all_empty",
                          "union64", "union65", "sum64", "sum65", "sum_stage", "sum_stage_p1", "len0", "len1",
                          "len63", "len64", "len65", "len_hundreds"}


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every CRDT_EINVAL case of the two folds, before any device work (as
    test_abi.py::test_device_entry_points_fail_cleanly_without_gpu): the
    context here is a stand-in that a refused call never looks into."""
    import crdts_hip
    from crdts_hip._lib import ClockCsr, ClockCsrOut, lib

    EINVAL, OK = crdts_hip.CRDT_EINVAL, crdts_hip.CRDT_OK
    ctx = C.cast(C.create_string_buffer(4096), C.c_void_p)
    arr = [np.zeros(8, np.uint64) for _ in range(12)]  # host arrays: a refused call reads none of them
    ptr = lambda a: a.ctypes.data  # noqa: E731
    MAXR = crdts_hip.CLOCK_FOLD_MAX_REPS

    # ---- dense
    rows = (C.c_void_p * (MAXR + 1))(*[ptr(arr[0])] * (MAXR + 1))
    dense = lambda c, h, R, out, n, slots: lib.crdt_clock_dense_fold(c, h, R, out, n, slots, None)  # noqa: E731
    assert dense(None, rows, 2, ptr(arr[1]), 4, 2) == EINVAL
    assert dense(ctx, None, 2, ptr(arr[1]), 4, 2) == EINVAL
    assert dense(ctx, rows, 0, ptr(arr[1]), 4, 2) == EINVAL
    assert dense(ctx, rows, MAXR + 1, ptr(arr[1]), 4, 2) == EINVAL
    assert dense(ctx, rows, 2, ptr(arr[1]), 4, 0) == EINVAL
    assert dense(ctx, rows, 2, None, 4, 2) == EINVAL
    holed = (C.c_void_p * 3)(ptr(arr[0]), None, ptr(arr[2]))
    assert dense(ctx, holed, 3, ptr(arr[1]), 4, 2) == EINVAL
    assert dense(ctx, holed, 3, None, 0, 2) == OK  # n_obj == 0: nothing to launch, null arrays included
    assert dense(ctx, rows, MAXR, ptr(arr[1]), 0, 2) == OK

    # ---- CSR
    def view(k, n_obj=4, n_entries=8, **nulls):
        f = dict(off=ptr(arr[k]), len=ptr(arr[k + 1]), act=ptr(arr[k + 2]), ctr=ptr(arr[k + 3]))
        f.update(nulls)
        return ClockCsr(f["off"], f["len"], f["act"], f["ctr"], n_obj, n_entries)

    def outv(n_entries=16, **nulls):
        f = dict(off=ptr(arr[8]), len=ptr(arr[9]), act=ptr(arr[10]), ctr=ptr(arr[11]))
        f.update(nulls)
        return ClockCsrOut(f["off"], f["len"], f["act"], f["ctr"], n_entries)

    def fold(c, views, out, R=None):
        h = (ClockCsr * max(1, len(views)))(*views) if views is not None else None
        return lib.crdt_clock_csr_fold(c, h, len(views) if R is None else R, C.byref(out) if out else None, None)

    good = [view(0), view(4)]
    assert fold(None, good, outv()) == EINVAL
    assert fold(ctx, None, outv(), R=2) == EINVAL
    assert fold(ctx, good, None) == EINVAL
    assert fold(ctx, good, outv(), R=0) == EINVAL
    assert fold(ctx, [view(0)] * (MAXR + 1), outv(8 * (MAXR + 1))) == EINVAL
    assert fold(ctx, [view(0), view(4, n_obj=5)], outv()) == EINVAL  # n_obj differ
    for f in ("off", "len", "act", "ctr"):  # a null array with n_obj > 0 (act / ctr: with n_entries > 0)
        assert fold(ctx, [view(0), view(4, **{f: None})], outv()) == EINVAL, f
        assert fold(ctx, [view(0, **{f: None}), view(4)], outv()) == EINVAL, f
        assert fold(ctx, good, outv(**{f: None})) == EINVAL, f
    for f, k in (("off", 4), ("len", 5), ("act", 2), ("ctr", 7)):  # an out array equal to a replica's array
        assert fold(ctx, good, outv(**{f: ptr(arr[k])})) == EINVAL, f
    assert fold(ctx, good, outv(15)) == crdts_hip.CRDT_ECAPACITY  # (the merge's code for an out too small)
    empty = [view(0, n_obj=0, n_entries=0, off=None, len=None, act=None, ctr=None)] * 2
    assert fold(ctx, empty, outv(0, off=None, len=None, act=None, ctr=None)) == OK  # n_obj == 0
