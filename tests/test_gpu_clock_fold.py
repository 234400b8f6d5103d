"""GPU parity: crdt_clock_csr_fold and crdt_clock_dense_fold
(rust-crdt_amd/csrc/clock_fold.hip). The CSR fold on the replica batches of
tests/clock_foldgen.py (every R, every tier, the u64 and 2^31 edges), exact in
off, len and used entries against the dict fold, with the pre-filled output
outside the objects' regions left as it was; a fold output as a gapped input;
R = 2 against crdt_vclock_csr_merge; R = 3 and 8 against the oracle's chained
merge on generated clocks; PNCounter as two folds; malformed runs, which the
kernel is specified to survive (the code latches, that object comes out empty,
every other object is folded). The dense fold against numpy's running maximum,
out of place and in place. That the batches tell a subtly wrong walk from a
right one is tests/test_clock_foldgen.py's, without a GPU."""
import functools

import numpy as np
import pytest

import clock_foldgen as fg
import clock_rungen as cr
import mvreg_pairgen as pg
import oracle_ffi
from test_clock_foldgen import batch, stage

pytestmark = pytest.mark.gpu
PAT32, PAT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


# ------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def host_reps(R, gaps=True):
    """The batch by replica as numpy CSR, with gaps between the runs (0, 1 or 2
    cells holding junk entries after each run) -> a tuple of (off, len, act, ctr)."""
    out = []
    for r, runs in enumerate(fg.replicas(batch(R)[0])):
        off, ln, act, ctr = fg.csr(runs)
        if gaps:
            gap = (np.arange(len(runs), dtype=np.uint64) + r) % 3
            noff = off + np.cumsum(gap) - gap
            total = int(noff[-1] + ln[-1] + gap[-1]) if len(runs) else 0
            nact, nctr = np.full(total, 7, np.uint32), np.zeros(total, np.uint64)  # junk: a repeated actor, counter 0
            idx = np.repeat(noff - off, ln.astype(np.int64)) + np.arange(len(act), dtype=np.uint64)
            nact[idx.astype(np.int64)], nctr[idx.astype(np.int64)] = act, ctr
            off, act, ctr = noff, nact, nctr
        for x in (off, ln, act, ctr):
            x.flags.writeable = False
        out.append((off, ln, act, ctr))
    return tuple(out)


def _dev(h):
    import crdts_hip

    return crdts_hip.ClockBatch.from_host(*[np.array(x) for x in h])  # (copies: the cached arrays are read-only)


def _prefilled(n_obj, cap):
    """An output batch holding a pattern in all four arrays."""
    import crdts_hip
    import torch

    def full(n, pat, dt):
        return torch.full((n,), pat, dtype=dt, device="cuda:0")

    cap = max(1, cap)
    return crdts_hip.ClockBatch(full(n_obj, PAT64, torch.int64), full(n_obj, PAT32, torch.int32),
                                full(cap, PAT32, torch.int32), full(cap, PAT64, torch.int64), n_entries=cap)


def _check(out, hreps, exp, what, empty=()):
    """off = the sum of the replicas' offsets and len, exact; the used entries,
    exact; every cell outside the regions [off, off + the lengths' sum) holds
    the pattern. The objects in `empty` must have len 0."""
    off, ln, act, ctr = out.to_host()
    eoff = sum(h[0] for h in hreps)
    room = sum(h[1].astype(np.uint64) for h in hreps)
    assert (off == eoff).all(), f"{what}: off"
    elen = np.array([0 if i in empty else len(e) for i, e in enumerate(exp)], np.uint32)
    bad = np.nonzero(ln != elen)[0]
    assert bad.size == 0, f"{what}: len of {bad.size} objects differs, first {bad[:5].tolist()}"
    outside = np.ones(len(act), bool)
    wrong = []
    for i, (o, n, e) in enumerate(zip(eoff.tolist(), room.tolist(), exp)):
        outside[o:o + n] = False
        if i in empty:
            continue
        if act[o:o + len(e)].tolist() != [a for a, _ in e] or ctr[o:o + len(e)].tolist() != [c for _, c in e]:
            wrong.append(i)
    assert not wrong, f"{what}: {len(wrong)} objects differ, first {wrong[:5]}"
    assert (act[outside] == PAT32).all() and (ctr[outside] == PAT64).all(), f"{what}: written outside the regions"


def _used(res):
    """The used entries of a numpy CSR result, in object order."""
    off, ln, act, ctr = res
    idx = np.repeat(off - (np.cumsum(ln, dtype=np.uint64) - ln), ln.astype(np.int64)) + np.arange(int(ln.sum()),
                                                                                                  dtype=np.uint64)
    idx = idx.astype(np.int64)
    return act[idx], ctr[idx]


def _same(got, exp, what):
    assert (got[0] == exp[0]).all(), f"{what}: off"
    assert (got[1] == exp[1]).all(), f"{what}: len"
    (ga, gc), (ea, ec) = _used(got), _used(exp)
    assert (ga == ea).all() and (gc == ec).all(), f"{what}: entries"


def _oracle_chain(hreps):
    acc = hreps[0]
    for h in hreps[1:]:
        acc = oracle_ffi.vclock_csr_merge(acc, h)
    return acc


def _generated(n, seeds):
    import crdts_hip

    return [crdts_hip.generate_clocks_csr(n, seed=s)[k % 2] for k, s in enumerate(seeds)]


# ------------------------------------------------------------------ CSR fold
@pytest.mark.parametrize("R", fg.REPS)
def test_csr_fold_edges(gpu, R):
    exp = batch(R)[1]
    assert len(exp) % 64
    hreps = host_reps(R)
    reps = [_dev(h) for h in hreps]
    cap = sum(r.n_entries for r in reps) + 37
    for run in (1, 2):
        out = gpu.clock_csr_fold(reps, out=_prefilled(len(exp), cap))
        _check(out, hreps, exp, f"R={R}, run {run}")
    got = gpu.clock_csr_fold(reps)  # the default output: sized for the entries' sum
    assert got.n_entries == max(1, cap - 37) and got.clocks() == [list(e) for e in exp]


def test_csr_fold_output_is_a_gapped_input(gpu):
    objs, exp = batch(3)
    hreps = host_reps(3)
    first = gpu.clock_csr_fold([_dev(h) for h in hreps])
    other = [objs[(i + 1) % len(objs)][2] for i in range(len(objs))]
    oh = fg.csr(other)
    out = gpu.clock_csr_fold([first, _dev(oh)], out=_prefilled(len(objs), first.n_entries + len(oh[2]) + 5))
    _check(out, [first.to_host(), oh], [fg.fold_dict([e, o]) for e, o in zip(exp, other)], "fold of a fold")


def test_csr_fold_of_two_is_the_merge(gpu):
    import crdts_hip

    hreps = host_reps(2)
    S, O = [_dev(h) for h in hreps]
    cap = S.n_entries + O.n_entries
    m = gpu.clock_csr_merge(S, O, out=_prefilled(S.n_obj, cap))
    f = gpu.clock_csr_fold([S, O], out=_prefilled(S.n_obj, cap))
    _same(f.to_host(), m.to_host(), "fold of two")
    _check(f, hreps, batch(2)[1], "fold of two")
    for call in (lambda w: gpu.clock_csr_merge(S, O, out=w), lambda w: gpu.clock_csr_fold([S, O], out=w)):
        with pytest.raises(crdts_hip.CrdtError) as e:  # an out that is too small: the same code
            call(_prefilled(S.n_obj, cap - 1))
        assert e.value.code == crdts_hip.CRDT_ECAPACITY


@pytest.mark.parametrize("R", [3, 8])
def test_csr_fold_generated_vs_oracle_chain(gpu, R):
    """5,000 clocks of the 1024-actor universe, a seed per replica."""
    hreps = _generated(5000, range(40 + R, 40 + 2 * R))
    exp = _oracle_chain(hreps)
    out = gpu.clock_csr_fold([_dev(h) for h in hreps])
    _same(out.to_host(), exp, f"R={R}")
    assert 64 < int(sum(h[1].astype(np.int64) for h in hreps).max()) <= stage()  # (the LDS tier's objects)


@pytest.mark.parametrize("seed", [7, 8])
def test_pncounter_csr_fold(gpu, seed):
    P = _generated(1000, range(seed * 10, seed * 10 + 3))
    N = _generated(1000, range(seed * 10 + 5, seed * 10 + 8))
    op, on = gpu.pncounter_csr_fold([_dev(h) for h in P], [_dev(h) for h in N])
    _same(op.to_host(), _oracle_chain(P), "P")
    _same(on.to_host(), _oracle_chain(N), "N")


def _victims(objs, r):
    """One object per tier whose run in replica r has two entries at the least (never the last object)."""
    out = {}
    for i, o in enumerate(objs[:-1]):
        if len(o[r]) >= 2:
            out.setdefault(fg.tier(o, stage()), i)
    assert set(out) == {"regs", "lds", "mem"}
    return sorted(out.values())


@pytest.mark.parametrize("r", [0, 1, 2], ids=["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["zero_counter", "unsorted", "overlap"])
def test_csr_fold_malformed_run(gpu, kind, r):
    """A bad run in replica r of one object per tier: the code latches, those
    objects come out empty, every other object is folded, the context is clear
    afterwards. (A run that overlaps its neighbour is a placement fault:
    CRDT_EINVAL; the other two are CRDT_ENONCANON.)"""
    import crdts_hip

    objs, exp = batch(3)
    hreps = [tuple(x.copy() for x in h) for h in host_reps(3)]
    off, ln, act, ctr = hreps[r]
    bad = _victims(objs, r)
    for i in bad:
        o = int(off[i])
        if kind == "zero_counter":
            ctr[o + 1] = 0
        elif kind == "unsorted":
            act[[o, o + 1]] = act[[o + 1, o]]
        else:
            ln[i] = off[i + 1] - off[i] + 1  # one cell into the next object's run (inside the arrays)
    out = gpu.clock_csr_fold([_dev(h) for h in hreps], out=_prefilled(len(objs), sum(len(h[2]) for h in hreps) + 9),
                             check_status=False)
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == (crdts_hip.CRDT_EINVAL if kind == "overlap" else crdts_hip.CRDT_ENONCANON)
    gpu.status()  # cleared
    _check(out, hreps, exp, f"{kind} in replica {r}", empty=set(bad))


# ---------------------------------------------------------------- dense fold
EDGE = np.array(sorted({v for p in cr.PAIRS for v in p} | set(pg.EDGE) | {0, cr.M64}), np.uint64)


@pytest.mark.parametrize("n_slots", [1, 3, 16, 33, 128])
@pytest.mark.parametrize("R", fg.REPS)
def test_dense_fold(gpu, R, n_slots):
    """Several blocks, a word count that is no multiple of the 16-byte vector
    (odd n_obj and n_slots) and, for every shape, rows that start 8 bytes off
    a 16-byte boundary; out a fresh tensor, replica 0 and replica R - 1."""
    import torch

    n_obj = {1: 4099, 3: 4099, 16: 1031, 33: 1031, 128: 257}[n_slots]
    words = n_obj * n_slots
    rng = np.random.default_rng(R * 1000 + n_slots)
    host = EDGE[rng.integers(0, len(EDGE), (R, words))]
    exp = np.maximum.accumulate(host, axis=0)[-1]
    for shift in (0, 1):
        def rows():
            return [torch.from_numpy(np.concatenate([np.zeros(shift, np.uint64), h]).view(np.int64)).cuda()[shift:]
                    for h in host]

        fresh = torch.full((words + 2,), PAT64, dtype=torch.int64, device="cuda:0")
        got = gpu.dense_fold(rows(), n_slots, out=fresh[shift:shift + words])
        assert (got.cpu().numpy().view(np.uint64) == exp).all(), (shift, "fresh")
        edge = fresh.cpu().numpy().view(np.uint64)
        assert (edge[:shift] == PAT64).all() and (edge[shift + words:] == PAT64).all()
        assert (gpu.dense_fold(rows(), n_slots).cpu().numpy().view(np.uint64) == exp).all(), (shift, "default")
        for at in {0, R - 1}:
            d = rows()
            got = gpu.dense_fold(d, n_slots, out=d[at])
            assert got.data_ptr() == d[at].data_ptr()
            assert (got.cpu().numpy().view(np.uint64) == exp).all(), (shift, "in place", at)
            for q in set(range(R)) - {at}:
                assert (d[q].cpu().numpy().view(np.uint64) == host[q]).all()
        if R == 2:
            d = rows()
            gpu.dense_merge(d[0], d[1], n_slots, "vclock")
            assert (d[0].cpu().numpy().view(np.uint64) == exp).all()
    gpu.status()


def test_fold_einval_with_a_context(gpu):
    """The refusals of tests/test_clock_foldgen.py hold with a live context too, and an empty batch is CRDT_OK."""
    import ctypes as C

    import crdts_hip
    import torch
    from crdts_hip._lib import lib

    S = _dev(host_reps(2)[0])
    w = _prefilled(S.n_obj, 2 * S.n_entries)
    s, o = S.cstruct(), w.cout()
    views = (type(s) * 2)(s, s)
    assert lib.crdt_clock_csr_fold(gpu.ctx, views, 0, C.byref(o), None) == crdts_hip.CRDT_EINVAL
    assert lib.crdt_clock_csr_fold(gpu.ctx, views, 33, C.byref(o), None) == crdts_hip.CRDT_EINVAL
    alias = crdts_hip.ClockBatch(S.off, w.len, w.act, w.ctr, n_entries=w.n_entries).cout()
    assert lib.crdt_clock_csr_fold(gpu.ctx, views, 2, C.byref(alias), None) == crdts_hip.CRDT_EINVAL
    rows = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    with pytest.raises(crdts_hip.CrdtError):
        gpu.dense_fold([rows], 0)
    with pytest.raises(crdts_hip.CrdtError):
        gpu.dense_fold([], 4)
    none = crdts_hip.ClockBatch.from_lists([])
    assert gpu.clock_csr_fold([none, none]).n_obj == 0
    gpu.status()
