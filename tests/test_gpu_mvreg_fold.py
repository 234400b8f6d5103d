"""GPU parity: crdt_mvreg_fold (rust-crdt_amd/csrc/mvreg_fold.hip) on the
replica batches of tests/mvreg_foldgen.py, whole arrays exact against the
chained C++ oracle, the output pre-filled with a pattern. The shapes cover
every launch tier (4, 3, 2 and 1 waves per block, the one-wave kernel, both
sides of the 64-slot and the 60 KB boundary: the tier of each is recomputed
from the header's rule and asserted), one and two replicas, the grid-stride
loops, partial blocks, out_cap other than the sum, the status paths, the
argument checks and a side stream. That these inputs tell a subtly wrong fold
from a right one is tests/test_mvreg_foldgen.py's, without a GPU."""
import ctypes as C

import numpy as np
import pytest

import mvreg_foldgen as fg
from test_gpu_mvreg_merge import BIG as PAIR_BIG
from test_gpu_mvreg_merge import FAST as PAIR_FAST
from test_gpu_mvreg_merge import _oriented
from test_gpu_mvreg_ops import PATTERN, _assert_slab, _dev, _host, _patterned, _status_code
from test_mvreg_foldgen import batch, out_cap_of

pytestmark = pytest.mark.gpu
TIERS = [fg.FAST, fg.BIG]


def _fold(gpu, reps, A, out_cap, **kw):
    """Host slabs -> the host output slab, written over a pattern."""
    reps = [tuple(x.copy() for x in r) for r in reps]  # (the shared batches are read-only)
    return _host(gpu.mvreg_fold([_dev(r) for r in reps], A, out=_patterned(len(reps[0][0]), out_cap, A), **kw))


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows(slab, rows):
    return tuple(x[rows] for x in slab)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("shape", fg.SHAPES, ids=fg.shape_id)
def test_mvreg_fold_parity(gpu, shape):
    A, caps, n, tier = shape
    assert fg.tier(A, caps) == tier  # a shape that changed tier is another test
    reps, _, E = batch(shape)
    assert (E[0] < E[0].max()).any() and E[1][:, :, A - 1].any() and E[1][:, :, 0].any()
    _assert_slab(_fold(gpu, reps, A, out_cap_of(shape)), E, what=f"{shape}")


@pytest.mark.parametrize("shape", TIERS, ids=["fast", "big"])
def test_mvreg_fold_one_replica(gpu, shape):
    """R = 1 copies replica 0 through, zero-filled to out_cap (the poison of
    its unused slots stays behind)."""
    A, caps, n, _ = shape
    reps, _, _ = batch(shape)
    cn, clk, val = reps[0]
    cap = caps[0] + 3
    assert fg.tier(A, caps[:1]) == "W4"  # (one replica of the big shape fits the fast kernel: the next test)
    use = np.arange(caps[0])[None, :] < cn[:, None]
    E = (cn, np.zeros((n, cap, A), np.uint64), np.zeros((n, cap), np.uint64))
    E[1][:, :caps[0]] = np.where(use[:, :, None], clk, np.uint64(0))
    E[2][:, :caps[0]] = np.where(use, val, np.uint64(0))
    _assert_slab(_fold(gpu, reps[:1], A, cap), E)


def test_mvreg_fold_one_replica_big(gpu):
    """R = 1 through the one-wave kernel: 70 slots."""
    A, scap = PAIR_BIG[0], PAIR_BIG[1]
    S, _, _ = _oriented(PAIR_BIG, False)
    assert fg.tier(A, (scap,)) == "big"
    E = (S[0], np.zeros((len(S[0]), scap + 1, A), np.uint64), np.zeros((len(S[0]), scap + 1), np.uint64))
    E[1][:, :scap], E[2][:, :scap] = S[1], S[2]  # (the pair batches hold zeros in their unused slots)
    _assert_slab(_fold(gpu, [S], A, scap + 1), E)


@pytest.mark.parametrize("swapped", [False, True], ids=["S_O", "O_S"])
@pytest.mark.parametrize("shape", [PAIR_FAST, PAIR_BIG], ids=["fast", "big"])
def test_mvreg_fold_two_replicas_are_the_merge(gpu, shape, swapped):
    """R = 2 is byte-equal to the oracle's merge on the merge's own batches."""
    A, scap, ocap, _, tier = shape
    assert fg.tier(A, (scap, ocap)) == tier
    S, O, E = _oriented(shape, swapped)
    _assert_slab(_fold(gpu, [S, O], A, scap + ocap), E)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 257])
def test_mvreg_fold_small_n(gpu, n):
    """Partial last blocks and partial waves: the first n registers of a batch."""
    A, caps = fg.FAST[:2]
    reps, _, E = batch(fg.FAST)
    _assert_slab(_fold(gpu, [_rows(r, slice(0, n)) for r in reps], A, sum(caps)), _rows(E, slice(0, n)))


@pytest.mark.parametrize("shape,per_cu,extra", [(fg.FAST, 32, 101), (fg.BIG, 16, 37)], ids=["fast", "big"])
def test_mvreg_fold_grid_stride(gpu, shape, per_cu, extra):
    """More registers than one sweep of the grid (the fast kernel launches at
    most 8 blocks of 4 waves per CU, the one-wave kernel 16 blocks): the
    loops' second round, the prefetch of the next register included. The
    batch is tiled, every value globally unique."""
    A, caps, _, tier = shape
    assert fg.tier(A, caps) == tier
    n = per_cu * _cus() + extra
    reps = fg.tile(batch(shape)[0], n)
    vals = np.concatenate([v[v != np.uint64(fg.POISON)] for _, _, v in reps])
    assert len(np.unique(vals)) == len(vals)
    _assert_slab(_fold(gpu, reps, A, sum(caps)), fg.chain_oracle(reps, sum(caps)))


@pytest.mark.parametrize("shape", TIERS, ids=["fast", "big"])
def test_mvreg_fold_out_cap(gpu, shape):
    """out_cap = the largest survivor count of the batch, and out_cap above the
    capacities' sum: the extra slots are zero-filled."""
    A, caps, n, tier = shape
    reps, _, E = batch(shape)
    T = sum(caps)
    keep = E[0] < T  # (register 0, every replica full, may keep every slot)
    reps = [_rows(r, keep) for r in reps]
    tight, wide = int(E[0][keep].max()), T + 5
    assert keep.sum() > n // 2 and tight < T
    for out_cap in (tight, wide):
        got = _fold(gpu, reps, A, out_cap)
        _assert_slab(got, fg.chain_oracle(reps, out_cap), what=f"out_cap {out_cap}")
    assert not got[1][:, T:].any() and not got[2][:, T:].any()


def test_mvreg_fold_side_stream(gpu):
    """The launch and the status read go to the stream given."""
    import torch

    A, caps, n, _ = fg.FAST
    reps, _, E = batch(fg.FAST)
    dreps = [_dev(tuple(x.copy() for x in r)) for r in reps]
    out = _patterned(n, sum(caps), A)
    side, cur = torch.cuda.Stream(device=0), torch.cuda.current_stream(0)
    side.wait_stream(cur)
    got = gpu.mvreg_fold(dreps, A, out=out, stream=side)
    cur.wait_stream(side)
    assert all(g is o for g, o in zip(got, out))
    _assert_slab(_host(got), E)
    assert gpu.mvreg_fold(dreps, A)[2].shape[1] == sum(caps)  # the default out_cap


# ------------------------------------------------------------------ status
@pytest.mark.parametrize("shape", TIERS, ids=["fast", "big"])
def test_mvreg_fold_noncanonical_count(gpu, shape):
    """A count of cap + 1 in a middle replica latches CRDT_ENONCANON for its
    register alone: its output is left unwritten, every other register is
    exact; the engine is usable afterwards."""
    import crdts_hip

    A, caps, n, _ = shape
    reps, _, E = batch(shape)
    bad, T = 6, sum(caps)
    cnt = reps[1][0].copy()
    cnt[bad] = caps[1] + 1
    broken = [reps[0], (cnt,) + tuple(reps[1][1:]), reps[2]]
    with pytest.raises(crdts_hip.CrdtError) as e:
        _fold(gpu, broken, A, T)
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    got = _fold(gpu, broken, A, T, check_status=False)
    assert _status_code(gpu) == crdts_hip.CRDT_ENONCANON
    _assert_slab(got, E, rows=[i for i in range(n) if i != bad])
    assert got[0][bad] == 0x5A5A5A5A and (got[1][bad] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    assert (got[2][bad] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    _assert_slab(_fold(gpu, reps, A, T), E, what="a later good call")


@pytest.mark.parametrize("shape", TIERS, ids=["fast", "big"])
def test_mvreg_fold_capacity(gpu, shape):
    """out_cap one below the largest survivor count latches CRDT_ECAPACITY for
    exactly the registers that need it: they are left unwritten, every other
    register is exact."""
    import crdts_hip

    A, caps, n, tier = shape
    reps, _, E = batch(shape)
    out_cap = int(E[0].max()) - 1
    fits, over = np.nonzero(E[0] <= out_cap)[0], np.nonzero(E[0] > out_cap)[0]
    assert out_cap >= 1 and 0 < len(fits) < n
    with pytest.raises(crdts_hip.CrdtError) as e:
        _fold(gpu, reps, A, out_cap)
    assert e.value.code == crdts_hip.CRDT_ECAPACITY
    got = _fold(gpu, reps, A, out_cap, check_status=False)
    assert _status_code(gpu) == crdts_hip.CRDT_ECAPACITY
    _assert_slab(got, (E[0], E[1][:, :out_cap], E[2][:, :out_cap]), rows=fits)
    assert (got[0][over] == 0x5A5A5A5A).all() and (got[1][over] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    _assert_slab(_fold(gpu, reps, A, sum(caps)), E, what="a later good call")


def test_mvreg_fold_einval(gpu):
    """The CRDT_EINVAL table of crdt_mvreg_fold, before any device work: the
    pattern is intact. No registers is CRDT_OK, null arrays included; an
    output array that is a replica's is rejected."""
    import crdts_hip
    from crdts_hip._lib import MVRegViewC, lib

    A, caps, n, _ = fg.FAST
    reps, _, E = batch(fg.FAST)
    d = [_dev(tuple(x.copy() for x in r)) for r in reps]
    out = _patterned(n, sum(caps), A)
    ptr = lambda t: (t.data_ptr() if t is not None else None)  # noqa: E731

    def views(reps_=d, caps_=caps, count=None):
        v = [MVRegViewC(ptr(r[0]), ptr(r[1]), ptr(r[2]), c) for r, c in zip(reps_, caps_)]
        return (MVRegViewC * max(1, count or len(v)))(*(v * 33)[:count or len(v)])

    def call(ctx=gpu.ctx, h=None, R=len(caps), out=out, outcap=sum(caps), n_=n, A_=A, null_h=False):
        h = None if null_h else (h if h is not None else views())
        return lib.crdt_mvreg_fold(ctx, h, R, C.c_void_p(ptr(out[0])), C.c_void_p(ptr(out[1])), C.c_void_p(ptr(out[2])),
                                   outcap, n_, A_, None)

    def without(t, i):
        return tuple(None if k == i else x for k, x in enumerate(t))

    bad = [call(ctx=None), call(null_h=True), call(R=0), call(h=views(count=33), R=33),
           call(h=views(caps_=(4, 0, 4))), call(h=views(caps_=(4, 1025, 4))), call(h=views(caps_=(1000, 1000, 49))),
           call(outcap=0), call(outcap=2049), call(A_=0)]
    bad += [call(h=views(reps_=[d[0], without(d[1], i), d[2]])) for i in range(3)]
    bad += [call(out=without(out, i)) for i in range(3)]
    bad += [call(out=(d[1][0], out[1], out[2])), call(out=(out[0], d[2][1], out[2])),
            call(out=(out[0], out[1], d[0][2]))]  # an output array that is a replica's
    assert bad == [crdts_hip.CRDT_EINVAL] * len(bad), bad
    gpu.status()
    assert (out[0].cpu().numpy() == 0x5A5A5A5A).all() and (out[1].cpu().numpy() == PATTERN).all()  # nothing ran
    none, nulls = (None, None, None), views(reps_=[(None, None, None)] * 3)
    assert call(h=nulls, out=none, n_=0) == crdts_hip.CRDT_OK
    assert call(h=views(reps_=[(None, None, None)] * 3, caps_=(4, 0, 4)), out=none, n_=0) == crdts_hip.CRDT_EINVAL
    assert call() == crdts_hip.CRDT_OK
    gpu.status()
    _assert_slab(_host(out), E)
    got = gpu.mvreg_fold([_dev(tuple(x[:0].copy() for x in r)) for r in reps], A)
    assert got[0].numel() == 0 and tuple(got[1].shape) == (0, sum(caps), A)
