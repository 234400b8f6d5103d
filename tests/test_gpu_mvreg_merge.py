"""GPU parity: crdt_mvreg_merge and crdt_vclock_partial_cmp
(rust-crdt_amd/csrc/mvreg.hip) on the structured pairs of
tests/mvreg_pairgen.py, whole arrays exact against the C++ oracle, the output
pre-filled with a pattern. The shapes cover every launch tier (4, 3, 2 and 1
waves per block, the one-wave kernel, both sides of the 64-slot and the 60 KB
boundary: the tier of each is recomputed from the header's rule and asserted),
both orientations, the grid-stride loops, partial blocks, out_cap other than
the sum, the status paths and a side stream. That these inputs tell a subtly
wrong merge from a right one is tests/test_mvreg_pairgen.py's, without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import mvreg_pairgen as pg
from test_gpu_mvreg_ops import _assert_slab, _dev, _host, _patterned, _status_code
from test_mvreg_pairgen import CMP_A, batch, cmp_batch

pytestmark = pytest.mark.gpu
FAST, BIG = (8, 4, 4, 1000, "W4"), (8, 70, 70, 100, "big")
TIERS = [FAST, BIG]


def _merge(gpu, S, O, A, out_cap, **kw):
    """Host slabs -> the host output slab, written over a pattern."""
    S, O = (tuple(x.copy() for x in s) for s in (S, O))  # (the shared batches are read-only)
    return _host(gpu.mvreg_merge(_dev(S), _dev(O), A, out=_patterned(len(S[0]), out_cap, A), **kw))


@functools.lru_cache(maxsize=None)
def _oriented(shape, swapped):
    """-> (S, O, oracle's merge at out_cap = the capacities' sum), once."""
    import oracle_ffi

    S, O, _, E = batch(shape)
    if swapped:
        S, O = O, S
        E = oracle_ffi.mvreg_merge(*S, *O, shape[0], shape[1] + shape[2])
        for x in E:
            x.flags.writeable = False
    return S, O, E


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("swapped", [False, True], ids=["S_O", "O_S"])
@pytest.mark.parametrize("shape", pg.SHAPES, ids=pg.shape_id)
def test_mvreg_merge_parity(gpu, shape, swapped):
    A, scap, ocap, n, tier = shape
    assert pg.tier(A, scap, ocap) == tier  # a shape that changed tier is another test
    S, O, E = _oriented(shape, swapped)
    assert (E[0] < E[0].max()).any() and E[1][:, :, A - 1].any() and E[1][:, :, 0].any()
    _assert_slab(_merge(gpu, S, O, A, scap + ocap), E, what=f"{shape} swapped={swapped}")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 257])
def test_mvreg_merge_small_n(gpu, n):
    """Partial last blocks and partial waves: the first n objects of a batch."""
    A, scap, ocap = FAST[:3]
    S, O, E = _oriented(FAST, False)
    _assert_slab(_merge(gpu, tuple(x[:n] for x in S), tuple(x[:n] for x in O), A, scap + ocap),
                 tuple(x[:n] for x in E))


@pytest.mark.parametrize("shape,per_cu,extra", [(FAST, 32, 101), ((300, 4, 4, 1000, "W3"), 32, 101),
                                                ((2, 65, 8, 1000, "big"), 16, 37)], ids=["W4", "W3", "big"])
def test_mvreg_merge_grid_stride(gpu, shape, per_cu, extra):
    """More objects than one sweep of the grid (the fast kernel launches at
    most 32 / W blocks of W waves per CU, the one-wave kernel 16 blocks): the
    loops' second round, the prefetch of the next pair included. The batch is
    a 1,000-object batch tiled, every value globally unique."""
    import oracle_ffi

    A, scap, ocap, _, tier = shape
    assert pg.tier(A, scap, ocap) == tier
    n = per_cu * _cus() + extra
    W = int(tier[1]) if tier != "big" else 1
    assert n > _cus() * (per_cu // W) * W  # (the launcher's grid, in objects)
    S, O, _, _ = batch(shape)
    S, O = pg.tile(S, O, n)
    vals = np.concatenate([S[2][S[2] > 0], O[2][O[2] > 0]])
    assert len(np.unique(vals)) == len(vals)
    _assert_slab(_merge(gpu, S, O, A, scap + ocap), oracle_ffi.mvreg_merge(*S, *O, A, scap + ocap))


@pytest.mark.parametrize("shape", TIERS, ids=["fast", "big"])
def test_mvreg_merge_out_cap(gpu, shape):
    """out_cap = the largest survivor count of the batch (below the sum), and
    out_cap above the sum: the extra slots are zero-filled."""
    import oracle_ffi

    A, scap, ocap, n, tier = shape
    S, O, E = _oriented(shape, False)
    keep = E[0] < scap + ocap  # (object 0, both sides full, may keep every slot)
    S, O = tuple(x[keep] for x in S), tuple(x[keep] for x in O)
    tight, wide = int(E[0][keep].max()), scap + ocap + 5
    assert keep.sum() > n // 2 and (E[0][keep] == tight).any()
    for out_cap in (tight, wide):
        assert pg.tier(A, scap, ocap, out_cap) == tier
        got = _merge(gpu, S, O, A, out_cap)
        _assert_slab(got, oracle_ffi.mvreg_merge(*S, *O, A, out_cap), what=f"out_cap {out_cap}")
    assert not got[1][:, scap + ocap:].any() and not got[2][:, scap + ocap:].any()


def test_mvreg_merge_side_stream(gpu):
    """The launch and the status read go to the stream given."""
    import torch

    A, scap, ocap, n, _ = FAST
    S, O, E = _oriented(FAST, False)
    dS, dO = (_dev(tuple(x.copy() for x in s)) for s in (S, O))
    out = _patterned(n, scap + ocap, A)
    side, cur = torch.cuda.Stream(device=0), torch.cuda.current_stream(0)
    side.wait_stream(cur)
    got = gpu.mvreg_merge(dS, dO, A, out=out, stream=side)
    cur.wait_stream(side)
    assert all(g is o for g, o in zip(got, out))
    _assert_slab(_host(got), E)


# ------------------------------------------------------------------ status
@pytest.mark.parametrize("side", ["self", "other"])
@pytest.mark.parametrize("shape", TIERS, ids=["fast", "big"])
def test_mvreg_merge_noncanonical_count(gpu, shape, side):
    """A count of cap + 1 latches CRDT_ENONCANON for its object alone: its
    output is left unwritten, every other object is exact; the engine is
    usable afterwards."""
    import crdts_hip

    A, scap, ocap, n, _ = shape
    S, O, E = _oriented(shape, False)
    bad = 5
    cnt = (S if side == "self" else O)[0].copy()
    cnt[bad] = (scap if side == "self" else ocap) + 1
    Sb, Ob = ((cnt,) + S[1:], O) if side == "self" else (S, (cnt,) + O[1:])
    with pytest.raises(crdts_hip.CrdtError) as e:
        _merge(gpu, Sb, Ob, A, scap + ocap)
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    got = _merge(gpu, Sb, Ob, A, scap + ocap, check_status=False)
    assert _status_code(gpu) == crdts_hip.CRDT_ENONCANON
    _assert_slab(got, E, rows=[i for i in range(n) if i != bad])
    assert got[0][bad] == 0x5A5A5A5A and (got[1][bad] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    _assert_slab(_merge(gpu, S, O, A, scap + ocap), E, what="a later good call")


@pytest.mark.parametrize("shape", TIERS, ids=["fast", "big"])
def test_mvreg_merge_capacity(gpu, shape):
    """out_cap one below the largest survivor count latches CRDT_ECAPACITY for
    the objects that need it; every other object is exact."""
    import crdts_hip

    A, scap, ocap, n, tier = shape
    S, O, E = _oriented(shape, False)
    out_cap = int(E[0].max()) - 1
    fits = np.nonzero(E[0] <= out_cap)[0]
    assert out_cap >= 1 and 0 < len(fits) < n and pg.tier(A, scap, ocap, out_cap) == tier
    with pytest.raises(crdts_hip.CrdtError) as e:
        _merge(gpu, S, O, A, out_cap)
    assert e.value.code == crdts_hip.CRDT_ECAPACITY
    got = _merge(gpu, S, O, A, out_cap, check_status=False)
    assert _status_code(gpu) == crdts_hip.CRDT_ECAPACITY
    _assert_slab(got, (E[0], E[1][:, :out_cap], E[2][:, :out_cap]), rows=fits)
    over = np.nonzero(E[0] > out_cap)[0]
    assert (got[0][over] == 0x5A5A5A5A).all()
    _assert_slab(_merge(gpu, S, O, A, scap + ocap), E, what="a later good call")


def test_mvreg_merge_einval(gpu):
    """The CRDT_EINVAL table of crdt_mvreg_merge, before any device work; no
    objects is CRDT_OK, null arrays included."""
    import crdts_hip
    from crdts_hip._lib import lib

    A, scap, ocap, n, _ = FAST
    S, O, E = _oriented(FAST, False)
    s, o = (_dev(tuple(x.copy() for x in t)) for t in (S, O))
    out = _patterned(n, scap + ocap, A)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(ctx=gpu.ctx, s=s, scap_=scap, o=o, ocap_=ocap, out=out, outcap=scap + ocap, n_=n, A_=A):
        return lib.crdt_mvreg_merge(ctx, p(s[0]), p(s[1]), p(s[2]), scap_, p(o[0]), p(o[1]), p(o[2]), ocap_,
                                    p(out[0]), p(out[1]), p(out[2]), outcap, n_, A_, None)

    def without(t, i):
        return tuple(None if k == i else x for k, x in enumerate(t))

    bad = [call(ctx=None), call(scap_=0), call(ocap_=0), call(scap_=1025), call(ocap_=1025), call(outcap=0),
           call(A_=0)]
    bad += [call(s=without(s, i)) for i in range(3)] + [call(o=without(o, i)) for i in range(3)]
    bad += [call(out=without(out, i)) for i in range(3)]
    assert bad == [crdts_hip.CRDT_EINVAL] * len(bad), bad
    gpu.status()
    assert (out[0].cpu().numpy() == 0x5A5A5A5A).all()  # nothing was launched
    none = (None, None, None)
    assert call(s=none, o=none, out=none, n_=0) == crdts_hip.CRDT_OK
    assert call(s=none, o=none, out=none, n_=0, scap_=0) == crdts_hip.CRDT_EINVAL  # (the capacities are still checked)
    assert call() == crdts_hip.CRDT_OK
    gpu.status()
    _assert_slab(_host(out), E)
    Z = tuple(x[:0].copy() for x in S), tuple(x[:0].copy() for x in O)
    got = gpu.mvreg_merge(_dev(Z[0]), _dev(Z[1]), A)
    assert got[0].numel() == 0 and tuple(got[1].shape) == (0, scap + ocap, A)


# ------------------------------------------------------------- partial_cmp
def _cmp(gpu, a, b, A):
    import torch

    ta, tb = (torch.from_numpy(x.copy().view(np.int64)).to("cuda:0") for x in (a, b))
    return gpu.vclock_partial_cmp(ta, tb, A).cpu().numpy()


@pytest.mark.parametrize("A", CMP_A)
def test_vclock_partial_cmp_rows(gpu, A):
    """Per slot x: equal rows, a > b at x only, a < b at x only, a > b at x
    with a < b elsewhere, over u64 edge counters; 4 A + 3 pairs (no multiple
    of the pairs per wave), and the first pair alone."""
    a, b, e = cmp_batch(A)
    assert set(e.tolist()) == ({0, 1, -1, 2} if A > 1 else {0, 1, -1})
    got = _cmp(gpu, a, b, A)
    bad = np.nonzero(got != e)[0]
    assert bad.size == 0, f"{bad.size} pairs differ, first {bad[:8].tolist()} (pair 4 x + t: slot x, case t)"
    for k in (1, 2):
        assert (_cmp(gpu, a[k:k + 1], b[k:k + 1], A) == e[k:k + 1]).all()


def test_vclock_partial_cmp_grid_stride(gpu, oracle):
    """A = 1: 256 pairs per block, 16 blocks per CU, 3 pairs past one sweep."""
    n = 4096 * _cus() + 3
    rng = np.random.default_rng(0xC1)
    edge = np.array(pg.EDGE + (0, 2**64 - 1), np.uint64)
    a, b = edge[rng.integers(0, len(edge), (n, 1))], edge[rng.integers(0, len(edge), (n, 1))]
    e = oracle.partial_cmp_rows(a, b, 1)
    assert set(e.tolist()) == {0, 1, -1}
    assert (e == pg.cmp_np(a, b)).all()
    got = _cmp(gpu, a, b, 1)
    bad = np.nonzero(got != e)[0]
    assert bad.size == 0, f"{bad.size} pairs differ, first {bad[:8].tolist()}"
