"""CPU: the host side of the batched read path (include/crdts_hip.h "Batched
read path"): the five entry points are declared, bound and exported; every
argument check comes before any device work; ReadQueries packs the arrays
crdt_read_queries describes; and the reference helper the GPU tests compare
against (tests/read_ref.py) reproduces the ctx asserts of the reference's
Orswot KATs on the Python restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import kat_runner
import read_ref

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["crdt_orswot_read_sizes", "crdt_orswot_read", "crdt_map_read_sizes", "crdt_map_read", "crdt_map_mvreg_get"]
CRDT_EINVAL = -1


def test_the_five_symbols_are_declared_bound_and_exported():
    import crdts_hip
    from crdts_hip._lib import lib

    header = open(os.path.join(HERE, "..", "include", "crdts_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in crdts_hip.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    for m in ("orswot_read", "map_read", "map_mvreg_get"):
        assert callable(getattr(crdts_hip.Engine, m)), m
    for cls in (crdts_hip.MapSlab, crdts_hip.MapMapSlab, crdts_hip.MapOrswotSlab):
        assert callable(cls.read_view)
    assert "ReadQueries" in crdts_hip.__all__


class _Args:
    """Valid arguments of the five calls over host memory nobody dereferences:
    every case below must be refused before the context or an array is touched.
    The context is a zeroed block standing in for a crdt_ctx."""

    def __init__(self):
        from crdts_hip import _lib as L

        self.L = L
        self.ctx = C.create_string_buffer(4096)
        self.mem = [np.zeros(64, np.uint64) for _ in range(24)]
        p = [m.ctypes.data for m in self.mem]
        self.p = p
        self.batch = L.Batch(p[0], p[1], 2, 512)
        self.q = L.ReadQueriesC(p[2], p[3], p[4], p[5], 3)
        self.sizes = L.ReadSizesC(*p[6:12])
        self.out = L.ReadOutC(p[12], p[13], p[14], 8, p[15], p[16], p[17], 8, p[18], p[19], 8)
        self.view = L.MapReadViewC(p[20], p[21], p[22], p[23], 4)
        self.slab = L.MapSlabC(p[20], p[21], p[22], p[23], p[0], p[1], p[6], p[7], p[8], p[9], p[10], 4, 2, 2, 2)

    def orswot_sizes(self, ctx=True, batch=True, q=True, A=16, flags=0, sizes=True):
        r = C.byref
        return self.L.lib.crdt_orswot_read_sizes(self.ctx if ctx else None, r(self.batch) if batch else None,
                                                 r(self.q) if q else None, A, flags, r(self.sizes) if sizes else None,
                                                 None)

    def orswot_write(self, ctx=True, batch=True, q=True, A=16, flags=0, out=True):
        r = C.byref
        return self.L.lib.crdt_orswot_read(self.ctx if ctx else None, r(self.batch) if batch else None,
                                           r(self.q) if q else None, A, flags, r(self.out) if out else None, None)

    def map_sizes(self, ctx=True, view=True, q=True, n=2, A=16, sizes=True):
        r = C.byref
        return self.L.lib.crdt_map_read_sizes(self.ctx if ctx else None, r(self.view) if view else None,
                                              r(self.q) if q else None, n, A, r(self.sizes) if sizes else None, None)

    def map_write(self, ctx=True, view=True, q=True, n=2, A=16, out=True):
        r = C.byref
        return self.L.lib.crdt_map_read(self.ctx if ctx else None, r(self.view) if view else None,
                                        r(self.q) if q else None, n, A, r(self.out) if out else None, None)

    def mvreg_get(self, ctx=True, slab=True, q=True, n=2, A=16, outs=(11, 12, 13), cap=2):
        r = C.byref
        o = [self.p[k] if k is not None else None for k in outs]
        return self.L.lib.crdt_map_mvreg_get(self.ctx if ctx else None, r(self.slab) if slab else None,
                                             r(self.q) if q else None, n, A, o[0], o[1], o[2], cap, None)


@pytest.fixture()
def a():
    return _Args()


def test_null_context_and_structs_are_einval(a):
    for call in (a.orswot_sizes, a.orswot_write, a.map_sizes, a.map_write, a.mvreg_get):
        assert call(ctx=False) == CRDT_EINVAL
        assert call(q=False) == CRDT_EINVAL
    assert a.orswot_sizes(batch=False) == a.orswot_write(batch=False) == CRDT_EINVAL
    assert a.orswot_sizes(sizes=False) == a.map_sizes(sizes=False) == CRDT_EINVAL
    assert a.orswot_write(out=False) == a.map_write(out=False) == CRDT_EINVAL
    assert a.map_sizes(view=False) == a.map_write(view=False) == a.mvreg_get(slab=False) == CRDT_EINVAL


def test_actor_counts_flags_and_capacities_are_einval(a):
    assert a.orswot_sizes(A=0) == a.orswot_write(A=0) == CRDT_EINVAL
    for A in (0, 129):
        assert a.map_sizes(A=A) == a.map_write(A=A) == a.mvreg_get(A=A) == CRDT_EINVAL
    for flags in (2, 3, 4):  # only 0 and CRDT_ORSWOT_SPARSE_CLOCK
        assert a.orswot_sizes(flags=flags) == a.orswot_write(flags=flags) == CRDT_EINVAL
    for kcap in (0, 8193):
        a.view.kcap = a.slab.kcap = kcap
        assert a.map_sizes() == a.map_write() == a.mvreg_get() == CRDT_EINVAL
    a.slab.kcap = 4
    assert a.mvreg_get(cap=1) == CRDT_EINVAL  # out_cap < slab.mcap


def test_null_required_arrays_are_einval(a):
    for f in ("base", "off"):
        b = _Args()
        setattr(b.batch, f, None)
        assert b.orswot_sizes() == b.orswot_write() == CRDT_EINVAL, f
    for f in ("obj_end", "kind", "key"):
        b = _Args()
        setattr(b.q, f, None)
        for call in (b.orswot_sizes, b.orswot_write, b.map_sizes, b.map_write, b.mvreg_get):
            assert call() == CRDT_EINVAL, f
    for f in ("clock", "n_keys", "keys", "eclock"):
        b = _Args()
        setattr(b.view, f, None)
        assert b.map_sizes() == b.map_write() == CRDT_EINVAL, f
    for f in ("n_keys", "keys", "mv_n", "mv_clock", "mv_val"):
        b = _Args()
        setattr(b.slab, f, None)
        assert b.mvreg_get() == CRDT_EINVAL, f
    for f in ("add_act", "add_ctr", "rm_act", "rm_ctr", "list_key"):  # a wanted group's arrays
        b = _Args()
        setattr(b.out, f, None)
        assert b.orswot_write() == b.map_write() == CRDT_EINVAL, f
    for k in range(3):
        outs = [11, 12, 13]
        outs[k] = None
        assert a.mvreg_get(outs=tuple(outs)) == CRDT_EINVAL


def test_an_output_equal_to_an_input_is_einval(a):
    for name, k in dict(obj_end=2, kind=3, key=4, actor=5, base=0, off=1).items():
        b = _Args()
        b.sizes.val = b.p[k]
        assert b.orswot_sizes() == CRDT_EINVAL, name
        b = _Args()
        b.out.rm_ctr = b.p[k]
        assert b.orswot_write() == CRDT_EINVAL, name
    for name, k in dict(clock=20, n_keys=21, keys=22, eclock=23, key=4).items():
        b = _Args()
        b.sizes.rm_len = b.p[k]
        assert b.map_sizes() == CRDT_EINVAL, name
        b = _Args()
        b.out.list_key = b.p[k]
        assert b.map_write() == CRDT_EINVAL, name
    b = _Args()
    b.out.add_act = b.out.add_end  # the ends are inputs of the write call
    assert b.orswot_write() == CRDT_EINVAL
    assert a.mvreg_get(outs=(21, 12, 13)) == CRDT_EINVAL  # d_out_n == slab.n_keys
    assert a.mvreg_get(outs=(11, 12, 4)) == CRDT_EINVAL   # d_out_val == queries.key


def test_read_queries_pack_as_documented():
    import crdts_hip

    RQ = crdts_hip.ReadQueries
    per_obj = [[("key", 7), ("all",), ("key", (1 << 64) - 1, 3)], [], [("all", 5), ("key", 0, None)]]
    end, kind, key, actor = RQ.arrays_from_lists(per_obj)
    assert end.dtype == np.uint64 and end.tolist() == [3, 3, 5]
    assert kind.dtype == np.uint32 and kind.tolist() == [RQ.KEY, RQ.ALL, RQ.KEY, RQ.ALL, RQ.KEY]
    assert key.dtype == np.uint64 and key.tolist() == [7, 0, (1 << 64) - 1, 0, 0]
    assert actor.dtype == np.uint32 and actor.tolist() == [RQ.NO_ACTOR, RQ.NO_ACTOR, 3, 5, RQ.NO_ACTOR]
    assert RQ.arrays_from_lists([[("key", 1)], [("all",)]])[3] is None  # no query names an actor: a null array
    q = RQ.from_lists(per_obj, device=None)
    assert (q.n_obj, q.n_q) == (3, 5)
    c = q.cqueries()
    assert c.n_q == 5 and c.obj_end == q.t[0].data_ptr() and c.actor == q.t[3].data_ptr()
    assert q.t[2].numpy().view(np.uint64).tolist() == key.tolist()
    q = RQ.from_lists([[("key", 1)]], device=None)
    assert q.t[3] is None and q.cqueries().actor is None
    q = RQ.from_arrays([0, 0], [], [], device=None)  # objects without queries: null arrays, n_q 0
    assert q.n_q == 0 and q.cqueries().kind is None


class _RefBackend(read_ref.RefReadBackend, kat_runner.PyBackend):
    def _read(self, o, queries):
        return [read_ref.orswot_query(o, q, 16) for q in queries]


@pytest.mark.parametrize("case", kat_runner.load_cases(), ids=lambda c: c["name"])
def test_read_ref_reproduces_the_kats_ctx_asserts(case):
    b = _RefBackend()
    kat_runner.run_case(case, b)
    if any(st[0] in ("read", "contains") for st in case["steps"]):
        assert b.reads > 0


def test_read_ref_contexts():
    import crdts_ref

    o = crdts_ref.Orswot()
    o.apply_add((2, 1), 10)
    o.apply_add((5, (1 << 64) - 1), 30)
    o.apply_add((2, 2), 30)
    r = read_ref.orswot_query(o, ("key", 30, 2), 16)
    assert (r["val"], r["slot"], r["dot_ctr"]) == (1, 1, 3)
    assert r["rm"] == [(2, 2), (5, (1 << 64) - 1)] and r["add"] == [(2, 3), (5, (1 << 64) - 1)]
    r = read_ref.orswot_query(o, ("key", 11, 7), 16)  # absent, an actor new to the clock
    assert (r["val"], r["slot"], r["dot_ctr"], r["rm"]) == (0, read_ref.NO_SLOT, 1, [])
    assert r["add"] == [(2, 2), (5, (1 << 64) - 1), (7, 1)]
    r = read_ref.orswot_query(o, ("all", 5), 16)  # inc overflows: no dot, answered as without an actor
    assert r["err"] and r["dot_ctr"] == 0 and r["add"] == r["rm"] == [(2, 2), (5, (1 << 64) - 1)]
    assert r["val"] == 2 and r["list"] == [10, 30]
    assert read_ref.orswot_query(o, ("all", 16), 16)["err"]
