"""GPU parity: the MVReg<u64, A> op path on device slabs — crdt_mvreg_apply
(Op::Put lists, src/mvreg.rs:158-186), crdt_mvreg_truncate (:100-113) and
crdt_mvreg_read_clock (:201-222), rust-crdt_amd/csrc/mvreg_apply.hip. Expected
values come from oracle/crdts_ref.py::MVReg over the same op lists, rendered
to the zero-filled slab (tests/mvreg_opgen.py); whole arrays are compared. The
reference's KATs and quickcheck properties (test/mvreg.rs) run with every
apply / merge / truncate / read on the kernels (the merge itself is
tests/test_gpu_mvreg_merge.py's); the error contract is the
header's (include/crdts_hip.h)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import mvreg_opgen as mo
from mvreg_opgen import crdts_ref

pytestmark = pytest.mark.gpu
PATTERN = 0x5A5A5A5A5A5A5A5A


def _dev(slab):
    import torch

    def put(t):
        t = np.ascontiguousarray(t)
        return torch.from_numpy(t.view(np.int32 if t.dtype == np.uint32 else np.int64)).to("cuda:0")

    return tuple(put(x) for x in slab)


def _host(slab):
    return (slab[0].cpu().numpy().view(np.uint32), slab[1].cpu().numpy().view(np.uint64),
            slab[2].cpu().numpy().view(np.uint64))


def _patterned(n, cap, A):
    """An output slab holding a pattern: the calls write every slot, zero fill included."""
    import torch

    return (torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"),
            torch.full((n, cap, A), PATTERN, dtype=torch.int64, device="cuda:0"),
            torch.full((n, cap), PATTERN, dtype=torch.int64, device="cuda:0"))


def _ops(per_obj):
    import crdts_hip

    return per_obj if isinstance(per_obj, crdts_hip.MVRegOps) else crdts_hip.MVRegOps.from_lists(per_obj)


def _apply(gpu, S, per_obj, A, out_cap, **kw):
    """S: a host or device slab -> the host output slab."""
    S = S if hasattr(S[0], "data_ptr") else _dev(S)
    return _host(gpu.mvreg_apply(S, _ops(per_obj), A, out=_patterned(int(S[0].numel()), out_cap, A), **kw))


def _assert_slab(got, exp, rows=None, what=""):
    n = len(exp[0])
    rows = np.arange(n) if rows is None else np.asarray(rows)
    for name, g, e in zip(("n", "clk", "val"), got, exp):
        d = (np.asarray(g) != np.asarray(e)).reshape(n, -1).any(axis=1)[rows]
        bad = rows[np.nonzero(d)[0]]
        assert bad.size == 0, f"{what} {name}: {bad.size} objects differ, first {bad[:5].tolist()}"


@functools.lru_cache(maxsize=None)
def _reference(seed, n, A, cap, hi, min_ops, max_ops):
    """(batch, S, E): the generated registers and op lists, the input slab and
    the restatement's output slab (out_cap = cap + 8) — computed once, never
    modified."""
    b = mo.gen_batch(seed, n, A, cap, hi, min_ops, max_ops)
    return b, mo.slab(b["regs0"], cap, A), mo.slab(b["regs"], cap + 8, A)


# ------------------------------------------------------------------ 1. KATs
class GpuBackend(mo.PyBackend):
    """A register is `reps` identical device registers; every apply is one
    crdt_mvreg_apply launch over them, every merge one crdt_mvreg_merge, every
    read one crdt_mvreg_read_clock. After every apply and merge the state must
    be the Python restatement's."""

    A, CAP = 8, 4

    def __init__(self, eng, reps):
        self.eng, self.reps = eng, reps

    def new(self):
        return dict(py=crdts_ref.MVReg(), slab=_dev(mo.slab([crdts_ref.MVReg()] * self.reps, self.CAP, self.A)))

    def apply(self, reg, op):
        out = self.eng.mvreg_apply(reg["slab"], _ops([[op]] * self.reps), self.A,
                                   out=_patterned(self.reps, self.CAP, self.A))
        mo.PyBackend.apply(self, reg["py"], op)
        _assert_slab(_host(out), mo.slab([reg["py"]] * self.reps, self.CAP, self.A), what=str(op))
        reg["slab"] = out

    def merge(self, reg, other):
        """One crdt_mvreg_merge launch over the copies (out_cap = CAP, below the capacities' sum)."""
        out = self.eng.mvreg_merge(reg["slab"], other["slab"], self.A, out=_patterned(self.reps, self.CAP, self.A))
        mo.PyBackend.merge(self, reg["py"], other["py"])
        _assert_slab(_host(out), mo.slab([reg["py"]] * self.reps, self.CAP, self.A), what="merge")
        reg["slab"] = out

    def read(self, reg):
        n, _, val = _host(reg["slab"])
        rc = self.eng.mvreg_read_clock(reg["slab"], self.A).cpu().numpy().view(np.uint64)
        assert (rc == rc[0]).all() and (n == n[0]).all() and (val == val[0]).all()
        return [int(v) for v in val[0, :n[0]]], [(a, int(c)) for a, c in enumerate(rc[0]) if c]

    def setlike(self, reg):
        s = mo.setlike(*_host(reg["slab"]))
        assert all(x == s[0] for x in s)
        return s[0]


KATS = mo.load_kats()


@pytest.mark.parametrize("reps", [1, 70])
@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_mvreg_op_kat_on_gpu(case, reps, gpu):
    applies = mo.run_kat(case, GpuBackend(gpu, reps))  # the reference's asserts, on kernel-made states
    assert applies == sum(st[0] == "apply" for st in case["steps"]) > 0


# ------------------------------------------------------- 2. random parity
@pytest.mark.parametrize("A,cap,hi", [(8, 4, 3), (16, 8, 2), (64, 3, 4), (5, 16, 2), (1, 4, 3)])
def test_mvreg_apply_parity(gpu, A, cap, hi):
    b, S, E = _reference(0xA000 + 100 * A + cap, 20_000, A, cap, hi, 0, 8)
    assert any(not ops for ops in b["ops"]) and (S[0] == 0).any()  # objects without ops; empty registers
    assert any(not ops and len(r.vals) for ops, r in zip(b["ops"], b["regs0"]))  # a non-empty copy-through
    assert len(set(E[0].tolist())) >= 4, set(E[0].tolist())
    # (64 actors at counters up to 4: no Put both drops a value and is dominated by another)
    assert all(b["classes"][c] > 0 for c in mo.CLASSES if A != 64 or c != "skip_drop"), b["classes"]
    _assert_slab(_apply(gpu, S, b["ops"], A, cap + 8), E)


@functools.lru_cache(maxsize=None)
def _cpp_reference(n, A, cap):
    """The parity check through the second restatement (oracle/ref_cpu.cpp):
    register i is the value of key 7 in a one-key OracleMap("mvreg"), every
    Put carried by an Op::Up whose dot is fresh (actor A, an actor of the Ups'
    own, counters 1, 2, ..), the nested register read back from .slab().
    0-4 Puts make the input registers, 0-8 more are the kernel's op lists.
    -> (ops, S, E, S_py, E_py): the slabs by the C++ oracle and by crdts_ref."""
    import oracle_ffi

    rng = random.Random(0xC99 + A)
    key, out_cap = 7, cap + 8

    def render(hs, mcap):
        cnt = np.zeros(n, np.uint32)
        clk = np.zeros((n, mcap, A), np.uint64)
        val = np.zeros((n, mcap), np.uint64)
        for i, h in enumerate(hs):
            M = h.slab(A + 1, dict(kcap=1, mcap=mcap, dcap=1, scap=1))
            if int(M.a["n_keys"][0]):
                assert int(M.a["keys"][0, 0]) == key and not M.a["mv_clock"][0, 0, :, A].any()
                cnt[i] = M.a["mv_n"][0, 0]
                clk[i] = M.a["mv_clock"][0, 0, :, :A]
                val[i] = M.a["mv_val"][0, 0]
        return cnt, clk, val

    hs, pys, ops, dots = [], [], [], []
    for i in range(n):
        h, r, d = oracle_ffi.OracleMap("mvreg"), crdts_ref.MVReg(), 0
        for t in range(rng.randint(0, cap)):
            c = mo.gen_op(rng, r, A, 3)
            d += 1
            h.apply_up_mvreg((A, d), key, mo.pairs_of(c), 1000 * i + t)
            r.apply_put(c, 1000 * i + t)
        hs.append(h)
        pys.append(r)
        dots.append(d)
    S, S_py = render(hs, cap), mo.slab(pys, cap, A)
    after = []
    for i, (h, r) in enumerate(zip(hs, pys)):
        r, lst = r.clone(), []
        for t in range(rng.randint(0, 8)):
            c = mo.gen_op(rng, r, A, 3)
            dots[i] += 1
            h.apply_up_mvreg((A, dots[i]), key, mo.pairs_of(c), 1000 * i + 500 + t)
            r.apply_put(c, 1000 * i + 500 + t)
            lst.append((mo.pairs_of(c), 1000 * i + 500 + t))
        ops.append(lst)
        after.append(r)
    return ops, S, render(hs, out_cap), S_py, mo.slab(after, out_cap, A)


def test_mvreg_apply_parity_cpp_oracle(gpu, oracle):
    """Whole-array equality with the C++ oracle's nested register (and the two
    restatements with each other), 3,000 registers at (A, cap) = (8, 4)."""
    A, cap = 8, 4
    ops, S, E, S_py, E_py = _cpp_reference(3000, A, cap)
    _assert_slab(S, S_py, what="input: C++ oracle vs crdts_ref")
    _assert_slab(E, E_py, what="output: C++ oracle vs crdts_ref")
    assert len(set(E[0].tolist())) >= 4 and (S[0] == 0).any() and any(not o for o in ops)
    _assert_slab(_apply(gpu, S, ops, A, cap + 8), E, what="kernel vs C++ oracle")


@pytest.mark.parametrize("A", [2, 3, 31, 33, 63, 65, 100, 128])
def test_mvreg_apply_actor_widths(gpu, A):
    """Actor counts around the lane mappings (a slot's elements within one
    step of 64 lanes, across two, across several)."""
    b, S, E = _reference(0xB000 + A, 2000, A, 3, 3, 0, 8)
    assert E[1][:, :, A - 1].any() and E[1][:, :, 0].any()
    _assert_slab(_apply(gpu, S, b["ops"], A, 3 + 8), E)


@pytest.mark.parametrize("A,cap,n", [(8, 100, 1000), (16, 300, 200), (512, 16, 500)])
def test_mvreg_apply_general_tier(gpu, A, cap, n):
    """Registers past the fast kernel's limits (more than 64 slots, or a block
    past its LDS: 24 slots x 512 actors = 96 KB) take the one-wave kernel."""
    b, S, E = _reference(0xC000 + A + cap, n, A, cap, 3 if A == 8 else 2, 6, 6)
    if cap > 64:
        assert E[0].max() > 64
    assert all(b["classes"][c] > 0 for c in ("add", "add_drop", "skip", "empty")), b["classes"]
    _assert_slab(_apply(gpu, S, b["ops"], A, cap + 8), E)


def test_mvreg_apply_chained_single_ops(gpu):
    """The same 8 ops as 8 single-op launches, each output the next input,
    equal one 8-op launch (and the restatement)."""
    A, cap = 8, 4
    b, S, E = _reference(0xD001, 1000, A, cap, 3, 8, 8)
    one = _apply(gpu, S, b["ops"], A, cap + 8)
    cur = _dev(S)
    for t in range(8):
        cur = gpu.mvreg_apply(cur, _ops([ops[t:t + 1] for ops in b["ops"]]), A,
                              out=_patterned(len(S[0]), cap + 8, A))
    _assert_slab(_host(cur), one, what="chained vs one launch")
    _assert_slab(one, E)


# ------------------------------------- 3. the reference's properties (test/mvreg.rs:145-320)
PA, PCAP, N_CASES = 9, 8, 2000


def _vectors(seed, pool=None):
    """N_CASES op vectors of 0-12 (val, actor) pairs; pool p: actors = p mod 3."""
    rng = random.Random(seed)
    actors = [a for a in range(PA) if pool is None or a % 3 == pool]
    return [[(rng.randrange(256), rng.choice(actors)) for _ in range(rng.randint(0, 12))] for _ in range(N_CASES)]


def _set_ops(gpu, slab, picks):
    """reg.set(val, reg.read().derive_add_ctx(actor)) per register, the read on
    the device: picks[i] = (val, actor) or None -> per-object op lists."""
    rc = gpu.mvreg_read_clock(slab, PA).cpu().numpy().view(np.uint64)
    step = []
    for i, p in enumerate(picks):
        if p is None:
            step.append([])
            continue
        row = rc[i].copy()
        row[p[1]] += 1  # derive_add_ctx: the read clock + inc(actor)
        step.append([([(a, int(c)) for a, c in enumerate(row) if c], p[0])])
    return step


def _build_test_regs(gpu, vecs):
    """build_test_reg (test/mvreg.rs:145-155), batched: -> (device slab, ops per case)."""
    slab = _dev(mo.slab([crdts_ref.MVReg()] * len(vecs), PCAP, PA))
    ops = [[] for _ in vecs]
    for t in range(max(len(v) for v in vecs)):
        step = _set_ops(gpu, slab, [v[t] if t < len(v) else None for v in vecs])
        for o, s in zip(ops, step):
            o.extend(s)
        slab = gpu.mvreg_apply(slab, _ops(step), PA, out=_patterned(len(vecs), PCAP, PA))
    return slab, ops


def _apply_dev(gpu, slab, ops):
    return gpu.mvreg_apply(slab, _ops(ops), PA, out=_patterned(int(slab[0].numel()), PCAP, PA))


def _not_compatible(opss):
    """ops_are_not_compatible, test/mvreg.rs:120-143."""
    for ai, a_ops in enumerate(opss):
        for bi, b_ops in enumerate(opss):
            if a_ops == b_ops:
                continue
            ac, bc = crdts_ref.VClock(), crdts_ref.VClock()
            for (_, aa), (_, ba) in zip(a_ops, b_ops):
                ac.apply(ac.inc(aa))
                bc.apply(bc.inc(ba))
                if bc.get(aa) == ac.get(aa):
                    return True
    return False


def test_prop_set_with_ctx_from_read(gpu):
    vecs = _vectors(0x51)
    slab, _ = _build_test_regs(gpu, vecs)
    rng = random.Random(0x52)
    n, _, val = _host(_apply_dev(gpu, slab, _set_ops(gpu, slab, [(23, rng.randrange(PA)) for _ in vecs])))
    assert (n == 1).all() and (val[:, 0] == 23).all() and (val[:, 1:] == 0).all()


def test_prop_truncate(gpu):
    import torch

    slab, _ = _build_test_regs(gpu, _vectors(0x53))
    snap = _host(slab)
    assert (snap[0] == 1).sum() > N_CASES // 2 and (snap[0] == 0).any()
    zero = torch.zeros((N_CASES, PA), dtype=torch.int64, device="cuda:0")
    same = _host(gpu.mvreg_truncate(slab, zero, PA, out=_patterned(N_CASES, PCAP, PA)))
    assert mo.setlike(*same) == mo.setlike(*snap)
    _assert_slab(same, snap)
    n, clk, val = _host(gpu.mvreg_truncate(slab, gpu.mvreg_read_clock(slab, PA), PA,
                                           out=_patterned(N_CASES, PCAP, PA)))
    assert (n == 0).all() and not clk.any() and not val.any()


def _merge_dev(gpu, a, b):
    """a.merge(&b) on the device, into a patterned slab of PCAP slots."""
    return gpu.mvreg_merge(a, b, PA, out=_patterned(int(a[0].numel()), PCAP, PA))


def test_prop_merge_idempotent(gpu):
    slab, _ = _build_test_regs(gpu, _vectors(0x5A))
    snap = _host(slab)
    assert (snap[0] == 1).sum() > N_CASES // 2 and (snap[0] == 0).any()
    again = _host(_merge_dev(gpu, slab, slab))
    assert mo.setlike(*again) == mo.setlike(*snap)
    _assert_slab(again, snap)


def test_prop_merge_commutative(gpu):
    v1, v2 = _vectors(0x5B, 0), _vectors(0x5C, 1)
    assert sum(_not_compatible([a, b]) for a, b in zip(v1, v2)) == 0  # no case is discarded
    (r1, _), (r2, _) = _build_test_regs(gpu, v1), _build_test_regs(gpu, v2)
    a = _host(_merge_dev(gpu, r1, r2))
    b = _host(_merge_dev(gpu, r2, r1))
    assert mo.setlike(*a) == mo.setlike(*b)
    assert (a[0] == 2).sum() > N_CASES // 2


def test_prop_merge_associative(gpu):
    v1, v2, v3 = _vectors(0x5D, 0), _vectors(0x5E, 1), _vectors(0x5F, 2)
    assert sum(_not_compatible([a, b, c]) for a, b, c in zip(v1, v2, v3)) == 0  # no case is discarded
    (r1, _), (r2, _), (r3, _) = (_build_test_regs(gpu, v) for v in (v1, v2, v3))
    a = _host(_merge_dev(gpu, _merge_dev(gpu, r1, r2), r3))  # (r1 ^ r2) ^ r3
    b = _host(_merge_dev(gpu, _merge_dev(gpu, r2, r3), r1))  # (r2 ^ r3) ^ r1
    assert mo.setlike(*a) == mo.setlike(*b)
    assert (a[0] == 3).sum() > N_CASES // 2


def test_prop_op_idempotent(gpu):
    slab, ops = _build_test_regs(gpu, _vectors(0x54))
    again = _host(_apply_dev(gpu, slab, ops))
    assert mo.setlike(*again) == mo.setlike(*_host(slab))


def test_prop_op_commutative(gpu):
    v1, v2 = _vectors(0x55, 0), _vectors(0x56, 1)
    assert sum(_not_compatible([a, b]) for a, b in zip(v1, v2)) == 0  # no case is discarded
    (r1, o1), (r2, o2) = _build_test_regs(gpu, v1), _build_test_regs(gpu, v2)
    a = _host(_apply_dev(gpu, r1, o2))
    b = _host(_apply_dev(gpu, r2, o1))
    assert mo.setlike(*a) == mo.setlike(*b)
    assert (a[0] == 2).sum() > N_CASES // 2


def test_prop_op_associative(gpu):
    v1, v2, v3 = _vectors(0x57, 0), _vectors(0x58, 1), _vectors(0x59, 2)
    assert sum(_not_compatible([a, b, c]) for a, b, c in zip(v1, v2, v3)) == 0  # no case is discarded
    (r1, o1), (r2, o2), (_, o3) = (_build_test_regs(gpu, v) for v in (v1, v2, v3))
    a = _host(_apply_dev(gpu, _apply_dev(gpu, r1, o2), o3))  # (r1 <- r2) <- r3
    b = _host(_apply_dev(gpu, _apply_dev(gpu, r2, o3), o1))  # (r2 <- r3) <- r1
    assert mo.setlike(*a) == mo.setlike(*b)
    assert (a[0] == 3).sum() > N_CASES // 2


# ------------------------------------------------- 4. truncate and read clock
SHAPES = [(8, 4, 3000), (16, 8, 3000), (100, 3, 2000), (16, 100, 300)]


@functools.lru_cache(maxsize=None)
def _truncate_reference(A, cap, n):
    """(S, T, E): registers of random rows, truncating clocks (30 % all zero,
    1 % the register's own read clock, the rest random rows) and the
    restatement's truncated registers."""
    rng = random.Random(0x7C00 + A + cap)
    regs = [mo.random_reg(rng, A, cap, 3, val0=1000 * i) for i in range(n)]
    T = np.zeros((n, A), np.uint64)
    out = []
    for i, r in enumerate(regs):
        u = rng.random()
        if u < 0.01:
            c = mo.fold(r)
        elif u < 0.31:
            c = crdts_ref.VClock()
        else:
            c = crdts_ref.VClock([(a, x) for a in range(A) for x in [rng.randrange(3)] if x])
        for a, x in c.dots.items():
            T[i, a] = x
        t = mo.regs_of(*mo.slab([r], cap, A))[0]  # rows as given
        t.truncate(c)
        out.append(t)
    return mo.slab(regs, cap, A), T, mo.slab(out, cap, A)


@pytest.mark.parametrize("A,cap,n", SHAPES)
def test_mvreg_truncate_parity(gpu, A, cap, n):
    S, T, E = _truncate_reference(A, cap, n)
    used = S[0] > 0
    unchanged = used & (E[0] == S[0]) & (E[1] == S[1]).reshape(n, -1).all(axis=1)
    emptied = used & (E[0] == 0)
    assert unchanged.any() and emptied.any() and (used & ~unchanged & ~emptied).any()
    got = _host(gpu.mvreg_truncate(_dev(S), _dev((T,))[0], A, out=_patterned(n, cap, A)))
    _assert_slab(got, E)
    # a wider output: zero-filled to out_cap
    got = _host(gpu.mvreg_truncate(_dev(S), _dev((T,))[0], A, out=_patterned(n, cap + 3, A)))
    assert (got[0] == E[0]).all() and (got[1][:, :cap] == E[1]).all() and (got[2][:, :cap] == E[2]).all()
    assert not got[1][:, cap:].any() and not got[2][:, cap:].any()


@pytest.mark.parametrize("A,cap,n", SHAPES)
def test_mvreg_read_clock_parity(gpu, A, cap, n):
    """The unused slots hold garbage: a kernel that reads past n[i] fails."""
    S, _, _ = _truncate_reference(A, cap, n)
    clk = S[1].copy()
    clk[np.arange(cap)[None, :] >= S[0][:, None]] = np.uint64(1 << 60)
    exp = np.where(np.arange(cap)[None, :, None] < S[0][:, None, None], S[1], 0).max(axis=1)
    assert (S[0] == 0).any() and (S[0] == cap).any()
    got = gpu.mvreg_read_clock(_dev((S[0], clk, S[2])), A).cpu().numpy().view(np.uint64)
    assert got.shape == (n, A) and (got == exp).all()


# ------------------------------------------------------------------ 5. errors
def _dot(a, c=1):
    return [(a, c)]


GOOD = [(_dot(0), 5), ([(0, 1), (1, 1)], 6)]


def _good_reg():
    r = crdts_ref.MVReg()
    r.apply_put(crdts_ref.VClock(_dot(2)), 4)
    return r


def _expect(regs, ops, cap, A):
    return mo.slab(mo.apply_ref(regs, ops), cap, A)


def _status_code(gpu):
    import crdts_hip

    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    gpu.status()  # the latch is cleared: the context is usable again
    return e.value.code


@pytest.mark.parametrize("A", [8, 2048], ids=["fast", "general"])
def test_mvreg_apply_capacity(gpu, A):
    """out_cap 4. A list that peaks at 5 slots latches CRDT_ECAPACITY, also one
    that ends within 4 but holds 5 mid-list; a Put that drops two values of a
    full register and appends one succeeds, with the kept rows moved down."""
    import crdts_hip

    cap, out_cap = 2, 4
    two = crdts_ref.MVReg()
    two.vals = [(crdts_ref.VClock(_dot(0)), 1), (crdts_ref.VClock(_dot(1)), 2)]
    regs = [_good_reg(), two, _good_reg(), crdts_ref.MVReg(), _good_reg()]
    fits = [GOOD,
            # full at 4 (slots 0..3), then a Put that drops slots 0 and 2 and is appended, then a fourth again
            [(_dot(2), 3), (_dot(3), 4), ([(0, 1), (2, 1), (4, 1)], 5), (_dot(5), 6)],
            [],
            # full at 4, then a Put that drops exactly one value and is appended: 4 - 1 + 1 = out_cap, judged
            # after the drop (4 + 1 before it would latch), the kept rows moved down for the append
            [(_dot(a), a) for a in range(4)] + [([(1, 1), (6, 1)], 7)], GOOD]
    E = _expect(regs, fits, out_cap, A)
    assert E[0].tolist() == [2, 4, 1, 4, 2] and E[2][1].tolist() == [2, 4, 5, 6] and E[2][3].tolist() == [0, 2, 3, 7]
    S = mo.slab(regs, cap, A)
    _assert_slab(_apply(gpu, S, fits, A, out_cap), E)  # clean status, every row exact
    five = [(_dot(a), a) for a in range(5)]
    # drop_then_overflow: the fifth Put's predecessor dropped one value of the full register (4 -> 4), so
    # only the count after that drop-then-append makes the next concurrent Put the overflowing one
    lists = (("peak_at_end", five, 5), ("peak_mid_list", five + [([(a, 1) for a in range(6)], 9)], 1),
             ("drop_then_overflow", fits[3] + [(_dot(5), 8)], 5))
    for name, lst, final in lists:
        ops = list(fits)
        ops[3] = lst
        assert len(mo.apply_ref([regs[3]], [lst])[0].vals) == final
        with pytest.raises(crdts_hip.CrdtError) as e:
            _apply(gpu, S, ops, A, out_cap)
        assert e.value.code == crdts_hip.CRDT_ECAPACITY, name
        got = _apply(gpu, S, ops, A, out_cap, check_status=False)
        assert _status_code(gpu) == crdts_hip.CRDT_ECAPACITY
        _assert_slab(got, E, rows=[0, 1, 2, 4], what=name)


POISON = 0xBAD0BAD0


def _raw_ops(per_obj, tail=0, **patch):
    """MVRegOps from lists, not validated, with arrays patched; `tail` poisoned
    ops (values and counters POISON) follow the arrays, past n_ops / n_clk."""
    import crdts_hip

    arrs = dict(obj_end=[], val=[], clk_end=[], clk_act=[], clk_ctr=[])
    for ops in per_obj:
        for pairs, v in ops:
            for a, c in pairs:
                arrs["clk_act"].append(a)
                arrs["clk_ctr"].append(c)
            arrs["clk_end"].append(len(arrs["clk_act"]))
            arrs["val"].append(v)
        arrs["obj_end"].append(len(arrs["val"]))
    arrs.update(patch)
    arrs = {k: np.asarray(v, dtype=np.uint32 if k == "clk_act" else np.uint64) for k, v in arrs.items()}
    n_ops, n_clk = len(arrs["val"]), len(arrs["clk_act"])
    if tail:
        arrs["val"] = np.concatenate([arrs["val"], np.full(tail, POISON, np.uint64)])
        arrs["clk_end"] = np.concatenate([arrs["clk_end"], n_clk + 1 + np.arange(tail, dtype=np.uint64)])
        arrs["clk_act"] = np.concatenate([arrs["clk_act"], np.full(tail, 3, np.uint32)])
        arrs["clk_ctr"] = np.concatenate([arrs["clk_ctr"], np.full(tail, POISON, np.uint64)])
    ops = crdts_hip.MVRegOps.from_arrays(*(arrs[k] for k in ("obj_end", "val", "clk_end", "clk_act", "clk_ctr")))
    ops.n_ops, ops.n_clk = n_ops, n_clk  # the tail is past the counts the call is given
    return ops


# three objects of GOOD: obj_end [2, 4, 6], clk_end [1, 3, 4, 6, 7, 9]
NONCANON = {
    # name: (ops builder, rows that must still be exact)
    "descending_clock_actors": (lambda A: _raw_ops([GOOD, [([(2, 1), (1, 1)], 9)], GOOD]), [0, 2]),
    "equal_clock_actors": (lambda A: _raw_ops([GOOD, [([(2, 1), (2, 2)], 9)], GOOD]), [0, 2]),
    "zero_counter": (lambda A: _raw_ops([GOOD, [([(1, 0)], 9)], GOOD]), [0, 2]),
    "clock_actor_out_of_range": (lambda A: _raw_ops([GOOD, [([(A, 1)], 9)], GOOD]), [0, 2]),
    "second_op_bad": (lambda A: _raw_ops([GOOD, [(_dot(1), 8), ([(1, 1), (A + 7, 1)], 9)], GOOD]), [0, 2]),
    "decreasing_obj_end": (lambda A: _raw_ops([GOOD, GOOD, GOOD], obj_end=[2, 1, 6]), [0]),
    "obj_end_past_n_ops": (lambda A: _raw_ops([GOOD, GOOD, GOOD], tail=16, obj_end=[2, 11, 6]), [0]),
    "decreasing_clk_end": (lambda A: _raw_ops([GOOD, GOOD, GOOD], clk_end=[1, 3, 4, 3, 7, 9]), [0]),
    "clk_end_past_n_clk": (lambda A: _raw_ops([GOOD, GOOD, GOOD], tail=16, clk_end=[1, 3, 4, 14, 7, 9]), [0]),
}


@pytest.mark.parametrize("A", [8, 2048], ids=["fast", "general"])
@pytest.mark.parametrize("name", sorted(NONCANON))
def test_mvreg_apply_noncanonical_ops(gpu, name, A):
    """A malformed op list latches CRDT_ENONCANON for its object; its
    neighbours whose lists are well formed are exact; nothing past n_ops /
    n_clk is read (the poisoned tail shows in no output)."""
    import crdts_hip

    build, rows = NONCANON[name]
    regs = [_good_reg(), _good_reg(), _good_reg()]
    E = _expect(regs, [GOOD, [], GOOD], 4, A)
    got = _apply(gpu, mo.slab(regs, 2, A), build(A), A, 4, check_status=False)
    assert _status_code(gpu) == crdts_hip.CRDT_ENONCANON
    _assert_slab(got, E, rows=rows, what=name)
    assert not (got[1] == POISON).any() and not (got[2] == POISON).any()


def test_mvreg_noncanonical_slot_count(gpu):
    """n[i] > cap: CRDT_ENONCANON from all three calls, neighbours intact."""
    import crdts_hip
    import torch

    A = 8
    regs = [_good_reg(), _good_reg(), _good_reg()]
    S = list(mo.slab(regs, 2, A))
    S[0] = S[0].copy()
    S[0][1] = 3
    got = _apply(gpu, tuple(S), [GOOD, [], GOOD], A, 4, check_status=False)
    assert _status_code(gpu) == crdts_hip.CRDT_ENONCANON
    _assert_slab(got, _expect(regs, [GOOD, [], GOOD], 4, A), rows=[0, 2])
    zero = torch.zeros((3, A), dtype=torch.int64, device="cuda:0")
    got = _host(gpu.mvreg_truncate(_dev(tuple(S)), zero, A, out=_patterned(3, 2, A), check_status=False))
    assert _status_code(gpu) == crdts_hip.CRDT_ENONCANON
    _assert_slab(got, mo.slab(regs, 2, A), rows=[0, 2])
    rc = gpu.mvreg_read_clock(_dev(tuple(S)), A, check_status=False).cpu().numpy().view(np.uint64)
    assert _status_code(gpu) == crdts_hip.CRDT_ENONCANON
    assert rc[0].tolist() == rc[2].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]


def test_mvreg_ops_einval(gpu):
    """The CRDT_EINVAL table of include/crdts_hip.h, before any device work."""
    import crdts_hip
    import torch
    from crdts_hip._lib import lib

    A, cap, ocap, n = 8, 2, 4, 3
    sn, sc, sv = _dev(mo.slab([_good_reg()] * n, cap, A))
    on, oc, ov = _patterned(n, ocap, A)
    clock = torch.zeros((n, A), dtype=torch.int64, device="cuda:0")
    ops = _ops([GOOD] * n)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def apply(ctx=gpu.ctx, s=(sn, sc, sv), scap=cap, o=ops.cops(), out=(on, oc, ov), ocap_=ocap, n_=n, A_=A):
        return lib.crdt_mvreg_apply(ctx, p(s[0]), p(s[1]), p(s[2]), scap, C.byref(o) if o is not None else None,
                                    p(out[0]), p(out[1]), p(out[2]), ocap_, n_, A_, None)

    def trunc(ctx=gpu.ctx, s=(sn, sc, sv), scap=cap, c=clock, out=(on, oc, ov), ocap_=ocap, n_=n, A_=A):
        return lib.crdt_mvreg_truncate(ctx, p(s[0]), p(s[1]), p(s[2]), scap, p(c), p(out[0]), p(out[1]), p(out[2]),
                                       ocap_, n_, A_, None)

    def read(ctx=gpu.ctx, s=(sn, sc), cap_=cap, out=clock, n_=n, A_=A):
        return lib.crdt_mvreg_read_clock(ctx, p(s[0]), p(s[1]), cap_, p(out), n_, A_, None)

    def patched(**kw):
        o = ops.cops()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    bad = [apply(ctx=None), apply(o=None), apply(o=None, n_=0), apply(A_=0), apply(scap=0), apply(scap=1025, ocap_=2048),
           apply(ocap_=cap - 1), apply(ocap_=2049), apply(s=(None, sc, sv)), apply(s=(sn, None, sv)),
           apply(s=(sn, sc, None)), apply(out=(None, oc, ov)), apply(out=(on, None, ov)), apply(out=(on, oc, None)),
           apply(o=patched(obj_end=None)), apply(o=patched(val=None)), apply(o=patched(clk_end=None)),
           apply(o=patched(clk_act=None)), apply(o=patched(clk_ctr=None)),
           apply(out=(sn, oc, ov)), apply(out=(on, sc, ov), ocap_=cap), apply(out=(on, oc, sv), ocap_=cap),
           trunc(ctx=None), trunc(A_=0), trunc(scap=0), trunc(scap=1025, ocap_=2048), trunc(ocap_=cap - 1),
           trunc(ocap_=2049), trunc(s=(None, sc, sv)), trunc(s=(sn, None, sv)), trunc(s=(sn, sc, None)),
           trunc(c=None), trunc(out=(None, oc, ov)), trunc(out=(on, None, ov)), trunc(out=(on, oc, None)),
           trunc(out=(sn, oc, ov)), trunc(out=(on, sc, ov), ocap_=cap), trunc(out=(on, oc, sv), ocap_=cap),
           read(ctx=None), read(A_=0), read(cap_=0), read(s=(None, sc)), read(s=(sn, None)), read(out=None),
           read(out=sc)]
    assert bad == [crdts_hip.CRDT_EINVAL] * len(bad), bad
    assert apply() == trunc() == read() == crdts_hip.CRDT_OK
    gpu.status()
    assert (on.cpu().numpy() != 0x5A5A5A5A).all()


def test_mvreg_read_clock_any_cap(gpu):
    """crdt_mvreg_read_clock has no upper limit on cap (the other two calls' outputs go up to 2 048)."""
    A, cap = 3, 2100
    cnt = np.array([cap, 5, 0], np.uint32)
    clk = np.random.default_rng(7).integers(0, 1 << 40, (3, cap, A)).astype(np.uint64)
    exp = np.where(np.arange(cap)[None, :, None] < cnt[:, None, None], clk, 0).max(axis=1)
    got = gpu.mvreg_read_clock(_dev((cnt, clk)), A).cpu().numpy().view(np.uint64)
    assert (got == exp).all() and got[0].all()


def test_mvreg_ops_records_longest_list(gpu):
    """MVRegOps packed from host arrays knows its longest list: the default
    output size of Engine.mvreg_apply needs no copy back from the device."""
    import crdts_hip

    ops = _ops([GOOD, [], GOOD + GOOD[:1]])
    assert ops.max_ops == 3
    regs = [_good_reg(), _good_reg(), _good_reg()]
    out = gpu.mvreg_apply(_dev(mo.slab(regs, 2, 8)), ops, 8)
    assert tuple(out[1].shape) == (3, 2 + 3, 8)
    _assert_slab(_host(out), _expect(regs, [GOOD, [], GOOD + GOOD[:1]], 5, 8))
    raw = crdts_hip.MVRegOps(*ops.t)  # built from device tensors: the size comes from obj_end
    assert raw.max_ops is None and tuple(gpu.mvreg_apply(_dev(mo.slab(regs, 2, 8)), raw, 8)[1].shape) == (3, 5, 8)


def test_mvreg_ops_no_objects(gpu):
    """n_obj == 0 is CRDT_OK, null arrays included."""
    import crdts_hip
    from crdts_hip._lib import MVRegOpsC, lib

    o = MVRegOpsC(None, None, None, None, None, 0, 0)
    assert lib.crdt_mvreg_apply(gpu.ctx, None, None, None, 2, C.byref(o), None, None, None, 4, 0, 8, None) == 0
    # (the ops struct itself is always read: null is CRDT_EINVAL also without objects)
    assert lib.crdt_mvreg_apply(gpu.ctx, None, None, None, 2, None, None, None, None, 4, 0, 8, None) == crdts_hip.CRDT_EINVAL
    assert lib.crdt_mvreg_truncate(gpu.ctx, None, None, None, 2, None, None, None, None, 4, 0, 8, None) == 0
    assert lib.crdt_mvreg_read_clock(gpu.ctx, None, None, 2, None, 0, 8, None) == 0
    Z = _dev(mo.slab([], 2, 8))
    out = gpu.mvreg_apply(Z, crdts_hip.MVRegOps.from_lists([]), 8, out_cap=4)
    assert out[0].numel() == 0 and tuple(out[1].shape) == (0, 4, 8)
    assert gpu.mvreg_read_clock(Z, 8).shape == (0, 8)
    gpu.status()
    # n_ops == 0 with objects: null op arrays, every register copied through and zero-filled
    regs = [_good_reg(), crdts_ref.MVReg(), _good_reg()]
    none = crdts_hip.MVRegOps.from_lists([[], [], []])
    assert none.n_ops == 0 and none.cops().val is None and none.cops().clk_act is None
    _assert_slab(_apply(gpu, mo.slab(regs, 2, 8), none, 8, 4), mo.slab(regs, 4, 8))
