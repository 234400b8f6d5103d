"""GPU parity: the op path of VClock / GCounter / PNCounter through the C ABI
(clock_ops.hip) — apply, truncate, subtract, intersection, value and get, on
dense rows and on CSR runs — exactly equal to the oracle restatement
(oracle/crdts_ref.py VClock / GCounter / PNCounter driven by the same ops;
subtract and intersection also against oracle_ffi.vclock_binop): the
reference's subtract KATs and test_basic scripts on the device, every kernel
tier (16-byte and scalar dense paths, 1 to 64 lanes per row, register and
chunked CSR runs, register and chunked op lists), the u64 edges, the latched
errors, and the reference's properties (test/vclock.rs:46-66,
test/pncounter.rs:22-51) over random clocks."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import crdts_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U64 = (1 << 64) - 1
AMAX = (1 << 32) - 1
BINOPS = ("truncate", "subtract", "intersection")


def _kats():
    return json.load(open(os.path.join(GOLDEN, "kat_vclock_counters.json")))


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _rows(clocks, A):
    r = np.zeros((len(clocks), A), np.uint64)
    for i, c in enumerate(clocks):
        for a, v in dict(c).items():
            r[i, a] = v
    return r


def _ref(pairs):
    return crdts_ref.VClock(dict(pairs) if not isinstance(pairs, dict) else pairs)


def _ref_binop(op, a, b):
    """canonical() of a.op(b) by the oracle restatement."""
    v, o = _ref(a), _ref(b)
    if op == "intersection":
        return v.intersection(o).canonical()
    getattr(v, op)(o)
    return v.canonical()


def _row_clock(row):
    return {a: int(c) for a, c in enumerate(row.tolist()) if c}


def _csr_op(gpu, op, A, B, **kw):
    import crdts_hip

    S, O = crdts_hip.ClockBatch.from_lists(A), crdts_hip.ClockBatch.from_lists(B)
    return getattr(gpu, "clock_csr_" + op)(S, O, **kw)


# ------------------------------------------------------------------ KATs
def test_subtract_kats_dense_and_csr(gpu, oracle):
    kats = [k for k in _kats()["vclock_binop"] if k["op"] == "subtract"]
    assert [k["name"] for k in kats] == ["test_subtract", "prop_subtract_with_empty_is_nop (instance)",
                                         "prop_subtract_self_is_empty (instance)"]
    A = 10
    a, b = [dict(map(tuple, k["a"])) for k in kats], [dict(map(tuple, k["b"])) for k in kats]
    rows = _dev(_rows(a, A))
    gpu.dense_subtract(rows, _dev(_rows(b, A)), A)
    out = _csr_op(gpu, "subtract", a, b).clocks()
    for i, k in enumerate(kats):
        exp = [tuple(x) for x in k["expect"]]
        assert sorted(_row_clock(_u64(rows).reshape(-1, A)[i]).items()) == exp, k["name"]
        assert out[i] == exp, k["name"]
        assert oracle.vclock_binop("subtract", k["a"], k["b"]) == exp


def test_gcounter_basic_script(gpu):
    """test/gcounter.rs:4-19: each step is get -> + 1 -> apply -> value on the device."""
    import crdts_hip

    g = _kats()["gcounter_basic"]
    A = 2
    rows = _dev(np.zeros((2, A), np.uint64))  # row 0 = a, row 1 = b

    def step(obj, actor):
        q = crdts_hip.ClockOps.from_lists([[actor] if i == obj else [] for i in range(2)])
        inc = int(_u64(gpu.dense_get(rows, q, A))[0]) + 1  # GCounter::inc = VClock::inc, src/vclock.rs:182-185
        ops = crdts_hip.ClockOps.from_lists([[(actor, inc)] if i == obj else [] for i in range(2)])
        gpu.dense_apply(rows, ops, A, kind="gcounter")
        return _u64(gpu.gcounter_value(rows, A)).tolist()

    step(0, g["a_ops"][0])
    assert step(1, g["b_ops"][0]) == g["values_after_first"]
    assert step(0, g["a_ops"][1]) == [g["a_value_final"], g["b_value_final"]]


def test_pncounter_basic_script(gpu):
    """test/pncounter.rs:56-74 on a dense [P|N] row and on sparse P and N clocks."""
    import crdts_hip

    p = _kats()["pncounter_basic"]
    A, actor = 3, 0
    rows = _dev(np.zeros((1, 2 * A), np.uint64))
    SP, SN = crdts_hip.ClockBatch.from_lists([{}]), crdts_hip.ClockBatch.from_lists([{}])
    q = crdts_hip.ClockOps.from_lists([[actor]])
    for op, want in zip(p["ops"], p["values"]):
        d = 0 if op == "inc" else 1
        # dense: get reads one clock of the pair ([P|N]: a view of that half)
        half = rows.view(-1)[d * A:(d + 1) * A]
        dot = (actor, int(_u64(gpu.dense_get(half, q, A))[0]) + 1, d)
        gpu.dense_apply(rows, crdts_hip.ClockOps.from_lists([[dot]], with_dir=True), A, kind="pncounter")
        assert gpu.pncounter_value(rows, A).cpu().tolist() == [want]
        # sparse
        sdot = (actor, int(_u64(gpu.clock_csr_get(SN if d else SP, q))[0]) + 1, d)
        assert sdot == dot
        SP, SN = gpu.pncounter_csr_apply(SP, SN, crdts_hip.ClockOps.from_lists([[sdot]], with_dir=True))
        assert gpu.pncounter_csr_value(SP, SN).cpu().tolist() == [want]


# ---------------------------------------------------------------- dense binops
def _mixed_pair(rng, n, A):
    """Rows mixing 0, 1, equal counters, 2^64 - 1, and self below / equal / above other."""
    vals = np.array([0, 0, 1, 1, 2, 5, 1 << 40, 1 << 63, U64 - 1, U64], np.uint64)
    s = vals[rng.integers(0, len(vals), (n, A))]
    o = s.copy()
    m = rng.integers(0, 4, (n, A))
    o[m == 1] = vals[rng.integers(0, len(vals), (n, A))][m == 1]
    up = (m == 2) & (s < U64)
    o[up] = s[up] + np.uint64(1)
    down = (m == 3) & (s > 0)
    o[down] = s[down] - np.uint64(1)
    return s, o


def _np_binop(op, s, o):
    if op == "truncate":
        return np.minimum(s, o)
    if op == "subtract":
        return np.where(o >= s, np.uint64(0), s)
    return np.where(s == o, s, np.uint64(0))


@pytest.mark.parametrize("A", [1, 3, 16, 17, 64, 65, 300])
def test_dense_binops(gpu, oracle, A):
    import torch

    rng = np.random.default_rng(A)
    n = 139  # odd: the word count is odd for odd A (the scalar tail); > one block of 2048 words from A = 16
    s, o = _mixed_pair(rng, n, A)
    for op in BINOPS:
        exp = _np_binop(op, s, o)
        # the numpy form is the oracle's: checked row by row against crdts_ref, and (subtract /
        # intersection) against the C++ oracle
        for i in range(0, n, 1 if A <= 17 else 23):
            a, b = _row_clock(s[i]), _row_clock(o[i])
            assert tuple(sorted(_row_clock(exp[i]).items())) == _ref_binop(op, a, b)
            if op != "truncate" and i % 9 == 0:
                assert oracle.vclock_binop(op, sorted(a.items()), sorted(b.items())) == sorted(_row_clock(exp[i]).items())
        ds, do = _dev(s), _dev(o)
        getattr(gpu, "dense_" + op)(ds, do, A)
        assert (_u64(ds).reshape(n, A) == exp).all(), op
        assert (_u64(do).reshape(n, A) == o).all()  # other is read only
        # views offset by 8 bytes: the unaligned path (both sides, then one side only)
        for off_s, off_o in ((1, 1), (1, 0), (0, 1)):
            bs = torch.zeros(n * A + 2, dtype=torch.int64, device="cuda")
            bo = torch.zeros(n * A + 2, dtype=torch.int64, device="cuda")
            vs, vo = bs[off_s:off_s + n * A], bo[off_o:off_o + n * A]
            assert vs.data_ptr() % 16 == 8 * off_s and vo.data_ptr() % 16 == 8 * off_o
            vs.copy_(_dev(s).view(-1))
            vo.copy_(_dev(o).view(-1))
            getattr(gpu, "dense_" + op)(vs, vo, A)
            assert (_u64(vs).reshape(n, A) == exp).all(), (op, off_s, off_o)
            assert int(bs[0]) == 0 or off_s == 0
            assert int(bs[off_s + n * A]) == 0  # nothing past the rows is written
    gpu.status()


# ----------------------------------------------------------------- dense apply
def _apply_expect(rows, per_obj, A, pn):
    exp = rows.copy()
    for i, ops in enumerate(per_obj):
        if pn:
            c = crdts_ref.PNCounter()
            c.p.inner, c.n.inner = _ref(_row_clock(rows[i, :A])), _ref(_row_clock(rows[i, A:]))
            for a, v, d in ops:
                c.apply(((a, v), d == 0))
            exp[i] = np.concatenate([_rows([c.p.inner.dots], A)[0], _rows([c.n.inner.dots], A)[0]])
        else:
            c = _ref(_row_clock(rows[i]))
            for a, v in ops:
                c.apply((a, v))
            exp[i] = _rows([c.dots], A)[0]
    return exp


def _apply_cases(rng, A, pn):
    def dot(a=None, c=None):
        a = int(rng.integers(0, A)) if a is None else a
        c = (0, 1, 2, 7, 1 << 40, U64)[int(rng.integers(0, 6))] if c is None else c
        return (a, c, int(rng.integers(0, 2))) if pn else (a, c)

    inc = [dot(5 % A, c) for c in range(1, 65)]  # 64 dots on one (object, actor), distinct counters
    shuf = list(inc)
    random.Random(3).shuffle(shuf)
    per_obj = [[], [dot()], [dot() for _ in range(64)], [dot() for _ in range(65)], [dot() for _ in range(200)], [],
               inc, inc[::-1], shuf, [dot(0, 0), dot(A - 1, 0)],  # counter-0 dots
               [dot(2 % A, 9), dot(2 % A, 10), dot(2 % A, 11)]]  # below, equal to and above the stored 10
    per_obj += [[dot() for _ in range(int(rng.integers(0, 12)))] for _ in range(80)]  # a second chunk of objects
    if pn:  # both directions on the same actor
        per_obj[1] = [(1 % A, 4, 0), (1 % A, 6, 1), (1 % A, 5, 0), (1 % A, 2, 1)]
        per_obj[6] = [(a, c, 1) for a, c, _ in per_obj[6]]
        per_obj[7] = [(a, c, 0) for a, c, _ in per_obj[7]]
    return per_obj


@pytest.mark.parametrize("kind,A", [("vclock", 16), ("gcounter", 7), ("pncounter", 16), ("pncounter", 5)])
def test_dense_apply(gpu, kind, A):
    import crdts_hip

    pn = kind == "pncounter"
    rng = np.random.default_rng(A + pn)
    per_obj = _apply_cases(rng, A, pn)
    n, slots = len(per_obj), A * (2 if pn else 1)
    rows = np.where(rng.integers(0, 3, (n, slots)) == 0, 0, rng.integers(1, 1 << 41, (n, slots))).astype(np.uint64)
    rows[10, 2 % A] = 10
    if pn:
        rows[10, A + 2 % A] = 10
    d = _dev(rows)
    gpu.dense_apply(d, crdts_hip.ClockOps.from_lists(per_obj, with_dir=pn), A, kind=kind)
    got = _u64(d).reshape(n, slots)
    assert (got == _apply_expect(rows, per_obj, A, pn)).all()
    for i in (0, 5):  # rows of op-less objects are bit-identical
        assert (got[i] == rows[i]).all()
    assert got[6, (A if pn else 0) + 5 % A] == max(64, rows[6, (A if pn else 0) + 5 % A])  # the maximum wins


@pytest.mark.parametrize("kind", ["vclock", "pncounter"])
def test_dense_apply_latches_a_bad_op_and_skips_only_it(gpu, kind):
    import crdts_hip
    from crdts_hip._lib import CRDT_ENONCANON

    A, pn = 4, kind == "pncounter"
    slots = A * (2 if pn else 1)
    rows = np.arange(1, 3 * slots + 1, dtype=np.uint64).reshape(3, slots) * np.uint64(10)
    tail = (0,) if pn else ()
    # object 1: an actor equal to n_actors (PNCounter: that slot is the first N slot) between two good dots
    per_obj = [[(0, 500) + tail], [(1, 600) + tail, (A, 999) + tail, (2, 700) + tail], []]
    exp = rows.copy()
    exp[0, 0], exp[1, 1], exp[1, 2] = 500, 600, 700
    d = _dev(rows)
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.dense_apply(d, crdts_hip.ClockOps.from_lists(per_obj, with_dir=pn), A, kind=kind)
    assert e.value.code == CRDT_ENONCANON
    assert (_u64(d).reshape(3, slots) == exp).all()
    gpu.status()  # cleared
    if pn:  # a dir above 1
        d = _dev(rows)
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.dense_apply(d, crdts_hip.ClockOps.from_lists([[(0, 500, 0)], [(1, 600, 2), (2, 700, 1)], []],
                                                             with_dir=True), A, kind=kind)
        assert e.value.code == CRDT_ENONCANON
        exp = rows.copy()
        exp[0, 0], exp[1, A + 2] = 500, 700
        assert (_u64(d).reshape(3, slots) == exp).all()


def test_dense_apply_rejects_bad_obj_end(gpu):
    import crdts_hip
    from crdts_hip._lib import CRDT_ENONCANON

    A = 4
    rows = np.full((3, A), 10, np.uint64)
    # object 1's range decreases (object 2's own range, [1, 3), is well-formed); object 2's runs past n_ops
    for ends, touched in (([2, 1, 3], [0, 2]), ([1, 2, 9], [0, 1])):
        d = _dev(rows)
        ops = crdts_hip.ClockOps.from_arrays(ends, [0, 1, 2], [50, 60, 70])
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.dense_apply(d, ops, A)
        assert e.value.code == CRDT_ENONCANON
        got = _u64(d).reshape(3, A)
        # only well-formed ranges apply, each to its own object; nothing else changes
        exp = rows.copy()
        lo = 0
        for i, hi in enumerate(ends):
            if i in touched:
                for j in range(lo, hi):
                    exp[i, j] = 50 + 10 * j
            lo = hi
        assert (got == exp).all(), ends
        with pytest.raises(crdts_hip.CrdtError) as e:  # the get walks the same ranges
            gpu.dense_get(_dev(rows), ops, A)
        assert e.value.code == CRDT_ENONCANON


# ---------------------------------------------------------------------- values
def _i64(x):
    x &= U64
    return x - (1 << 64) if x >= 1 << 63 else x


@pytest.mark.parametrize("A", [1, 3, 16, 17, 64, 65, 300])
def test_values_and_get(gpu, A):
    import crdts_hip

    rng = np.random.default_rng(100 + A)
    n = 139
    rows, _ = _mixed_pair(rng, n, 2 * A)  # wrapping sums throughout
    rows[0] = 0
    d = _dev(rows)
    g = _u64(gpu.gcounter_value(d, 2 * A))
    assert g.tolist() == [sum(r) & U64 for r in rows.tolist()]
    gc = crdts_ref.GCounter()
    gc.inner = _ref(_row_clock(rows[1]))
    assert int(g[1]) == gc.value()
    gh = _u64(gpu.gcounter_value(d, A))  # the same buffer as 2n rows of A slots (odd A: rows 8-byte aligned only)
    assert gh.tolist() == [sum(r) & U64 for r in rows.reshape(2 * n, A).tolist()]
    p = gpu.pncounter_value(d, A).cpu().tolist()
    assert p == [_i64(_i64(sum(r[:A])) - _i64(sum(r[A:]))) for r in rows.tolist()]
    pc = crdts_ref.PNCounter()
    pc.p.inner, pc.n.inner = _ref(_row_clock(rows[2, :A])), _ref(_row_clock(rows[2, A:]))
    assert p[2] == pc.value()
    # a view offset by 8 bytes: even row widths leave the 16-byte-load form for the 8-byte one
    import torch

    buf = torch.zeros(n * 2 * A + 1, dtype=torch.int64, device="cuda")
    v = buf[1:]
    assert v.data_ptr() % 16 == 8
    v.copy_(d.view(-1))
    assert _u64(gpu.gcounter_value(v, 2 * A)).tolist() == g.tolist()
    assert _u64(gpu.gcounter_value(v, A)).tolist() == gh.tolist()
    assert gpu.pncounter_value(v, A).cpu().tolist() == p
    # get: every actor of a few rows, absent ones, and actors >= n_actors (0, not latched)
    qs = [[int(x) for x in rng.integers(0, 2 * A + 3, int(rng.integers(0, 9)))] for _ in range(n)]
    qs[3] = list(range(2 * A)) + [2 * A, AMAX]
    got = _u64(gpu.dense_get(d, crdts_hip.ClockOps.from_lists(qs), 2 * A)).tolist()
    assert got == [int(rows[i, a]) if a < 2 * A else 0 for i, q in enumerate(qs) for a in q]


def test_value_edges(gpu):
    rows = np.array([[U64, 2], [0, 0]], np.uint64)
    assert _u64(gpu.gcounter_value(_dev(rows), 2)).tolist() == [1, 0]  # [2^64 - 1, 2] sums to 1
    pn = np.array([[3, 0, 9, 1],            # 3 - 10: negative
                   [1 << 62, 1 << 62, 5, 0],  # P sum 2^63: wraps to i64::MIN, then - 5 wraps again
                   [U64, U64, 0, 0],          # P sum 2^65 - 2 -> -2
                   [0, 0, 0, 1 << 63]], np.uint64)
    got = gpu.pncounter_value(_dev(pn), 2).cpu().tolist()
    exp = []
    for r in pn.tolist():
        c = crdts_ref.PNCounter()
        c.p.inner, c.n.inner = _ref(_row_clock(np.array(r[:2], np.uint64))), _ref(_row_clock(np.array(r[2:], np.uint64)))
        exp.append(c.value())
    assert got == exp and exp[0] == -7 and exp[1] == (1 << 63) - 5 and exp[2] == -2


# ----------------------------------------------------------- CSR filters, apply
def _rnd_clock(rng, n, universe=100_000):
    return {int(x): int(rng.integers(1, 1 << 62)) for x in rng.choice(universe, n, replace=False)}


def _filter_batch(rng):
    lens = (0, 1, 63, 64, 65, 700)
    A, B = [], []
    for la in lens:
        for lb in lens:
            a, b = _rnd_clock(rng, la), _rnd_clock(rng, lb)
            ka = list(a)
            for j, k in enumerate(ka[: len(ka) // 2 + 1]):  # shared actors: equal, above, below
                if len(b) >= lb and lb:
                    b.pop(next(iter(b)))
                    b[k] = a[k] + (j % 3) - 1 or a[k]
            A.append(a)
            B.append(dict(sorted(b.items())))
    A += [{0: 1, AMAX: 2}, {0: 5, AMAX: U64}, {0: 3}, {AMAX: 1}]
    B += [{AMAX: 2}, {0: 5, AMAX: U64 - 1}, {0: 4, AMAX: 1}, {0: 1}]
    # equal actors straddling the 64-entry chunk boundary of both runs
    a = {k: k + 1 for k in range(1000, 1130)}
    A.append(a)
    B.append({k: (v if k % 2 else v + 1) for k, v in a.items() if 1050 <= k < 1080 or k >= 1120})
    return A, B


def test_csr_filters(gpu, oracle):
    A, B = _filter_batch(np.random.default_rng(5))
    for op in BINOPS:
        out = _csr_op(gpu, op, A, B)
        got = out.clocks()
        for i, (a, b) in enumerate(zip(A, B)):
            assert tuple(got[i]) == _ref_binop(op, a, b), (op, i, len(a), len(b))
            if op != "truncate" and len(a) + len(b) < 200:
                assert got[i] == oracle.vclock_binop(op, sorted(a.items()), sorted(b.items()))
        assert (out.to_host()[0] == np.cumsum([0] + [len(a) for a in A[:-1]])).all()  # out.off = self.off


def _apply_lists(rng):
    """(self clocks, op lists): 0 / 1 / 64 / 65 / 200 dots against runs of 0 / 1 / 63 / 64 / 65 / 700."""
    S, P = [], []
    for ns in (0, 1, 63, 64, 65, 700):
        for m in (0, 1, 64, 65, 200):
            s = _rnd_clock(rng, ns, universe=5000)
            keys = list(s)
            ops = []
            for _ in range(m):
                k = int(rng.integers(0, 4))
                if k == 0 and keys:  # a present actor: below / equal / above
                    a = keys[int(rng.integers(0, len(keys)))]
                    ops.append((a, max(0, s[a] + int(rng.integers(-1, 2)))))
                elif k == 1 and ops:  # a repeated actor
                    ops.append((ops[int(rng.integers(0, len(ops)))][0], int(rng.integers(0, 1 << 62))))
                else:
                    ops.append((int(rng.integers(0, 5200)), (0, 1, 9, 1 << 50, U64)[int(rng.integers(0, 5))]))
            S.append(s)
            P.append(ops)
    # counter-0 dots on an absent actor create no entry; actors below the first and above the last entry
    S += [{10: 1, 20: 2}, {10: 1, 20: 2}, {}, {5: 5}]
    P += [[(15, 0), (30, 0), (15, 0)], [(0, 7), (AMAX, 8), (9, 1), (21, 1)], [(3, 0)], [(5, 0), (5, 5), (5, 4)]]
    # 64 dots on one actor, the maximum in the middle; 130 dots over 3 actors (the chunked op path)
    S += [{7: 3}, {1: 1, 2: 50, 3: 1}]
    P += [[(7, c) for c in list(range(1, 40)) + [1000] + list(range(40, 64))],
          [(1 + j % 3, 1 + (j * 37) % 101) for j in range(130)]]
    return S, P


def _witnessed(s, ops):
    c = _ref(s)
    for d in ops:
        c.apply(d)
    return c.canonical()


def test_csr_apply_value_get(gpu):
    import crdts_hip

    rng = np.random.default_rng(9)
    S, P = _apply_lists(rng)
    SB = crdts_hip.ClockBatch.from_lists(S)
    for kind in ("vclock", "gcounter"):
        out = gpu.clock_csr_apply(SB, crdts_hip.ClockOps.from_lists(P), kind=kind)
        got = out.clocks()
        for i, (s, ops) in enumerate(zip(S, P)):
            assert tuple(got[i]) == _witnessed(s, ops), (i, len(s), len(ops))
        off = out.to_host()[0]
        before = np.cumsum([0] + [len(p) for p in P[:-1]])
        assert (off == SB.to_host()[0] + before.astype(np.uint64)).all()  # self.off[i] + obj_end[i-1]
    # value and get read the (gapped) apply output
    assert _u64(gpu.clock_csr_value(out)).tolist() == [sum(c for _, c in r) & U64 for r in got]
    qs = [[a for a, _ in r[:3]] + [min(a + 1, AMAX) for a, _ in r[-2:]] + [0, AMAX] for r in got]
    want = [dict(r).get(a, 0) for r, q in zip(got, qs) for a in q]
    assert _u64(gpu.clock_csr_get(out, crdts_hip.ClockOps.from_lists(qs))).tolist() == want
    # [2^64 - 1, 2] sums to 1
    assert _u64(gpu.clock_csr_value(crdts_hip.ClockBatch.from_lists([{1: U64, 9: 2}, {}]))).tolist() == [1, 0]


def test_csr_outputs_feed_back_as_gapped_inputs(gpu, oracle):
    import crdts_hip

    rng = np.random.default_rng(13)
    S, P = _apply_lists(rng)
    O = [_rnd_clock(rng, int(rng.choice([0, 3, 64, 90])), universe=5000) for _ in S]
    SB, OB = crdts_hip.ClockBatch.from_lists(S), crdts_hip.ClockBatch.from_lists(O)
    ops = crdts_hip.ClockOps.from_lists(P)
    applied = gpu.clock_csr_apply(SB, ops)  # gapped by the op counts
    filtered = gpu.clock_csr_subtract(applied, OB)  # gapped input -> gapped output
    e_applied = [dict(_witnessed(s, p)) for s, p in zip(S, P)]
    e_filtered = [dict(_ref_binop("subtract", a, o)) for a, o in zip(e_applied, O)]
    assert filtered.clocks() == [sorted(c.items()) for c in e_filtered]
    merged = gpu.clock_csr_merge(filtered, applied)  # both gapped, into the CSR merge
    e_merged = []
    for f, a in zip(e_filtered, e_applied):
        c = _ref(f)
        c.merge(_ref(a))
        e_merged.append(list(c.canonical()))
    assert merged.clocks() == e_merged
    again = gpu.clock_csr_apply(filtered, ops)  # a filter output into apply
    assert again.clocks() == [list(_witnessed(f, p)) for f, p in zip(e_filtered, P)]
    trunc = gpu.clock_csr_truncate(merged, again)  # a merge output and an apply output into a filter
    assert trunc.clocks() == [list(_ref_binop("truncate", dict(m), dict(a))) for m, a in zip(e_merged, again.clocks())]


@pytest.mark.parametrize("bad", ["zero", "unsorted", "misplaced"])
def test_csr_bad_runs_latch_and_write_no_length(gpu, bad):
    import crdts_hip
    from crdts_hip._lib import CRDT_EINVAL, CRDT_ENONCANON

    from test_oracle_csr import csr

    A = [{1: 1, 2: 2}, {1: 1, 2: 2, 3: 3}, {4: 4, 6: 6}]
    s = [x.copy() for x in csr(A)]
    if bad == "zero":
        s[3][3] = 0
    elif bad == "unsorted":
        s[2][[2, 3]] = s[2][[3, 2]]
    else:
        s[0][1] = 1  # object 1's run overlaps object 0's: object 0 is misplaced
    code = CRDT_EINVAL if bad == "misplaced" else CRDT_ENONCANON
    hit = 0 if bad == "misplaced" else 1
    S = crdts_hip.ClockBatch.from_host(*s)
    O = crdts_hip.ClockBatch.from_lists([{2: 2}, {9: 9}, {4: 4, 6: 1}])
    ops = crdts_hip.ClockOps.from_lists([[(7, 7)], [(8, 8)], []])
    # (object 2 keeps both entries under truncate and apply, (6, 6) under subtract, (4, 4) under intersection)
    for call, served in ((lambda: gpu.clock_csr_truncate(S, O, check_status=False), [(4, 4), (6, 1)]),
                         (lambda: gpu.clock_csr_subtract(S, O, check_status=False), [(6, 6)]),
                         (lambda: gpu.clock_csr_intersection(S, O, check_status=False), [(4, 4)]),
                         (lambda: gpu.clock_csr_apply(S, ops, check_status=False), [(4, 4), (6, 6)])):
        out = call()
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.status()
        assert e.value.code == code
        assert out.to_host()[1][hit] == 0
        assert out.clocks()[2] == served  # the other objects are served
    gpu.status()
    # a bad run on the `other` side of a filter
    out = gpu.clock_csr_subtract(O, S, check_status=False)
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == code and out.to_host()[1][hit] == 0


# ------------------------------------------------------------------ properties
def test_vclock_properties_on_the_kernels(gpu):
    """test/vclock.rs:46-66 over 2,000 random clocks, dense and sparse."""
    import torch

    import crdts_hip

    s, _ = crdts_hip.generate_clocks_csr(2000, seed=77)
    S = crdts_hip.ClockBatch.from_host(*s)
    E = crdts_hip.ClockBatch.from_lists([{} for _ in range(2000)])
    want = S.clocks()
    assert gpu.clock_csr_truncate(S, S).clocks() == want  # truncate by self is the identity
    assert gpu.clock_csr_subtract(S, E).clocks() == want  # subtract an empty clock is the identity
    assert gpu.clock_csr_subtract(S, S).clocks() == [[] for _ in want]  # subtract self is empty
    assert gpu.clock_csr_intersection(S, S).clocks() == want
    A = 19
    rows = crdts_hip.generate_dense(2000, A, seed=78)
    d = _dev(rows)
    t = d.clone()
    gpu.dense_truncate(t, d.clone(), A)
    assert torch.equal(t, d)
    gpu.dense_subtract(t, torch.zeros_like(d), A)
    assert torch.equal(t, d)
    gpu.dense_subtract(t, d, A)
    assert not t.any()


def test_pncounter_prop_merge_converges(gpu):
    """test/pncounter.rs:22-51: op vectors dealt to i witnesses by actor % i
    (i in 2..11), applied with crdt_pncounter_apply, folded with
    crdt_pncounter_merge and read with crdt_pncounter_value: one value per op
    vector, and it is the oracle's."""
    import crdts_hip

    rng = np.random.default_rng(51)
    A, n_vec = 24, 220
    vecs = [[(int(rng.integers(0, A)), int(rng.integers(0, 40)), int(rng.integers(0, 2)))
             for _ in range(int(rng.integers(0, 30)))] for _ in range(n_vec)]
    expect = []
    for v in vecs:  # the oracle: every op on one counter
        c = crdts_ref.PNCounter()
        for a, k, d in v:
            c.apply(((a, k), d == 0))
        expect.append(c.value())
    for i in range(2, 11):
        # witness w of vector j is object j * i + w
        per_obj = [[op for op in v if op[0] % i == w] for v in vecs for w in range(i)]
        rows = _dev(np.zeros((n_vec * i, 2 * A), np.uint64))
        gpu.dense_apply(rows, crdts_hip.ClockOps.from_lists(per_obj, with_dir=True), A, kind="pncounter")
        r = rows.view(n_vec, i, 2 * A)
        values = set()
        # every witness as the merge target: fold the others into a copy of it
        for w in (0, i - 1):
            acc = r[:, w].contiguous()
            for o in range(i):
                if o != w:
                    gpu.dense_merge(acc, r[:, o].contiguous(), A, "pncounter")
            values.add(tuple(gpu.pncounter_value(acc, A).cpu().tolist()))
        assert values == {tuple(expect)}, i
    gpu.status()


# ------------------------------------------------------------- argument checks
def test_argument_checks(gpu):
    import torch

    import crdts_hip
    from crdts_hip._lib import CRDT_ECAPACITY, CRDT_EINVAL, CRDT_OK, ClockCsrOut, lib

    ctx, st = gpu.ctx, gpu._stream()
    rows = _dev(np.full((2, 4), 7, np.uint64))
    other = _dev(np.full((2, 4), 3, np.uint64))
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    ops = crdts_hip.ClockOps.from_lists([[(0, 9)], [(1, 9)]], with_dir=False)
    c = ops.cops()
    P = lambda t: C.c_void_p(t.data_ptr())
    for fn in (lib.crdt_vclock_dense_apply, lib.crdt_gcounter_apply, lib.crdt_pncounter_apply):
        assert fn(None, P(rows), C.byref(c), 2, 4, st) == CRDT_EINVAL  # null ctx
        assert fn(ctx, None, C.byref(c), 2, 4, st) == CRDT_EINVAL  # null rows
        assert fn(ctx, P(rows), None, 2, 4, st) == CRDT_EINVAL  # null ops
        assert fn(ctx, P(rows), C.byref(c), 2, 0, st) == CRDT_EINVAL  # n_actors == 0
        assert fn(ctx, P(ops.t[2]), C.byref(c), 2, 4, st) == CRDT_EINVAL  # rows alias an op array
    assert lib.crdt_pncounter_apply(ctx, P(rows), C.byref(c), 2, 2, st) == CRDT_EINVAL  # ops without dir
    assert lib.crdt_vclock_dense_apply(ctx, None, C.byref(c), 0, 4, st) == CRDT_OK  # n_obj == 0
    for fn in (lib.crdt_vclock_dense_truncate, lib.crdt_vclock_dense_subtract, lib.crdt_vclock_dense_intersection):
        assert fn(None, P(rows), P(other), 2, 4, st) == CRDT_EINVAL
        assert fn(ctx, None, P(other), 2, 4, st) == CRDT_EINVAL
        assert fn(ctx, P(rows), None, 2, 4, st) == CRDT_EINVAL
        assert fn(ctx, P(rows), P(other), 2, 0, st) == CRDT_EINVAL
        assert fn(ctx, P(rows), P(rows), 2, 4, st) == CRDT_EINVAL  # in place on self only: other != self
        assert fn(ctx, None, None, 0, 4, st) == CRDT_OK
    for fn in (lib.crdt_gcounter_value, lib.crdt_pncounter_value):
        assert fn(None, P(rows), P(out), 2, 2, st) == CRDT_EINVAL
        assert fn(ctx, None, P(out), 2, 2, st) == CRDT_EINVAL
        assert fn(ctx, P(rows), None, 2, 2, st) == CRDT_EINVAL
        assert fn(ctx, P(rows), P(out), 2, 0, st) == CRDT_EINVAL
        assert fn(ctx, P(rows), P(rows), 2, 2, st) == CRDT_EINVAL
        assert fn(ctx, None, None, 0, 2, st) == CRDT_OK
    g = lib.crdt_vclock_dense_get
    assert g(None, P(rows), C.byref(c), P(out), 2, 4, st) == CRDT_EINVAL
    assert g(ctx, None, C.byref(c), P(out), 2, 4, st) == CRDT_EINVAL
    assert g(ctx, P(rows), None, P(out), 2, 4, st) == CRDT_EINVAL
    assert g(ctx, P(rows), C.byref(c), None, 2, 4, st) == CRDT_EINVAL
    assert g(ctx, P(rows), C.byref(c), P(out), 2, 0, st) == CRDT_EINVAL
    assert g(ctx, P(rows), C.byref(c), P(rows), 2, 4, st) == CRDT_EINVAL
    assert g(ctx, None, C.byref(c), None, 0, 4, st) == CRDT_OK
    # CSR
    S = crdts_hip.ClockBatch.from_lists([{1: 1}, {2: 2, 3: 3}])
    W = gpu._csr_out(2, 8)
    s = S.cstruct()
    w = ClockCsrOut(W.off.data_ptr(), W.len.data_ptr(), W.act.data_ptr(), W.ctr.data_ptr(), W.n_entries)
    small = ClockCsrOut(W.off.data_ptr(), W.len.data_ptr(), W.act.data_ptr(), W.ctr.data_ptr(), 2)
    alias = ClockCsrOut(W.off.data_ptr(), W.len.data_ptr(), S.act.data_ptr(), W.ctr.data_ptr(), W.n_entries)
    one = crdts_hip.ClockBatch.from_lists([{1: 1}]).cstruct()
    for fn in (lib.crdt_vclock_csr_truncate, lib.crdt_vclock_csr_subtract, lib.crdt_vclock_csr_intersection):
        assert fn(None, C.byref(s), C.byref(s), C.byref(w), st) == CRDT_EINVAL
        assert fn(ctx, None, C.byref(s), C.byref(w), st) == CRDT_EINVAL
        assert fn(ctx, C.byref(s), None, C.byref(w), st) == CRDT_EINVAL
        assert fn(ctx, C.byref(s), C.byref(s), None, st) == CRDT_EINVAL
        assert fn(ctx, C.byref(s), C.byref(one), C.byref(w), st) == CRDT_EINVAL  # n_obj differ
        assert fn(ctx, C.byref(s), C.byref(s), C.byref(alias), st) == CRDT_EINVAL  # out aliases an input
        assert fn(ctx, C.byref(s), C.byref(s), C.byref(small), st) == CRDT_ECAPACITY
    for fn in (lib.crdt_vclock_csr_apply, lib.crdt_gcounter_csr_apply):
        assert fn(None, C.byref(s), C.byref(c), C.byref(w), st) == CRDT_EINVAL
        assert fn(ctx, None, C.byref(c), C.byref(w), st) == CRDT_EINVAL
        assert fn(ctx, C.byref(s), None, C.byref(w), st) == CRDT_EINVAL
        assert fn(ctx, C.byref(s), C.byref(c), None, st) == CRDT_EINVAL
        assert fn(ctx, C.byref(s), C.byref(c), C.byref(alias), st) == CRDT_EINVAL
        assert fn(ctx, C.byref(s), C.byref(c), C.byref(small), st) == CRDT_ECAPACITY  # 3 entries + 2 ops
    assert lib.crdt_gcounter_csr_value(None, C.byref(s), P(out), st) == CRDT_EINVAL
    assert lib.crdt_gcounter_csr_value(ctx, None, P(out), st) == CRDT_EINVAL
    assert lib.crdt_gcounter_csr_value(ctx, C.byref(s), None, st) == CRDT_EINVAL
    assert lib.crdt_gcounter_csr_value(ctx, C.byref(s), P(S.ctr), st) == CRDT_EINVAL
    assert lib.crdt_vclock_csr_get(None, C.byref(s), C.byref(c), P(out), st) == CRDT_EINVAL
    assert lib.crdt_vclock_csr_get(ctx, None, C.byref(c), P(out), st) == CRDT_EINVAL
    assert lib.crdt_vclock_csr_get(ctx, C.byref(s), None, P(out), st) == CRDT_EINVAL
    assert lib.crdt_vclock_csr_get(ctx, C.byref(s), C.byref(c), None, st) == CRDT_EINVAL
    assert lib.crdt_vclock_csr_get(ctx, C.byref(s), C.byref(c), P(ops.t[1]), st) == CRDT_EINVAL
    # nothing ran: the inputs are untouched and nothing is latched
    gpu.status()
    assert (_u64(rows) == 7).all() and (_u64(other) == 3).all() and not out.any()
