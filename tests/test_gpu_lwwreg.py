"""GPU: the batched LWWReg calls (crdt_lwwreg_merge / _apply / _fold /
_from_bincode / _to_bincode) against the sequential restatement of
src/lwwreg.rs in tests/lwwreg_ref.py, exactly."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import lwwreg_cases as cases
import lwwreg_ref as ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 64) - 1


def _kats():
    with open(os.path.join(REPO, "tests", "golden", "kat_lwwreg.json")) as f:
        return json.load(f)


def _r(d):
    return (d["val"], d["marker"])


def _batch(regs, mw, misalign=False):
    """Device batch; misalign: both arrays start 8 bytes past a 16-byte boundary."""
    import crdts_hip
    import torch

    B = crdts_hip.LWWBatch.from_lists(regs, marker_words=mw)
    if not misalign:
        return B
    n = B.n
    v = torch.zeros(n + 1, dtype=torch.int64, device=B.val.device)
    m = torch.zeros(n * mw + 1, dtype=torch.int64, device=B.val.device)
    v[1:] = B.val
    m[1:] = B.marker.reshape(-1)
    out = crdts_hip.LWWBatch(v[1:], m[1:].view(n, mw))
    assert out.val.data_ptr() % 16 == 8 and out.marker.data_ptr() % 16 == 8
    return out


def _bits(bitmap, n):
    w = bitmap.cpu().numpy().view(np.uint64)
    return [bool((int(w[i // 64]) >> (i % 64)) & 1) for i in range(n)], w


def _pairs(seed, n, mw):
    rng = random.Random(seed)
    return [cases.rnd_reg(rng, mw) for _ in range(n)], [cases.rnd_reg(rng, mw) for _ in range(n)]


def _check_merge(gpu, s, o, mw, misalign=False):
    import torch

    n = len(s)
    exp = [ref.merge(a, b) for a, b in zip(s, o)]
    S, O = _batch(s, mw, misalign), _batch(o, mw, misalign)
    # every word of the bitmap and the count must be written: start them dirty
    bitmap = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    count = torch.full((1,), 12345 if n else 0, dtype=torch.int64, device="cuda")  # (n == 0 writes nothing)
    gpu.lwwreg_merge(S, O, bitmap=bitmap, count=count)
    gpu.status()  # conflicts are results: nothing is latched
    assert S.to_lists() == [e[0] for e in exp]
    assert O.to_lists() == o  # other is only read
    got, words = _bits(bitmap, n)
    assert got == [e[1] for e in exp]
    if n % 64:
        assert int(words[-1]) >> (n % 64) == 0  # tail bits zero
    assert int(count.item()) == sum(e[1] for e in exp)
    # both outputs null: the same state
    S2 = _batch(s, mw, misalign)
    assert gpu.lwwreg_merge(S2, O, want_bitmap=False, want_count=False) == (None, None)
    assert S2.to_lists() == [e[0] for e in exp]
    return exp


# ----------------------------------------------------------------------- KATs
def test_kats_on_the_device(gpu):
    import crdts_hip

    k = _kats()
    for name, want in (("test_update", [0, 0, 0, 1]), ("update_doctest", [0, 1, 0, 0])):
        script = k[name]
        assert [0 if st["ok"] else 1 for st in script["steps"]] == want
        ops = [_r(st["update"]) for st in script["steps"]]
        S = _batch([_r(script["start"])], 1)
        n_err, op_err = gpu.lwwreg_apply(S, crdts_hip.LWWOps.from_lists([ops]), want_op_err=True)
        assert S.to_lists() == [_r(script["steps"][-1]["state"])]
        assert op_err.cpu().tolist() == want and n_err.cpu().tolist() == [sum(want)]
        # and step by step, each op as a merge
        S = _batch([_r(script["start"])], 1)
        for st in script["steps"]:
            bitmap, count = gpu.lwwreg_merge(S, _batch([_r(st["update"])], 1))
            assert S.to_lists() == [_r(st["state"])]
            assert (int(bitmap.item()), int(count.item())) == ((0, 0) if st["ok"] else (1, 1))
    m = k["merge_doctest"]
    S = _batch([_r(m["self"])], 1)
    bitmap, count = gpu.lwwreg_merge(S, _batch([_r(m["other"])], 1))
    assert S.to_lists() == [_r(m["state"])] and int(bitmap.item()) == 1 and int(count.item()) == 1
    D = _batch([_r(k["test_default"])], 1)
    gpu.lwwreg_merge(D, _batch([ref.default()], 1))
    assert D.to_lists() == [(0, 0)]


# ---------------------------------------------------------------------- merge
@pytest.mark.parametrize("mw", [1, 2])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 127, 128, 129, 257, 70_001])
def test_merge_parity(gpu, n, mw):
    s, o = _pairs(0x3E46E + n, n, mw)
    exp = _check_merge(gpu, s, o, mw)
    if n >= 63:  # the alphabets make every outcome frequent
        assert any(e[1] for e in exp) and any(e[0] != a for e, a in zip(exp, s))
        assert any(a == b for a, b in zip(s, o))  # equal marker and value: an Ok no-op


@pytest.mark.parametrize("mw", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 65, 129])
def test_merge_parity_on_unaligned_arrays(gpu, n, mw):
    s, o = _pairs(0xA11 + n, n, mw)
    _check_merge(gpu, s, o, mw, misalign=True)


def test_merge_marker_order_edges(gpu):
    # one word: 0, 2^32 and 2^64 - 1 against each other (an unsigned 64-bit compare)
    edge = [0, 1 << 32, BIG, (1 << 63), (1 << 32) - 1]
    s = [(7, a) for a in edge for _ in edge]
    o = [(8, b) for _ in edge for b in edge]
    _check_merge(gpu, s, o, 1)
    # two words: differing in word 1 only; word 0 deciding against word 1
    pairs = [((5, 5), (5, 6)), ((5, 6), (5, 5)), ((1, BIG), (2, 0)), ((2, 0), (1, BIG)), ((0, 1 << 32), (1 << 32, 0)),
             ((BIG, 0), (BIG, BIG)), ((3, 3), (3, 3))]
    s2 = [(7, a) for a, _ in pairs]
    o2 = [(8, b) for _, b in pairs]
    exp = _check_merge(gpu, s2, o2, 2)
    assert [e[0][0] for e in exp] == [8, 7, 8, 7, 8, 8, 7] and [e[1] for e in exp] == [False] * 6 + [True]


@pytest.mark.parametrize("mw", [1, 2])
def test_a_batch_of_conflicts_leaves_the_status_ok(gpu, mw):
    from crdts_hip._lib import lib

    n = 300
    m = (3, 4)[:mw] if mw == 2 else 3
    s, o = [(7, m)] * n, [(8, m)] * n
    exp = _check_merge(gpu, s, o, mw)
    assert all(e[1] for e in exp)
    assert lib.crdt_ctx_status(gpu.ctx, None) == 0


# ---------------------------------------------------------------------- apply
def _apply_lists(mw):
    import crdts_hip

    B = crdts_hip.LWWREG_WAVE_MIN_OPS
    lengths = [0, 1, 2, B - 1, B, B + 1, 63, 64, 65, 129, 300]
    rng = random.Random(0xA991 + mw)
    ms = cases.markers(mw)
    lo, hi = ms[1], ms[2]
    batch = []
    # the largest marker first appears in a later 64-op chunk, then repeats with another value
    batch.append(((7, ms[0]), [(7, lo)] * 70 + [(8, hi), (7, hi), (8, hi)] + [(7, lo)] * 55 + [(7, hi)]))
    # every op repeats the register's own marker, values alternating
    batch.append(((7, lo), [(8, lo), (7, lo)] * 50))
    batch.append(((7, lo), [(8, lo), (7, lo)] * 5))
    # duplicates only
    batch.append(((7, hi), [(7, hi)] * 65))
    batch.append(((7, hi), [(7, hi)] * 3))
    while len(batch) < 2000:
        ln = lengths[len(batch) % len(lengths)] if rng.random() < 0.85 else rng.randrange(0, 8)
        batch.append((cases.rnd_reg(rng, mw), [cases.rnd_reg(rng, mw) for _ in range(ln)]))
    rng.shuffle(batch)
    lens = {len(ops) for _, ops in batch}
    assert set(lengths) <= lens
    assert any(x < B for x in lens) and any(x >= B for x in lens)  # both tiers are reached
    return batch


@pytest.fixture(scope="module", params=[1, 2])
def apply_case(request):
    mw = request.param
    batch = _apply_lists(mw)
    return mw, batch, [ref.apply_list(s, ops) for s, ops in batch]


def test_apply_parity(gpu, apply_case):
    import crdts_hip

    mw, batch, exp = apply_case
    S = _batch([s for s, _ in batch], mw)
    ops = crdts_hip.LWWOps.from_lists([o for _, o in batch], marker_words=mw)
    n_err, op_err = gpu.lwwreg_apply(S, ops, want_op_err=True)
    assert S.to_lists() == [e[0] for e in exp]
    assert n_err.cpu().tolist() == [sum(e[1]) for e in exp]
    assert op_err.cpu().tolist() == [int(x) for e in exp for x in e[1]]
    assert sum(sum(e[1]) for e in exp) > 100
    # the per-op bytes are optional
    S2 = _batch([s for s, _ in batch], mw)
    assert gpu.lwwreg_apply(S2, ops).cpu().tolist() == [sum(e[1]) for e in exp]
    assert S2.to_lists() == [e[0] for e in exp]
    # the closed form agrees with what the device did
    assert all(cases.closed_form(s, o) == e for (s, o), e in zip(batch[:200], exp[:200]))


@pytest.mark.parametrize("mw", [1, 2])
def test_apply_rejects_bad_obj_end_and_spares_the_neighbours(gpu, mw):
    import crdts_hip
    from crdts_hip._lib import CRDT_ENONCANON

    ms = cases.markers(mw)
    start = [(7, ms[0]), (7, ms[1]), (7, ms[0])]
    ops = [(8, ms[1]), (8, ms[2]), (9, ms[2])]
    # object 1's range decreases (object 2's own range, [1, 3), is well-formed); object 2's runs past n_ops
    for ends, good in (([2, 1, 3], [0, 2]), ([1, 2, 9], [0, 1])):
        S = _batch(start, mw)
        val, mk = np.array([v for v, _ in ops], np.uint64), np.array([m for _, m in ops], np.uint64)
        P = crdts_hip.LWWOps.from_arrays(ends, val, mk)
        n_err, op_err = gpu.lwwreg_apply(S, P, want_op_err=True, check_status=False)
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.status()
        assert e.value.code == CRDT_ENONCANON
        exp_state, exp_n = list(start), [0, 0, 0]
        lo = 0
        for i, hi in enumerate(ends):
            if i in good:
                exp_state[i], errs = ref.apply_list(start[i], ops[lo:hi])
                exp_n[i] = sum(errs)
            lo = hi
        assert S.to_lists() == exp_state, ends
        assert n_err.cpu().tolist() == exp_n
        gpu.status()  # cleared


# ----------------------------------------------------------------------- fold
@pytest.fixture(scope="module", params=[1, 2])
def fold_reps(request):
    mw = request.param
    rng = random.Random(0xF01D + mw)
    return mw, [[cases.rnd_reg(rng, mw) for _ in range(1025)] for _ in range(32)]


@pytest.mark.parametrize("n_reps", [1, 2, 3, 8, 32])
def test_fold(gpu, fold_reps, n_reps):
    mw, reps = fold_reps
    reps = reps[:n_reps]
    n = len(reps[0])
    exp = [ref.fold([r[i] for r in reps]) for i in range(n)]
    D = [_batch(r, mw) for r in reps]
    out, n_err = gpu.lwwreg_fold(D)
    gpu.status()
    assert out.to_lists() == [e[0] for e in exp]
    assert n_err.cpu().tolist() == [e[1] for e in exp]
    assert all(d.to_lists() == r for d, r in zip(D, reps))  # inputs are only read
    # n_reps - 1 device merges in rank order
    acc, errs = _batch(reps[0], mw), [0] * n
    for d in D[1:]:
        bitmap, _ = gpu.lwwreg_merge(acc, d)
        errs = [a + b for a, b in zip(errs, _bits(bitmap, n)[0])]
    assert acc.to_lists() == out.to_lists() and errs == n_err.cpu().tolist()
    # in place on replica 0, without the counts
    out2, none = gpu.lwwreg_fold(D, out=D[0], want_n_err=False)
    assert none is None and out2.to_lists() == [e[0] for e in exp]
    if n_reps >= 2:
        assert sum(e[1] for e in exp) > 0


def test_fold_orientation_and_rep_limit(gpu):
    import crdts_hip

    # equal markers, different values: the first replica in rank order keeps its value
    reps = [[(7 + r, 5)] * 3 for r in range(3)]
    D = [_batch(r, 1) for r in reps]
    fwd, e1 = gpu.lwwreg_fold(D)
    rev, e2 = gpu.lwwreg_fold(D[::-1])
    assert fwd.to_lists() == [(7, 5)] * 3 and rev.to_lists() == [(9, 5)] * 3
    assert fwd.to_lists() != rev.to_lists()
    assert e1.cpu().tolist() == e2.cpu().tolist() == [2, 2, 2]
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.lwwreg_fold([D[0]] + [D[1]] * 32)
    assert e.value.code == -1
    with pytest.raises(crdts_hip.CrdtError) as e:  # the output may be replica 0 only
        gpu.lwwreg_fold(D, out=D[1])
    assert e.value.code == -1


# ------------------------------------------- the reference's three properties
def _prims(seed, n):
    rng = random.Random(seed)
    # build_from_prim (test/lwwreg.rs:39-45): val = prim.0, marker = (prim.1, prim.0)
    out = []
    for _ in range(n):
        p0, p1 = rng.randrange(256), rng.randrange(1 << 16) if rng.random() < 0.7 else rng.randrange(4)
        out.append((p0, (p1, p0)))
    return out


def _merged(gpu, a, b):
    """(a merged with b, conflicts) on the device."""
    A = _batch(a, 2)
    _, count = gpu.lwwreg_merge(A, _batch(b, 2))
    return A.to_lists(), int(count.item())


def test_reference_properties(gpu):
    n = 4096
    r1, r2, r3 = _prims(1, n), _prims(2, n), _prims(3, n)
    assert any(a[1][0] == b[1][0] for a, b in zip(r1, r2))  # equal first words occur: word 1 decides
    # the marker contains the value, so equal markers imply equal values: no
    # case is discarded and no merge may report a conflict
    total = 0
    # associative (test/lwwreg.rs:48-73)
    r12, c = _merged(gpu, r1, r2); total += c
    left, c = _merged(gpu, r12, r3); total += c
    r23, c = _merged(gpu, r2, r3); total += c
    right, c = _merged(gpu, r1, r23); total += c
    assert left == right
    # commutative (:75-92)
    r21, c = _merged(gpu, r2, r1); total += c
    assert r12 == r21
    # idempotent (:94-102)
    rr, c = _merged(gpu, r1, list(r1)); total += c
    assert rr == r1
    assert total == 0
    assert left == [ref.merge(ref.merge(a, b)[0], c_)[0] for a, b, c_ in zip(r1, r2, r3)]


# -------------------------------------------------------------------- bincode
GOLDEN = [
    # LWWReg<u8, (u16, u8)>: 4 bytes
    (1, (2, 1), [(0xAB, (0x1234, 0xAB)), (0, (0, 0)), (0xFF, (0xFFFF, 0xFF))],
     "ab3412ab" "00000000" "ffffffff"),
    # LWWReg<u64, u64>: 16 bytes
    (8, 8, [(0x0102030405060708, 0x1112131415161718), (1, BIG)],
     "0807060504030201" "1817161514131211" "0100000000000000" "ffffffffffffffff"),
    # LWWReg<u32, (u16, u8)>: 7 bytes, every blob after the first unaligned
    (4, (2, 1), [(0xDEADBEEF, (0xCAFE, 0x7F)), (1, (2, 3)), (0xFFFFFFFF, (0, 0x80))],
     "efbeadde" "feca" "7f" "01000000" "0200" "03" "ffffffff" "0000" "80"),
    # LWWReg<u16, u8>: 3 bytes
    (2, 1, [(0x0102, 0x03), (0xFFFF, 0)], "020103" "ffff00"),
]


@pytest.mark.parametrize("vb,mb,regs,blob_hex", GOLDEN)
def test_bincode_golden_blobs(gpu, vb, mb, regs, blob_hex):
    import torch

    blob = bytes.fromhex(blob_hex)
    assert blob == b"".join(ref.to_binary(r, vb, mb) for r in regs)
    mw = len(mb) if isinstance(mb, tuple) else 1
    d = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    got = gpu.lwwreg_from_bincode(d, len(regs), vb, mb)
    assert got.to_lists() == regs
    out = gpu.lwwreg_to_bincode(_batch(regs, mw), vb, mb)
    assert bytes(out.cpu().numpy()) == blob


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_bincode_round_trip(gpu, n):
    import torch

    rng = random.Random(0xB1C + n)
    for vb, mb, pad in ((1, (2, 1), 0), (8, 8, 0), (4, (2, 1), 0), (2, 4, 3), (8, (8, 8), 0), (1, 1, 1), (4, (8, 2), 5)):
        widths = mb if isinstance(mb, tuple) else (mb,)
        mw = len(widths)

        def word(w):
            return rng.choice((0, (1 << (8 * w)) - 1, rng.randrange(1 << (8 * w))))

        regs = [(word(vb), tuple(word(w) for w in widths) if mw == 2 else word(mb)) for _ in range(n)]
        size = vb + sum(widths)
        stride = size + pad
        blob = b"".join(ref.to_binary(r, vb, mb) + b"\xee" * pad for r in regs)[:(n - 1) * stride + size]
        out = torch.full((len(blob),), 0xEE, dtype=torch.uint8, device="cuda")
        gpu.lwwreg_to_bincode(_batch(regs, mw), vb, mb, stride=stride, out=out)
        assert bytes(out.cpu().numpy()) == blob  # the bytes between blobs are untouched
        assert gpu.lwwreg_from_bincode(out, n, vb, mb, stride=stride).to_lists() == regs


@pytest.mark.parametrize("which", ["val", "marker0", "marker1"])
def test_bincode_egest_latches_a_word_that_does_not_fit(gpu, which):
    import crdts_hip
    import torch
    from crdts_hip._lib import CRDT_ENONCANON

    vb, mb = 1, (2, 1)
    regs = [(i, (1000 + i, i)) for i in range(70)]
    bad = 33
    regs[bad] = {"val": (256, (5, 5)), "marker0": (5, (1 << 16, 5)), "marker1": (5, (5, 1 << 63))}[which]
    out = torch.full((4 * len(regs),), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.lwwreg_to_bincode(_batch(regs, 2), vb, mb, out=out)
    assert e.value.code == CRDT_ENONCANON
    exp = b"".join(b"\xee" * 4 if i == bad else ref.to_binary(r, vb, mb) for i, r in enumerate(regs))
    assert bytes(out.cpu().numpy()) == exp  # that blob unwritten, the neighbours exact
    gpu.status()


# ------------------------------------------------- argument checks, live ctx
def test_argument_checks_with_a_live_context(gpu):
    import crdts_hip
    from crdts_hip._lib import LWWOpsC, LWWViewC, lib

    S, O = _batch([(1, 2)] * 4, 1), _batch([(3, 2)] * 4, 1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ctx = gpu.ctx
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.lwwreg_merge(S, S)  # self == other
    assert e.value.code == -1
    assert lib.crdt_lwwreg_merge(ctx, p(S.val), p(S.marker), p(O.val), p(S.marker), 4, 1, None, None, None) == -1
    assert lib.crdt_lwwreg_merge(ctx, p(S.val), None, p(O.val), p(O.marker), 4, 1, None, None, None) == -1
    assert lib.crdt_lwwreg_merge(ctx, p(S.val), p(S.marker), p(O.val), p(O.marker), 4, 3, None, None, None) == -1
    assert lib.crdt_lwwreg_merge(ctx, None, None, None, None, 0, 1, None, None, None) == 0
    ops = crdts_hip.LWWOps.from_lists([[(5, 5)]] * 4)
    n_err = S.val.new_zeros(4).int()
    c = ops.cops()
    assert lib.crdt_lwwreg_apply(ctx, p(S.val), p(S.marker), None, 4, 1, p(n_err), None, None) == -1
    assert lib.crdt_lwwreg_apply(ctx, p(S.val), p(S.marker), C.byref(c), 4, 3, p(n_err), None, None) == -1
    assert lib.crdt_lwwreg_apply(ctx, p(S.val), p(S.marker), C.byref(c), 4, 1, None, None, None) == -1
    alias = LWWOpsC(c.obj_end, S.val.data_ptr(), c.marker, 4)
    assert lib.crdt_lwwreg_apply(ctx, p(S.val), p(S.marker), C.byref(alias), 4, 1, p(n_err), None, None) == -1
    hole = LWWOpsC(c.obj_end, None, c.marker, 4)
    assert lib.crdt_lwwreg_apply(ctx, p(S.val), p(S.marker), C.byref(hole), 4, 1, p(n_err), None, None) == -1
    empty = LWWOpsC(None, None, None, 0)
    assert lib.crdt_lwwreg_apply(ctx, None, None, C.byref(empty), 0, 1, None, None, None) == 0
    views = (LWWViewC * 2)(S.view(), LWWViewC(None, O.marker.data_ptr()))
    assert lib.crdt_lwwreg_fold(ctx, views, 2, 4, 1, p(S.val), p(S.marker), None, None) == -1
    assert lib.crdt_lwwreg_fold(ctx, views, 2, 0, 1, None, None, None, None) == 0
    assert lib.crdt_lwwreg_from_bincode(ctx, None, 16, 0, 8, 1, 8, 8, None, None, None) == 0
    assert lib.crdt_lwwreg_from_bincode(ctx, p(S.val), 16, 1, 3, 1, 8, 8, p(O.val), p(O.marker), None) == -1
    assert lib.crdt_lwwreg_to_bincode(ctx, p(S.val), p(S.marker), 1, 8, 1, 8, 8, None, 16, None) == -1
    # an empty batch through the Engine
    E = _batch([], 2)
    bitmap, count = gpu.lwwreg_merge(E, _batch([], 2))
    assert bitmap.numel() == 0 and int(count.item()) == 0
    assert S.to_lists() == [(1, 2)] * 4 and O.to_lists() == [(3, 2)] * 4  # nothing above touched the arrays
    gpu.status()
