"""GPU: the bincode codec of VClock / GCounter / PNCounter and of their ops
(crdt_clock_*_bincode*), exact against tests/clock_bincode_ref.py and the
host models crdts_hip.VClock / GCounter / PNCounter.

A 1 024-actor universe cannot hold a run of 1 100 distinct actors: there the
longest run is the full universe (1 024 entries); the 2^32 - 1 universe takes
the 1 100."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import clock_bincode_ref as ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENONCANON, ECAPACITY = 0, -2, -4
U64 = (1 << 64) - 1
SENTINEL = 0xA5


def _torch():
    import torch

    return torch


def u8(b):
    t = _torch()
    return t.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()


def i64(x):
    t = _torch()
    return t.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint64)).view(np.int64)).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def status(eng):
    from crdts_hip._lib import lib

    return lib.crdt_ctx_status(eng.ctx, None)


def p(t):
    return C.c_void_p(t.data_ptr())


def golden():
    with open(os.path.join(REPO, "tests", "golden", "bincode_clocks.json")) as f:
        return json.load(f)


def gen_clock(rng, universe, full=None, counters=None):
    """A clock over [0, universe): empty, single, full or random."""
    shape = rng.choice(["empty", "single", "full", "some", "some"]) if full is None else full
    if shape == "empty":
        acts = []
    elif shape == "single":
        acts = [rng.randrange(universe)]
    elif shape == "full" and universe <= 4096:
        acts = range(universe)
    else:
        acts = rng.sample(range(universe), rng.randrange(0, min(universe, 40) + 1))
    return {a: rng.choice(counters or [1, U64, rng.randrange(1, 1 << 40)]) for a in acts}


def gen_states(rng, n, universe, kind):
    return [[gen_clock(rng, universe) for _ in range(ref.n_clocks(kind))] for _ in range(n)]


def ingest_dense(eng, blobs, ab, A, kind, lead=0, gap=0, check_status=True):
    buf, off, ln = ref.pack(blobs, lead, gap)
    rows = eng.clock_from_bincode(u8(buf), i64(off), i64(ln), A, ab, kind, check_status=check_status)
    return host_u64(rows), off


def blobs_of(out, off, lens):
    o, f, ln = out.cpu().numpy().tobytes(), off.cpu().tolist(), lens.cpu().tolist()
    return [o[a:a + b] for a, b in zip(f, ln)]


# ----------------------------------------------------------------- golden
def test_golden_states_dense_and_csr(gpu):
    for s in golden()["states"]:
        blob, ab, kind = bytes.fromhex(s["hex"]), s["actor_bytes"], s["kind"]
        clocks = [dict(map(tuple, c)) for c in s["clocks"]]
        top = max([a for c in clocks for a in c] + [0]) + 1
        for A in {top, top + 3} if top <= 4096 else ():
            rows, _ = ingest_dense(gpu, [blob], ab, A, kind)
            assert rows[0].tolist() == ref.state_row(clocks, A), s["name"]
            out, off, lens = gpu.clock_to_bincode(i64(rows), A, ab, kind)
            assert blobs_of(out, off, lens) == [blob], s["name"]
        buf, off, ln = ref.pack([blob])
        B = gpu.clock_csr_from_bincode(u8(buf), i64(off), i64(ln), ab, kind)
        Bs = B if isinstance(B, tuple) else (B,)
        assert [b.clocks()[0] for b in Bs] == [sorted(c.items()) for c in clocks], s["name"]
        assert blobs_of(*gpu.clock_csr_to_bincode(B, ab)) == [blob], s["name"]


def test_golden_ops(gpu):
    import crdts_hip

    for o in golden()["ops"]:
        blob, ab, wd = bytes.fromhex(o["hex"]), o["actor_bytes"], o["dir"] is not None
        ops = crdts_hip.ClockOps.from_bincode(u8(blob), None, [1], ab, wd, engine=gpu)
        _, act, ctr, dr = ops.t
        assert act.cpu().numpy().view(np.uint32).tolist() == [o["actor"]], o["name"]
        assert host_u64(ctr).tolist() == [o["counter"]]
        assert (dr.cpu().tolist() == [o["dir"]]) if wd else dr is None
        assert ops.to_bincode(ab, engine=gpu).cpu().numpy().tobytes() == blob, o["name"]


# ------------------------------------------------------------------ dense
def widths_for(A):
    return [w for w in (1, 2, 4, 8) if A <= 1 << (8 * w)]


@pytest.mark.parametrize("kind", ["vclock", "pncounter"])
@pytest.mark.parametrize("A", [1, 16, 17, 64, 65, 128, 300])
def test_dense_actor_counts(gpu, A, kind):
    rng = random.Random(A * 7 + len(kind))
    n = 65
    states = gen_states(rng, n, A, kind)
    states[0] = [dict.fromkeys(range(A), U64)] * ref.n_clocks(kind)  # full, every counter 2^64 - 1
    states[1] = [{}] * ref.n_clocks(kind)
    states[2] = [{A - 1: 1}] * ref.n_clocks(kind)
    want = [ref.state_row(s, A) for s in states]
    for ab in widths_for(A):
        blobs = [ref.encode_state(s, ab) for s in states]
        rows, off = ingest_dense(gpu, blobs, ab, A, kind, lead=rng.randrange(16), gap=rng.randrange(4))
        assert rows.tolist() == want, (A, kind, ab)
        out, boff, lens = gpu.clock_to_bincode(i64(rows), A, ab, kind)
        assert blobs_of(out, boff, lens) == blobs, (A, kind, ab)
        assert lens.cpu().tolist() == [8 * len(s) + sum(map(len, s)) * (ab + 8) for s in states]


@pytest.mark.parametrize("kind", ["gcounter", "pncounter"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3001])
def test_dense_object_counts(gpu, n, kind):
    rng = random.Random(n)
    A, ab = 16, rng.choice([1, 8])
    states = gen_states(rng, n, A, kind)
    blobs = [ref.encode_state(s, ab) for s in states]
    gaps, end = [], 5 + len(blobs[0])  # blob k starts at byte residue (5 + 7 k) mod 16
    for k in range(1, n):
        gaps.append((5 + 7 * k - end) % 16)
        end += gaps[-1] + len(blobs[k])
    # (no gap after the last blob: it ends on the buffer's last byte)
    rows, off = ingest_dense(gpu, blobs, ab, A, kind, lead=5, gap=gaps + [0])
    assert rows.tolist() == [ref.state_row(s, A) for s in states]
    if n >= 63:
        assert {o % 16 for o in off} == set(range(16))
    out, boff, lens = gpu.clock_to_bincode(i64(rows), A, ab, kind)
    assert blobs_of(out, boff, lens) == blobs


@pytest.mark.parametrize("kind,A", [("pncounter", 1024), ("vclock", 1500), ("pncounter", 513)])
def test_dense_rows_past_the_tile(gpu, kind, A):
    """Rows wider than the staging tile leave it in windows; a bad one is zero in every window."""
    rng = random.Random(A)
    nc, ab = ref.n_clocks(kind), 2
    states = gen_states(rng, 9, A, kind)
    states[0] = [dict.fromkeys(range(A), U64)] * nc
    edge = [{}, {}]  # the slots on both sides of the first window boundary, and the row's ends
    for slot in (0, 1023, 1024, A * nc - 1):
        edge[slot // A][slot % A] = slot + 1
    states[3] = edge[:nc]
    blobs = [ref.encode_state(s, ab) for s in states]
    bad = bytearray(ref.encode_state([dict.fromkeys(range(A), 7)] * nc, ab))
    bad[-8:] = bytes(8)  # the last counter of the last clock is zero
    blobs.insert(5, bytes(bad))
    rows, _ = ingest_dense(gpu, blobs, ab, A, kind, lead=9, gap=1, check_status=False)
    assert status(gpu) == ENONCANON
    want = [ref.state_row(s, A) for s in states]
    want.insert(5, [0] * (A * nc))
    assert rows.tolist() == want
    keep = [k for k in range(len(blobs)) if k != 5]
    out, off, lens = gpu.clock_to_bincode(i64(rows[keep]), A, ab, kind)
    assert blobs_of(out, off, lens) == [blobs[k] for k in keep]


def test_dense_every_offset_residue(gpu):
    rng = random.Random(3)
    for kind, A, ab in (("vclock", 16, 1), ("pncounter", 20, 2), ("gcounter", 70, 8)):
        s = [gen_clock(rng, A, "some") for _ in range(ref.n_clocks(kind))]
        for lead in range(16):
            rows, _ = ingest_dense(gpu, [ref.encode_state(s, ab)], ab, A, kind, lead=lead)
            assert rows[0].tolist() == ref.state_row(s, A), (kind, lead)


@pytest.mark.parametrize("kind,A,ab", [("vclock", 16, 1), ("pncounter", 16, 8), ("gcounter", 65, 2),
                                       ("pncounter", 300, 4)])
def test_dense_egest_into_sentinel_buffer(gpu, kind, A, ab):
    """Blobs at arbitrary byte offsets: every byte outside them is unchanged."""
    from crdts_hip._lib import lib

    t = _torch()
    rng = random.Random(A + ab)
    n, nc = 130, ref.n_clocks(kind)
    states = gen_states(rng, n, A, kind)
    blobs = [ref.encode_state(s, ab) for s in states]
    rows = i64([ref.state_row(s, A) for s in states])
    sizes = t.zeros(n, dtype=t.int64).cuda()
    assert lib.crdt_clock_dense_bincode_sizes(gpu.ctx, p(rows), n, A, nc, ab, p(sizes), None) == OK
    assert sizes.cpu().tolist() == [len(b) for b in blobs]
    want, off = bytearray([SENTINEL] * rng.randrange(1, 17)), []
    for k, b in enumerate(blobs):
        want += bytes([SENTINEL] * ((3 + 5 * k - len(want)) % 16))  # blob k at byte residue (3 + 5 k) mod 16
        off.append(len(want))
        want += b
    want += bytes([SENTINEL] * 7)
    assert {o % 16 for o in off} == set(range(16))
    out = t.full((len(want),), SENTINEL, dtype=t.uint8).cuda()
    assert lib.crdt_clock_dense_to_bincode(gpu.ctx, p(rows), n, A, nc, ab, p(out), p(i64(off)), len(want), None) == OK
    assert status(gpu) == OK
    assert out.cpu().numpy().tobytes() == bytes(want)


# -------------------------------------------------------------------- CSR
def csr_run(rng, length, universe):
    if length == universe:
        acts = range(universe)
    else:
        acts = set()
        while len(acts) < length:
            acts.add(rng.randrange(universe))
    return {a: rng.choice([1, U64, rng.randrange(1, 1 << 40)]) for a in acts}


@pytest.mark.parametrize("kind", ["vclock", "pncounter"])
@pytest.mark.parametrize("universe", [1024, (1 << 32) - 1])
def test_csr_runs(gpu, universe, kind):
    import crdts_hip

    rng = random.Random(universe % 1000 + len(kind))
    lengths = [0, 1, 64, 65, 200, min(1100, universe)] + [rng.randrange(0, 70) for _ in range(70)]
    rng.shuffle(lengths)
    nc = ref.n_clocks(kind)
    states = [[csr_run(rng, lengths[(i + 3 * c) % len(lengths)], universe) for c in range(nc)]
              for i in range(len(lengths))]
    want = [[sorted(s[c].items()) for s in states] for c in range(nc)]
    for ab in (2, 8) if universe == 1024 else (4, 8):
        blobs = [ref.encode_state(s, ab) for s in states]
        buf, off, ln = ref.pack(blobs, lead=rng.randrange(16), gap=rng.randrange(5))
        for gap in (0, 3):  # gapped placement
            B = gpu.clock_csr_from_bincode(u8(buf), i64(off), i64(ln), ab, kind, gap=gap)
            Bs = B if isinstance(B, tuple) else (B,)
            for c, b in enumerate(Bs):
                assert b.clocks() == want[c], (universe, kind, ab, gap, c)
                o, l_ = b.off.cpu().tolist(), b.len.cpu().tolist()
                assert all(o[k] + l_[k] + gap == o[k + 1] for k in range(len(o) - 1))
            assert blobs_of(*gpu.clock_csr_to_bincode(B, ab)) == blobs
    # straight into the CSR kernels
    others = [dict([(universe - 1, 3)] + [(a, 1 << 41) for a, _ in w[::2]]) for w in want[0]]
    S, O = Bs[0], crdts_hip.ClockBatch.from_lists(others)
    merged = gpu.clock_csr_merge(S, O).clocks()
    for got, w, o in zip(merged, want[0], others):
        m = crdts_hip.VClock(w, n_actors=universe)
        for a, c in o.items():
            m.witness(a, c)
        assert got == sorted(m.dots.items())
    vals = host_u64(gpu.clock_csr_value(S)).tolist()
    assert vals == [crdts_hip.GCounter(w).value() for w in want[0]]


# -------------------------------------------------------------- malformed
def _q(v):
    return v.to_bytes(8, "little")


GOOD = {1: {1: 2, 3: 4}, 2: {0: 7}}  # neighbours of every bad blob


def bad_states(ab, kind, limit):
    """name -> blob, one per CRDT_ENONCANON class (limit: n_actors, or 2^32)."""
    a = lambda v: v.to_bytes(ab, "little")  # noqa: E731
    tail = _q(0) if kind == "pncounter" else b""
    out = {
        "zero counter": _q(1) + a(1) + _q(0) + tail,
        "descending": _q(2) + a(3) + _q(1) + a(1) + _q(1) + tail,
        "duplicate": _q(2) + a(3) + _q(1) + a(3) + _q(2) + tail,
        "ends early": (_q(1) + a(1) + _q(1) + tail)[:-1],
        "trailing byte": _q(1) + a(1) + _q(1) + tail + b"\x00",
        "length 2^63": _q(1 << 63) + a(1) + _q(1) + tail,
        "length 2^64-1": _q(U64) + a(1) + _q(1) + tail,
        "length too large by one": _q(2) + a(1) + _q(1) + tail,
        "shorter than a length word": b"\x00" * 7,
    }
    if limit < 1 << (8 * ab):
        out["actor at the limit"] = _q(1) + a(limit) + _q(1) + tail
    if kind == "pncounter":
        out["p swallows n"] = _q(1) + a(1) + _q(1)
        out["p runs past the blob"] = _q(3) + a(1) + _q(1) + _q(0)
        out["bad n clock"] = _q(1) + a(1) + _q(1) + _q(1) + a(2) + _q(0)
    return out


@pytest.mark.parametrize("kind", ["vclock", "pncounter"])
@pytest.mark.parametrize("ab,A", [(1, 16), (8, 300)])
def test_dense_malformed(gpu, ab, A, kind):
    nc = ref.n_clocks(kind)
    goods = [[GOOD[1]] * nc, [GOOD[2]] * nc]
    gb = [ref.encode_state(s, ab) for s in goods]
    for name, bad in bad_states(ab, kind, A).items():
        with pytest.raises(ref.FormatError):
            ref.decode_state(bad, ab, kind, actor_limit=A)
        rows, _ = ingest_dense(gpu, [gb[0], bad, gb[1]], ab, A, kind, lead=3, check_status=False)
        assert status(gpu) == ENONCANON, name
        assert rows[1].tolist() == [0] * (A * nc), name
        assert rows[0].tolist() == ref.state_row(goods[0], A) and rows[2].tolist() == ref.state_row(goods[1], A), name
    edge = ref.encode_state([{A - 1: 1}] * nc, ab)  # actor n_actors - 1 is good
    rows, _ = ingest_dense(gpu, [gb[0], edge, gb[1]], ab, A, kind)
    assert rows[1].tolist() == ref.state_row([{A - 1: 1}] * nc, A)


@pytest.mark.parametrize("kind", ["vclock", "pncounter"])
@pytest.mark.parametrize("ab", [1, 8])
def test_csr_malformed(gpu, ab, kind):
    nc = ref.n_clocks(kind)
    goods = [[GOOD[1]] * nc, [GOOD[2]] * nc]
    gb = [ref.encode_state(s, ab) for s in goods]
    cases = bad_states(ab, kind, 1 << 32)
    if ab == 8:
        cases["actor 2^32"] = _q(1) + _q(1 << 32) + _q(1) + (_q(0) if nc == 2 else b"")
    for name, bad in cases.items():
        with pytest.raises(ref.FormatError):
            ref.decode_state(bad, ab, kind, actor_limit=1 << 32)
        buf, off, ln = ref.pack([gb[0], bad, gb[1]], lead=1)
        B = gpu.clock_csr_from_bincode(u8(buf), i64(off), i64(ln), ab, kind, check_status=False)
        assert status(gpu) == ENONCANON, name
        for c, b in enumerate(B if isinstance(B, tuple) else (B,)):
            assert b.len.cpu().tolist()[1] == 0, name
            got = b.clocks()
            assert got[0] == sorted(goods[0][c].items()) and got[2] == sorted(goods[1][c].items()), name
    if ab == 8:  # 2^32 - 1 is the largest actor a run holds
        buf, off, ln = ref.pack([ref.encode_state([{(1 << 32) - 1: 5}] * nc, ab)])
        B = gpu.clock_csr_from_bincode(u8(buf), i64(off), i64(ln), ab, kind)
        assert (B[0] if nc == 2 else B).clocks() == [[((1 << 32) - 1, 5)]]


@pytest.mark.parametrize("kind", ["vclock", "pncounter"])
def test_blob_not_inside_the_buffer(gpu, kind):
    nc = ref.n_clocks(kind)
    g = ref.encode_state([GOOD[1]] * nc, 1)
    buf = g + g
    for off, ln in ((len(buf) - 4, len(g)), (len(buf) + 1, 0), (U64 - 3, len(g)), (0, U64)):
        rows = gpu.clock_from_bincode(u8(buf), i64([0, off, len(g)]), i64([len(g), ln, len(g)]), 16, 1, kind,
                                      check_status=False)
        assert status(gpu) == ENONCANON
        rows = host_u64(rows)
        assert rows[1].tolist() == [0] * (16 * nc)
        assert rows[0].tolist() == rows[2].tolist() == ref.state_row([GOOD[1]] * nc, 16)
        B = gpu.clock_csr_from_bincode(u8(buf), i64([0, off, len(g)]), i64([len(g), ln, len(g)]), 1, kind,
                                       check_status=False)
        assert status(gpu) == ENONCANON
        for b in (B if isinstance(B, tuple) else (B,)):
            assert b.len.cpu().tolist() == [2, 0, 2]


def test_dense_egest_errors(gpu):
    from crdts_hip._lib import lib

    t = _torch()
    A = 300
    rows = np.zeros((3, A), np.uint64)
    rows[0, 5], rows[1, 256], rows[2, 255] = 9, 1, 3  # slot 256 does not fit one byte
    out, off, lens = gpu.clock_to_bincode(i64(rows), A, 1, "vclock", check_status=False)
    assert status(gpu) == ENONCANON
    assert lens.cpu().tolist() == [17, 0, 17]
    got = blobs_of(out, off, lens)
    assert got[0] == ref.encode_state([{5: 9}], 1) and got[2] == ref.encode_state([{255: 3}], 1) and got[1] == b""
    rows[1, 256] = 0  # the same slot set to zero is fine
    out, off, lens = gpu.clock_to_bincode(i64(rows), A, 1, "vclock")
    assert lens.cpu().tolist() == [17, 8, 17]
    # a blob placed past out_bytes
    d = i64(rows)
    buf = t.full((64,), SENTINEL, dtype=t.uint8).cuda()
    rc = lib.crdt_clock_dense_to_bincode(gpu.ctx, p(d), 3, A, 1, 1, p(buf), p(i64([0, 17, 48])), 64, None)
    assert rc == OK and status(gpu) == ECAPACITY
    got = buf.cpu().numpy().tobytes()
    assert got[:17] == ref.encode_state([{5: 9}], 1) and got[17:25] == bytes(8)
    assert got[25:] == bytes([SENTINEL] * 39)  # blob 2 (17 bytes at 48) is not written


def test_csr_egest_errors(gpu):
    import crdts_hip

    good = {1: 2, 300: 4}
    off = np.array([0, 2, 4, 6], np.uint64)
    ln = np.array([2, 2, 2, 2], np.uint32)
    act = np.array([1, 300, 300, 1, 1, 2, 7, 7], np.uint32)  # run 1 descends, run 3 repeats an actor
    ctr = np.array([2, 4, 1, 1, 1, 0, 1, 1], np.uint64)      # run 2 holds a zero counter
    B = crdts_hip.ClockBatch.from_host(off, ln, act, ctr)
    out, boff, lens = gpu.clock_csr_to_bincode(B, 2, check_status=False)
    assert status(gpu) == ENONCANON
    assert lens.cpu().tolist() == [28, 0, 0, 0]
    assert blobs_of(out, boff, lens)[0] == ref.encode_state([good], 2)
    out, boff, lens = gpu.clock_csr_to_bincode(B, 1, check_status=False)  # 300 does not fit a byte
    assert status(gpu) == ENONCANON and lens.cpu().tolist() == [0, 0, 0, 0]
    far = crdts_hip.ClockBatch.from_host(np.array([0, 7], np.uint64), np.array([2, 2], np.uint32), act, ctr)
    out, boff, lens = gpu.clock_csr_to_bincode(far, 2, check_status=False)  # run 1 leaves the arrays
    assert status(gpu) == ENONCANON and lens.cpu().tolist() == [28, 0]


def test_csr_run_placed_past_capacity(gpu):
    """out.off is the caller's: a run that does not fit out.n_entries latches CRDT_ECAPACITY and is not written."""
    from crdts_hip._lib import ClockCsrOut, lib

    t = _torch()
    blobs = [ref.encode_state([c], 1) for c in ({1: 2, 3: 4}, {5: 6, 7: 8}, {9: 1})]
    buf, off, ln = ref.pack(blobs)
    d = u8(buf)
    lens = t.zeros(3, dtype=t.int32).cuda()
    act = t.full((5,), -1, dtype=t.int32).cuda()
    ctr = t.full((5,), -1, dtype=t.int64).cuda()
    place = i64([0, 3, 2])  # run 1 would end at entry 5 of 4
    w = ClockCsrOut(p(place), p(lens), p(act), p(ctr), 4)
    assert lib.crdt_clock_csr_from_bincode(gpu.ctx, p(d), len(buf), p(i64(off)), p(i64(ln)), 3, 1, 1, C.byref(w),
                                           None, None) == OK
    assert status(gpu) == ECAPACITY
    assert lens.cpu().tolist() == [2, 0, 1]
    assert act.cpu().tolist() == [1, 3, 9, -1, -1] and ctr.cpu().tolist() == [2, 4, 1, -1, -1]


# -------------------------------------------------------------------- ops
@pytest.mark.parametrize("with_dir", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5003])
def test_ops_round_trip(gpu, n, with_dir):
    import crdts_hip

    t = _torch()
    rng = random.Random(n + with_dir)
    for ab in (1, 2, 4, 8):
        top = min(1 << (8 * ab), 1 << 32)
        ops = [(rng.randrange(top), rng.choice([0, 1, U64, rng.randrange(1 << 50)]),
                rng.randrange(2) if with_dir else None) for _ in range(n)]
        size = ref.op_bytes(ab, with_dir)
        for stride in (size, size + rng.randrange(1, 9)):
            want = bytearray([SENTINEL] * (ref.op_bytes(ab, with_dir) + (n - 1) * stride if n else 0))
            for j, o in enumerate(ops):
                want[j * stride:j * stride + size] = ref.encode_op(o[0], o[1], ab, o[2])
            got = crdts_hip.ClockOps.from_bincode(u8(want), stride, [n] if n else [], ab, with_dir, engine=gpu)
            _, act, ctr, dr = got.t
            assert act.cpu().numpy().view(np.uint32).tolist() == [o[0] for o in ops]
            assert host_u64(ctr).tolist() == [o[1] for o in ops]
            if with_dir:
                assert dr.cpu().tolist() == [o[2] for o in ops]
            out = t.full((len(want),), SENTINEL, dtype=t.uint8).cuda()
            got.to_bincode(ab, stride, out=out, engine=gpu)
            assert out.cpu().numpy().tobytes() == bytes(want)  # the gaps keep the sentinel


def test_ops_malformed(gpu):
    import crdts_hip

    good = [(7, 1, 1), (9, 5, 0)]
    for d in (0, 1, 2, 0x100, 0x01000000):
        blobs = ref.encode_op(*good[0][:2], 1, good[0][2]) + (ref.encode_op(3, 4, 1) + d.to_bytes(4, "little")) + \
            ref.encode_op(*good[1][:2], 1, good[1][2])
        ops = crdts_hip.ClockOps.from_bincode(u8(blobs), None, [3], 1, True, engine=gpu, check_status=False)
        _, act, ctr, dr = ops.t
        act = act.cpu().numpy().view(np.uint32).tolist()
        assert status(gpu) == (OK if d <= 1 else ENONCANON), d
        mid = (3, 4, d) if d <= 1 else (0xFFFFFFFF, 0, 0)  # the skip sentinel
        assert list(zip(act, host_u64(ctr).tolist(), dr.cpu().tolist())) == [good[0], mid, good[1]], d
    for wd in (False, True):  # an 8-byte actor of 2^32
        tail = [0] if wd else []
        blobs = b"".join(ref.encode_op(a, 6, 8, *tail) for a in ((1 << 32) - 1, 1 << 32, 5))
        ops = crdts_hip.ClockOps.from_bincode(u8(blobs), None, [3], 8, wd, engine=gpu, check_status=False)
        assert status(gpu) == ENONCANON
        assert ops.t[1].cpu().numpy().view(np.uint32).tolist() == [(1 << 32) - 1, 0xFFFFFFFF, 5]
        assert host_u64(ops.t[2]).tolist() == [6, 0, 6]
    # egest: a dir above 1, an actor too wide
    ops = crdts_hip.ClockOps.from_lists([[(1, 2, 0), (3, 4, 2), (5, 6, 1)]], with_dir=True)
    out = _torch().full((39,), SENTINEL, dtype=_torch().uint8).cuda()
    ops.to_bincode(1, out=out, engine=gpu, check_status=False)
    assert status(gpu) == ENONCANON
    assert out.cpu().numpy().tobytes() == ref.encode_op(1, 2, 1, 0) + bytes([SENTINEL] * 13) + ref.encode_op(5, 6, 1, 1)
    ops = crdts_hip.ClockOps.from_lists([[(1, 2), (256, 4)]])
    out = _torch().full((18,), SENTINEL, dtype=_torch().uint8).cuda()
    ops.to_bincode(1, out=out, engine=gpu, check_status=False)
    assert status(gpu) == ENONCANON
    assert out.cpu().numpy().tobytes() == ref.encode_op(1, 2, 1) + bytes([SENTINEL] * 9)


# -------------------------------------------------------- the loop closes
def gen_op_lists(rng, n, universe, with_dir):
    return [[(rng.randrange(universe), rng.choice([0, 1, U64, rng.randrange(1 << 40)])) +
             ((rng.randrange(2),) if with_dir else ()) for _ in range(rng.choice([0, 1, 3, 9]))] for _ in range(n)]


def ops_from_wire(gpu, per_obj, ab, with_dir):
    import crdts_hip

    flat = [o for ops in per_obj for o in ops]
    blobs = b"".join(ref.encode_op(o[0], o[1], ab, o[2] if with_dir else None) for o in flat)
    ends = np.cumsum([len(ops) for ops in per_obj]).astype(np.uint64)
    return crdts_hip.ClockOps.from_bincode(u8(blobs), None, ends, ab, with_dir, engine=gpu)


@pytest.mark.parametrize("kind", ["gcounter", "pncounter"])
def test_loop_dense(gpu, kind):
    import crdts_hip

    rng = random.Random(len(kind))
    n, A, ab, wd = 200, 20, 2, kind == "pncounter"
    states = gen_states(rng, n, A, kind)
    per_obj = gen_op_lists(rng, n, A, wd)
    buf, off, ln = ref.pack([ref.encode_state(s, ab) for s in states], lead=7)
    rows = gpu.clock_from_bincode(u8(buf), i64(off), i64(ln), A, ab, kind)
    gpu.dense_apply(rows, ops_from_wire(gpu, per_obj, ab, wd), A, kind)
    want = []
    for s, ops in zip(states, per_obj):
        if wd:
            m = crdts_hip.PNCounter(A)
            m.p.dots, m.n.dots = dict(s[0]), dict(s[1])
            for a, c, d in ops:
                m.apply(((a, c), d == 0))
            want.append(ref.encode_state([m.p.dots, m.n.dots], ab))
        else:
            m = crdts_hip.GCounter(n_actors=A)
            m.dots = dict(s[0])
            for dot in ops:
                m.apply(dot)
            want.append(ref.encode_state([m.dots], ab))
    assert blobs_of(*gpu.clock_to_bincode(rows, A, ab, kind)) == want


def test_loop_csr(gpu):
    import crdts_hip

    rng = random.Random(77)
    n, universe, ab = 200, (1 << 32) - 1, 4
    states = [[csr_run(rng, rng.choice([0, 1, 5, 64, 70]), universe)] for _ in range(n)]
    per_obj = []
    for s in states:  # dots that hit existing actors and new ones
        acts = list(s[0]) or [3]
        per_obj.append([(rng.choice([rng.choice(acts), rng.randrange(universe)]), rng.choice([0, 1, U64, 1 << 33]))
                        for _ in range(rng.choice([0, 1, 3, 9]))])
    buf, off, ln = ref.pack([ref.encode_state(s, ab) for s in states], lead=2, gap=1)
    S = gpu.clock_csr_from_bincode(u8(buf), i64(off), i64(ln), ab, "vclock", gap=2)
    out = gpu.clock_csr_apply(S, ops_from_wire(gpu, per_obj, ab, False))
    want = []
    for s, ops in zip(states, per_obj):
        m = crdts_hip.VClock(n_actors=universe)
        m.dots = dict(s[0])
        for a, c in ops:
            m.witness(a, c)
        want.append(ref.encode_state([m.dots], ab))
    assert blobs_of(*gpu.clock_csr_to_bincode(out, ab)) == want


# ------------------------------------------------------------ round trips
@pytest.mark.parametrize("kind", ["vclock", "pncounter"])
def test_round_trip_blobs(gpu, kind):
    """egest(ingest(b)) == b over generated canonical blobs, dense and CSR."""
    rng = random.Random(len(kind) + 40)
    n, A = 3000, 48
    for ab in (1, 4):
        blobs = [ref.encode_state(s, ab) for s in gen_states(rng, n, A, kind)]
        buf, off, ln = ref.pack(blobs, lead=rng.randrange(16))
        d, o, l_ = u8(buf), i64(off), i64(ln)
        rows = gpu.clock_from_bincode(d, o, l_, A, ab, kind)
        assert blobs_of(*gpu.clock_to_bincode(rows, A, ab, kind)) == blobs
        B = gpu.clock_csr_from_bincode(d, o, l_, ab, kind)
        assert blobs_of(*gpu.clock_csr_to_bincode(B, ab)) == blobs


def test_round_trip_generated_rows(gpu):
    """ingest(egest(rows)) == rows over generate_dense / generate_clocks_csr."""
    import crdts_hip

    for A, nc, kind in ((16, 1, "vclock"), (64, 2, "pncounter"), (33, 1, "gcounter")):
        rows = crdts_hip.generate_dense(3000, A * nc, seed=A)
        d = i64(rows)
        out, off, lens = gpu.clock_to_bincode(d, A, 8, kind)
        back = gpu.clock_from_bincode(out, off, lens, A, 8, kind)
        assert (host_u64(back).reshape(rows.shape) == rows).all()
        assert lens.cpu().tolist() == (8 * nc + 16 * (rows != 0).sum(1)).tolist()
    (off, ln, act, ctr), other = crdts_hip.generate_clocks_csr(3000, seed=11)
    S = crdts_hip.ClockBatch.from_host(off, ln, act, ctr)
    for ab in (2, 4):
        out, boff, lens = gpu.clock_csr_to_bincode(S, ab)
        assert lens.cpu().tolist() == (8 + (ab + 8) * ln.astype(np.int64)).tolist()
        back = gpu.clock_csr_from_bincode(out, boff, lens, ab)
        assert back.clocks() == S.clocks()
    N = crdts_hip.ClockBatch.from_host(*other)
    out, boff, lens = gpu.clock_csr_to_bincode((S, N), 4)
    bp, bn = gpu.clock_csr_from_bincode(out, boff, lens, 4, "pncounter")
    assert bp.clocks() == S.clocks() and bn.clocks() == N.clocks()
