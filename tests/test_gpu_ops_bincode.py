"""GPU: the bincode codec of the Orswot, MVReg and Map op streams (crdt_ops_*),
exact against tests/ops_bincode_ref.py and the host packers
(crdts_hip.*Ops.arrays_from_lists / from_lists), and through the five applies."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import ops_bincode_cases as cases
import ops_bincode_ref as ref

pytestmark = pytest.mark.gpu

OK, ENONCANON, ECAPACITY = 0, -2, -4
U64 = cases.U64
SENTINEL = 0xA5
TYPES = (ref.ORSWOT, ref.MVREG, ref.MAP_MVREG, ref.MAP_ORSWOT, ref.MAP_MAP)
W8 = (8, 8, 8, 8)


def _torch():
    import torch

    return torch


def u8(b):
    t = _torch()
    return t.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()


def i64(x):
    t = _torch()
    return t.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint64)).view(np.int64)).cuda()


def dev(a):
    """{field: numpy u32 / u64} -> {field: device tensor}."""
    t = _torch()
    return {f: t.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.int64)).cuda()
            for f, x in a.items()}


def host(a):
    """{field: device tensor} -> {field: list of unsigned ints} (op_err: signed)."""
    out = {}
    for f, x in a.items():
        x = x.cpu().numpy()
        out[f] = x.tolist() if f == "op_err" else x.view(np.uint32 if x.dtype == np.int32 else np.uint64).tolist()
    return out


def lists(a):
    return {f: np.asarray(x).tolist() for f, x in a.items()}


def status(eng):
    from crdts_hip._lib import lib

    return lib.crdt_ctx_status(eng.ctx, None)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def ingest(gpu, t, blobs, w, lead=0, gap=0, check_status=True):
    buf, off, ln = ref.pack(blobs, lead, gap)
    return host(gpu.ops_from_bincode(u8(buf), i64(off), i64(ln), t, w, op_err=True, check_status=check_status))


def blobs_of(out, off, lens):
    o, f, ln = out.cpu().numpy().tobytes(), off.cpu().tolist(), lens.cpu().tolist()
    return [o[a:a + b] for a, b in zip(f, ln)]


def egest(gpu, t, arrays, w, check_status=True):
    return blobs_of(*gpu.ops_to_bincode(t, w, dev(arrays), check_status=check_status))


def round_trip(gpu, t, ops, w, lead=0, gap=0):
    """blobs of the restatement -> arrays == the host packing; arrays -> the same blobs."""
    blobs = [ref.encode(t, op, w) for op in ops]
    want = cases.arrays_of(t, ops)
    got = ingest(gpu, t, blobs, w, lead, gap)
    assert got.pop("op_err") == [0] * len(ops)
    assert got == lists(want)
    assert egest(gpu, t, want, w) == blobs
    return blobs, want


# ----------------------------------------------------------------- golden
def test_golden_blobs_into_arrays_and_out(gpu):
    groups = {}
    for o in cases.golden():
        groups.setdefault((ref.TYPES[o["type"]], tuple(o["widths"])), []).append(o)
    assert {t for t, _ in groups} == set(TYPES)
    for (t, w), g in groups.items():
        ops = [o["op"] for o in g]
        blobs = [bytes.fromhex(o["hex"]) for o in g]
        got = ingest(gpu, t, blobs, w, lead=3)
        assert got.pop("op_err") == [0] * len(g), (t, w)
        assert got == lists(cases.arrays_of(t, ops)), (t, w)
        assert egest(gpu, t, cases.arrays_of(t, ops), w) == blobs, (t, w)


# ------------------------------------------- the existing generators' ops
@functools.lru_cache(maxsize=None)
def generated(t):
    """>= 5 003 ops of the existing generator of the type, flat — computed once."""
    import map_opgen
    import map_orswot_opgen
    import mvreg_opgen
    import nested_opgen
    import opgen

    if t == ref.ORSWOT:
        rng, ops = random.Random(0x0B5), []
        while len(ops) < 5003:
            ops += orswot_wire_ops(opgen.orswot_opvec(rng))
    elif t == ref.MVREG:
        ops = [op for lst in mvreg_opgen.gen_batch(0x0B6, 1500, 8, 4, 9, 0, 8)["ops"] for op in lst]
    elif t == ref.MAP_MVREG:
        ops = [op for _, lst in map_opgen.gen_batch(0x0B7, 700, 8) for op in lst]
    elif t == ref.MAP_ORSWOT:
        ops = [op for _, lst in map_orswot_opgen.gen_batch(0x0B8, 700, 8) for op in lst]
    else:
        ops = [op for _, lst in nested_opgen.gen_batch(0x0B9, 900, 16) for op in lst]
    assert len(ops) >= 5003
    return tuple(ops)


def orswot_wire_ops(opvec):
    """The op vector as the reference puts it on the wire: a Dot with counter 0
    turns into the empty clock (VClock::from(Dot) witnesses nothing)."""
    return [op if op[0] == "add" else ("rm", op[1], [q for q in op[2] if q[1]]) for _, op in opvec]


def op_class(t):
    import crdts_hip

    return (crdts_hip.OrswotOps, crdts_hip.MVRegOps, crdts_hip.MapOps, crdts_hip.MapOrswotOps, crdts_hip.MapMapOps)[t]


def class_widths(t, w):
    """(actor, key, key2, val) -> the positional widths of the class's from_bincode / to_bincode."""
    wa, wk, w2, wv = w
    return {ref.ORSWOT: (wa, w2), ref.MVREG: (wa, wv), ref.MAP_MVREG: (wa, wk, wv), ref.MAP_ORSWOT: (wa, wk, w2),
            ref.MAP_MAP: (wa, wk, w2, wv)}[t]


def packed_tensors(t, per_obj):
    """The host packer's arrays after obj_end, as lists."""
    cls = op_class(t)
    if t == ref.ORSWOT:  # (no arrays_from_lists: the device batch, read back)
        return [x.cpu().numpy().view(np.uint32 if x.dtype == _torch().int32 else np.uint64).tolist()
                for x in cls.from_lists(per_obj).t[1:]]
    return [x.tolist() for x in cls.arrays_from_lists(per_obj)[1:]]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5003])
@pytest.mark.parametrize("t", TYPES)
def test_generated_ops_through_the_classes(gpu, t, n):
    ops = list(generated(t)[:n])
    blobs = [ref.encode(t, op, W8) for op in ops]
    buf, off, ln = ref.pack(blobs, lead=n % 16, gap=n % 3)
    per_obj = [ops[:n // 3], [], ops[n // 3:]]
    ends = [n // 3, n // 3, n]
    cw = class_widths(t, W8)
    got = op_class(t).from_bincode(u8(buf), i64(off), i64(ln), ends, *cw, engine=gpu)
    assert got.t[0].cpu().tolist() == ends and got.n_ops == n
    view = [x.cpu().numpy().view(np.uint32 if x.dtype == _torch().int32 else np.uint64).tolist() for x in got.t[1:]]
    assert view == packed_tensors(t, per_obj)
    out = blobs_of(*got.to_bincode(*cw, engine=gpu))
    assert out == blobs


# ---------------------------------------------------------- clock lengths
@pytest.mark.parametrize("t", TYPES)
def test_clock_lengths(gpu, t):
    """0 .. 2 048 pairs in one batch (every clocked kind of the type), ops
    without a clock between them, and one op with a 5 000-pair clock."""
    rng = random.Random(40 + t)
    w = (2, 8, 8, 8)
    ops = []
    for n in (0, 1, 2, 63, 64, 65, 130, 2048):
        for kind in cases.CLOCKED[t]:
            ops.append(cases.random_op(rng, t, w, kind=kind, n_pairs=n))
            ops.append(cases.random_op(rng, t, w))
    rng.shuffle(ops)
    blobs, want = round_trip(gpu, t, ops, w, lead=7, gap=1)
    assert max(np.diff(want["clk_end"].astype(np.int64), prepend=0)) == 2048
    lens = gpu.ops_clk_lens(u8(b"".join(blobs)), i64(np.cumsum([0] + [len(b) for b in blobs[:-1]])),
                            i64([len(b) for b in blobs]), t, w)
    assert lens.cpu().tolist() == [len(ref.pairs_of(t, op)) for op in ops]
    big = cases.random_op(rng, t, (4, 8, 8, 8), kind=cases.CLOCKED[t][-1], n_pairs=5000)
    round_trip(gpu, t, [ops[0], big, ops[1]], (4, 8, 8, 8), lead=1)


# ----------------------------------------------------------------- widths
@pytest.mark.parametrize("w", cases.WIDTH_SETS)
@pytest.mark.parametrize("t", TYPES)
def test_widths_with_the_largest_values(gpu, t, w):
    rng = random.Random(sum(w) + t)
    ops = cases.random_ops(rng, t, w, 200)
    top = {f: 0 for f in cases.FIELDS}
    for op in ops:
        for f, v in cases.fields_of(t, op).items():
            top[f] = max(top[f], v)
    wa, wk, w2, wv = w
    for f, width in (("key", wk), ("key2", w2), ("val", wv)):
        if f in cases.USED[t]:
            assert top[f] == (1 << (8 * width)) - 1, f
    if t != ref.MVREG:
        assert top["actor"] == min(1 << (8 * wa), 1 << 32) - 1 and top["counter"] == U64
    round_trip(gpu, t, ops, w, lead=5)


# ------------------------------------------------- offsets and sentinels
@pytest.mark.parametrize("t", TYPES)
def test_every_offset_residue_and_sentinel_buffers(gpu, t):
    from crdts_hip._lib import OP_ARRAYS_FIELDS, OpArraysC, OpWidthsC, lib

    tt = _torch()
    rng = random.Random(90 + t)
    w = (1, 2, 4, 8)
    ops = cases.random_ops(rng, t, w, 70)
    blobs = [ref.encode(t, op, w) for op in ops]
    want = cases.arrays_of(t, ops)
    # ingest: the first blob at offset 0, blob k at byte residue 7 k mod 16, the last ending on the last byte
    buf, off = bytearray(), []
    for k, b in enumerate(blobs):
        buf += bytes([SENTINEL] * ((7 * k - len(buf)) % 16))
        off.append(len(buf))
        buf += b
    assert off[0] == 0 and {o % 16 for o in off} == set(range(16)) and off[-1] + len(blobs[-1]) == len(buf)
    got = host(gpu.ops_from_bincode(u8(buf), i64(off), i64([len(b) for b in blobs]), t, w))
    assert got == lists(want)
    # egest into a sentinel-filled buffer: blob k at residue (3 + 5 k) mod 16, nothing else changes
    d = dev(want)
    n, n_clk = len(ops), len(want["clk_act"])
    ca = OpArraysC(*[p(d.get(f)) for f in OP_ARRAYS_FIELDS], n, n_clk)
    cw = OpWidthsC(*w)
    sizes = tt.zeros(n, dtype=tt.int64).cuda()
    assert lib.crdt_ops_bincode_sizes(gpu.ctx, t, C.byref(cw), C.byref(ca), p(sizes), None) == OK
    assert sizes.cpu().tolist() == [len(b) for b in blobs]
    exp, place = bytearray([SENTINEL] * rng.randrange(1, 17)), []
    for k, b in enumerate(blobs):
        exp += bytes([SENTINEL] * ((3 + 5 * k - len(exp)) % 16))
        place.append(len(exp))
        exp += b
    exp += bytes([SENTINEL] * 9)
    assert {o % 16 for o in place} == set(range(16))
    out = tt.full((len(exp),), SENTINEL, dtype=tt.uint8).cuda()
    assert lib.crdt_ops_to_bincode(gpu.ctx, t, C.byref(cw), C.byref(ca), p(out), p(i64(place)), len(exp), None) == OK
    assert status(gpu) == OK
    assert out.cpu().numpy().tobytes() == bytes(exp)
    # the last blob ending on the buffer's last byte
    tight = tt.full((place[-1] + len(blobs[-1]),), SENTINEL, dtype=tt.uint8).cuda()
    assert lib.crdt_ops_to_bincode(gpu.ctx, t, C.byref(cw), C.byref(ca), p(tight), p(i64(place)), int(tight.numel()),
                                   None) == OK
    assert status(gpu) == OK and tight.cpu().numpy().tobytes() == bytes(exp[:len(exp) - 9])


# ------------------------------------------------------ malformed: ingest
def assert_bad_op(t, got, j, code, want_good, goods_at):
    """Op j is the bad-op sentinel with `code`; the ops at goods_at equal want_good's (fields and pairs)."""
    assert got["op_err"][j] == code and [got["op_err"][k] for k in goods_at] == [0] * len(goods_at)
    end = got["clk_end"]
    if t == ref.MVREG:  # no kind array: the first pair of its span, if it has one
        b = end[j - 1] if j else 0
        if end[j] > b:
            assert (got["clk_act"][b], got["clk_ctr"][b]) == (0xFFFFFFFF, 0)
        assert got["val"][j] == 0
    else:
        assert got["kind"][j] == 0xFFFFFFFF
        assert all(got[f][j] == 0 for f in cases.USED[t] if f != "kind")
    wend = want_good["clk_end"].tolist()
    for k, g in zip(goods_at, range(len(goods_at))):
        for f in cases.USED[t]:
            assert got[f][k] == int(want_good[f][g]), (f, k)
        gb, wb = (end[k - 1] if k else 0), (wend[g - 1] if g else 0)
        n = wend[g] - wb
        assert end[k] - gb == n
        assert got["clk_act"][gb:gb + n] == want_good["clk_act"][wb:wb + n].tolist()
        assert got["clk_ctr"][gb:gb + n] == want_good["clk_ctr"][wb:wb + n].tolist()


@pytest.mark.parametrize("w", [(1, 1, 1, 1), (8, 8, 8, 8)])
@pytest.mark.parametrize("t", TYPES)
def test_ingest_malformed_between_good_neighbours(gpu, t, w):
    goods = cases.good_ops(t)
    gb = [ref.encode(t, op, w) for op in goods]
    want = cases.arrays_of(t, goods)
    for name, bad in cases.malformed(t, w).items():
        with pytest.raises(ref.FormatError):
            ref.decode(t, bad, w)
        got = ingest(gpu, t, [gb[0], bad, gb[1]], w, lead=3, check_status=False)
        assert status(gpu) == ENONCANON, name
        assert_bad_op(t, got, 1, ENONCANON, want, [0, 2])
    assert status(gpu) == OK  # the latch is cleared


@pytest.mark.parametrize("t", TYPES)
def test_ingest_blob_not_inside_the_buffer(gpu, t):
    goods = cases.good_ops(t)
    g = [ref.encode(t, op, W8) for op in goods]
    want = cases.arrays_of(t, goods)
    buf = g[0] + g[1]
    for off, ln in ((len(buf) - 4, len(g[0])), (len(buf) + 1, 0), (U64 - 3, len(g[0])), (0, U64), (8, U64 - 7)):
        a = gpu.ops_from_bincode(u8(buf), i64([0, off, len(g[0])]), i64([len(g[0]), ln, len(g[1])]), t, W8,
                                 op_err=True, check_status=False)
        assert status(gpu) == ENONCANON, (off, ln)
        assert_bad_op(t, host(a), 1, ENONCANON, want, [0, 2])


@pytest.mark.parametrize("t", TYPES)
def test_ingest_wrong_clk_end_span(gpu, t):
    """clk_end is the caller's: a span that is not the op's length, or that
    leaves [0, n_clk), is CRDT_ECAPACITY for that op alone."""
    from crdts_hip._lib import OP_ARRAYS_FIELDS, OpArraysC, OpWidthsC, lib

    tt = _torch()
    goods = cases.good_ops(t)
    ops = [goods[0], goods[0], goods[1]]
    w = (1, 1, 1, 1)
    buf, off, ln = ref.pack([ref.encode(t, op, w) for op in ops])
    want = cases.arrays_of(t, [goods[0], goods[1]])
    n1 = len(ref.pairs_of(t, goods[1]))
    untouched = 2 ** 32 - 7
    for ends, n_clk in (([2, 5, 5 + n1], 5 + n1),      # op 1: three pairs of room for a two-pair clock
                        ([2, 3, 3 + n1], 3 + n1),      # ... one
                        ([2, 1, 1 + n1], 2 + n1),      # a decreasing end
                        ([2, 4, 4 + n1], 3)):          # the right spans, but ops 1 and 2 leave [0, n_clk)
        d = {f: tt.full((3,), -1, dtype=tt.int32 if f in cases.U32 else tt.int64).cuda() for f in cases.USED[t]}
        d["clk_end"] = i64(ends)
        d["clk_act"] = tt.full((8,), -7, dtype=tt.int32).cuda()
        d["clk_ctr"] = tt.full((8,), -7, dtype=tt.int64).cuda()
        err = tt.zeros(3, dtype=tt.int32).cuda()
        ca = OpArraysC(*[p(d.get(f)) for f in OP_ARRAYS_FIELDS], 3, n_clk)
        assert lib.crdt_ops_from_bincode(gpu.ctx, p(u8(buf)), len(buf), p(i64(off)), p(i64(ln)), t,
                                         C.byref(OpWidthsC(*w)), C.byref(ca), p(err), None) == OK
        assert status(gpu) == ECAPACITY, ends
        got = host(dict(d, op_err=err))
        if ends[1] == 4:
            assert got["op_err"] == [0, ECAPACITY, ECAPACITY]
            assert got["clk_act"][:2] == want["clk_act"][:2].tolist() and got["clk_act"][2:] == [untouched] * 6
        elif ends[1] < ends[0]:  # (op 2's span [1, 1 + n1) then overlaps op 0's: only ops 0 and 1 are looked at)
            assert got["op_err"] == [0, ECAPACITY, 0]
        else:
            assert_bad_op(t, got, 1, ECAPACITY, want, [0, 2])
            assert got["clk_act"][n_clk:] == [untouched] * (8 - n_clk)  # nothing past n_clk


# ------------------------------------------------------- malformed: egest
def egest_cases(t, w):
    """name -> (arrays of three ops, the middle one unwritable)."""
    goods = cases.good_ops(t)
    base = cases.arrays_of(t, [goods[0], goods[0], goods[1]])
    wa, wk, w2, wv = w
    out = {}

    def mutate(name, **over):
        a = {f: x.copy() for f, x in base.items()}
        for f, v in over.items():
            if f in ("clk_act", "clk_ctr"):
                a[f][2 + v[0]] = v[1]  # a pair of op 1 (its span starts at pair 2)
            else:
                a[f][1] = v
        out[name] = a

    if t != ref.MVREG:
        mutate("unknown kind", kind=cases.N_KINDS[t])
        mutate("kind CRDT_OP_KIND_BAD", kind=0xFFFFFFFF)
    mutate("clock actor too wide", clk_act=(1, 1 << (8 * wa)))
    mutate("clock descends", clk_act=(1, 1))
    mutate("zero counter", clk_ctr=(0, 0))
    for f, width in (("key", wk), ("key2", w2), ("val", wv)):
        if f in cases.USED[t] and cases.fields_of(t, goods[0])[f]:
            mutate(f"{f} too wide", **{f: 1 << (8 * width)})
    if t != ref.MVREG and cases.fields_of(t, goods[0])["actor"]:
        mutate("dot actor too wide", actor=1 << (8 * wa))
    if t == ref.MAP_MAP:
        mutate("inner dot actor too wide", actor2=1 << (8 * wa))
    a = {f: x.copy() for f, x in base.items()}
    a["clk_end"][1] = 1  # below op 0's end
    out["clk_end decreasing"] = a
    return out


@pytest.mark.parametrize("t", TYPES)
def test_egest_malformed(gpu, t):
    w = (1, 1, 1, 1)
    goods = cases.good_ops(t)
    gb = [ref.encode(t, op, w) for op in goods]
    for name, a in egest_cases(t, w).items():
        out, off, lens = gpu.ops_to_bincode(t, w, dev(a), check_status=False)
        assert status(gpu) == ENONCANON, name
        got = blobs_of(out, off, lens)
        if name == "clk_end decreasing":  # op 2's span [1, ..) is then not its own clock either
            assert got[0] == gb[0] and got[1] == b"", name
        else:
            assert got == [gb[0], b"", gb[1]], name
    # pairs owned by a kind that carries no clock: the wire cannot say it
    for kind in range(cases.N_KINDS[t]):
        if kind in cases.CLOCKED[t]:
            continue
        rng = random.Random(kind)
        plain = cases.random_op(rng, t, w, kind=kind)
        a = cases.arrays_of(t, [goods[0], plain, goods[0]])
        assert egest(gpu, t, a, w) == [gb[0], ref.encode(t, plain, w), gb[0]]
        a["clk_end"][1] += 1  # op 1 now owns the first pair of op 2's clock
        out, off, lens = gpu.ops_to_bincode(t, w, dev(a), check_status=False)
        assert status(gpu) == ENONCANON, kind
        got = blobs_of(out, off, lens)
        assert got[0] == gb[0] and got[1] == b"" and lens.cpu().tolist()[1] == 0, kind
    # clk_end past n_clk
    a = cases.arrays_of(t, [goods[0], goods[0]])
    a["clk_end"][1] += 1
    out, off, lens = gpu.ops_to_bincode(t, w, dev(a), check_status=False)
    assert status(gpu) == ENONCANON and blobs_of(out, off, lens) == [gb[0], b""]


@pytest.mark.parametrize("t", TYPES)
def test_egest_blob_placed_past_out_bytes(gpu, t):
    from crdts_hip._lib import OP_ARRAYS_FIELDS, OpArraysC, OpWidthsC, lib

    tt = _torch()
    w = (1, 1, 1, 1)
    goods = cases.good_ops(t)
    gb = [ref.encode(t, op, w) for op in goods]
    d = dev(cases.arrays_of(t, [goods[0], goods[1], goods[0]]))
    ca = OpArraysC(*[p(d.get(f)) for f in OP_ARRAYS_FIELDS], 3, int(d["clk_act"].numel()))
    size = len(gb[0]) + len(gb[1]) + len(gb[0])
    place = [0, len(gb[0]), len(gb[0]) + len(gb[1]) + 1]  # the last blob ends one byte past out_bytes
    for placed, written in ((place, 2), ([0, len(gb[0]), U64 - 2], 2), ([0, size + 5, len(gb[0])], 1)):
        buf = tt.full((size + 16,), SENTINEL, dtype=tt.uint8).cuda()
        assert lib.crdt_ops_to_bincode(gpu.ctx, t, C.byref(OpWidthsC(*w)), C.byref(ca), p(buf), p(i64(placed)), size,
                                       None) == OK
        assert status(gpu) == ECAPACITY
        exp = bytearray([SENTINEL] * (size + 16))
        exp[:len(gb[0])] = gb[0]
        if written == 2:
            exp[len(gb[0]):len(gb[0]) + len(gb[1])] = gb[1]
        else:
            exp[len(gb[0]):2 * len(gb[0])] = gb[0]
        assert buf.cpu().numpy().tobytes() == bytes(exp)


# ------------------------------------------------------------- end to end
N_OBJ = 300
BAD_OBJ = 17


def wire_batch(gpu, t, per_obj, w, bad_obj=None):
    """per_obj op lists -> the op batch of the type, through the wire; bad_obj:
    the first op blob of that object loses its last byte."""
    flat = [op for ops in per_obj for op in ops]
    blobs = [ref.encode(t, op, w) for op in flat]
    ends = np.cumsum([len(ops) for ops in per_obj]).astype(np.uint64)
    if bad_obj is not None:
        j = int(ends[bad_obj - 1])
        assert ends[bad_obj] > j
        blobs[j] = blobs[j][:-1]
    buf, off, ln = ref.pack(blobs, lead=5, gap=1)
    return op_class(t).from_bincode(u8(buf), i64(off), i64(ln), ends, *class_widths(t, w), engine=gpu,
                                    check_status=bad_obj is None)


def rows_differ(a, b):
    """Per object: do two canonical host slabs (dicts of arrays) differ?"""
    n = len(next(iter(a.values())))
    d = np.zeros(n, bool)
    for f in a:
        d |= (np.asarray(a[f]) != np.asarray(b[f])).reshape(n, -1).any(axis=1)
    return d


def check_end_to_end(gpu, t, per_obj, apply, rows):
    """apply(ops) -> output; rows(output) -> dict of per-object host arrays."""
    import crdts_hip

    assert len(per_obj) == N_OBJ and per_obj[BAD_OBJ]
    want = rows(apply(op_class(t).from_lists(per_obj)))
    assert not rows_differ(rows(apply(wire_batch(gpu, t, per_obj, W8))), want).any()
    assert status(gpu) == OK
    ops = wire_batch(gpu, t, per_obj, W8, bad_obj=BAD_OBJ)
    assert status(gpu) == ENONCANON  # the ingest latched it
    got = apply(ops, check_status=False)
    with pytest.raises(crdts_hip.CrdtError) as e:  # ... and so does the object's apply
        gpu.status()
    assert e.value.code == ENONCANON
    keep = np.arange(N_OBJ) != BAD_OBJ
    assert not rows_differ(rows(got), want)[keep].any()


def test_end_to_end_orswot(gpu):
    import crdts_hip
    import records
    import kat_runner
    import opgen

    A, rng, be = 16, random.Random(0xE2E), kat_runner.PyBackend()
    objs, per_obj = [], []
    for _ in range(N_OBJ):
        o = be.new()
        for _, op in opgen.orswot_opvec(rng, max_len=20, actor_range=A, member_range=40):
            opgen.apply_op(be, o, op)
        objs.append(o)
        per_obj.append(orswot_wire_ops(opgen.orswot_opvec(rng, max_len=8, actor_range=A, member_range=40)) or
                       [("add", 1, 99, 5)])
    B = crdts_hip.OrswotBatch.from_records([records.from_py(o, A) for o in objs], A)

    def rows(out):
        recs = out.records()
        return {"record": np.array([hash(r) for r in recs], np.int64), "len": np.array([len(r) for r in recs])}

    # (the bad object's record is not written: records() of it is whatever the offset holds)
    check_end_to_end(gpu, ref.ORSWOT, per_obj, lambda ops, **kw: gpu.orswot_apply(B, ops, **kw), rows)


def test_end_to_end_mvreg(gpu):
    import mvreg_opgen as mo
    import test_gpu_mvreg_ops as tm

    A, cap = 8, 4
    b = mo.gen_batch(0xE2F, N_OBJ, A, cap, 3, 1, 8)
    S = tm._dev(mo.slab(b["regs0"], cap, A))

    def rows(out):
        n, clk, val = tm._host(out)
        return {"n": n, "clk": clk, "val": val}

    check_end_to_end(gpu, ref.MVREG, b["ops"],
                     lambda ops, **kw: gpu.mvreg_apply(S, ops, A, out=tm._patterned(N_OBJ, cap + 8, A), **kw), rows)


def _nonempty(batch):
    return [(pre, ops or [("nop",)]) for pre, ops in batch]


def test_end_to_end_map_mvreg(gpu, oracle):
    import map_opgen
    import test_gpu_map_apply as tm

    batch = _nonempty(map_opgen.gen_batch(0xE30, N_OBJ, tm.A))
    S, _ = map_opgen.oracle_slabs(oracle, batch, tm.A, tm.IN_CAPS, tm.OUT_CAPS)
    S = S.to("cuda")
    check_end_to_end(gpu, ref.MAP_MVREG, [ops for _, ops in batch],
                     lambda ops, **kw: gpu.map_mvreg_apply(S, ops, tm.A, out=tm._patterned(N_OBJ, tm.A, tm.OUT_CAPS),
                                                           **kw),
                     lambda out: out.canonical().a)


def test_end_to_end_map_orswot(gpu, oracle):
    import map_orswot_opgen as og
    import test_gpu_map_orswot_apply as tm

    batch = _nonempty(og.gen_batch(0xE31, N_OBJ, tm.A))
    S, _ = og.oracle_slabs(oracle, batch, tm.A, tm.IN_CAPS, tm.OUT_CAPS)
    S = S.to("cuda")
    check_end_to_end(gpu, ref.MAP_ORSWOT, [ops for _, ops in batch],
                     lambda ops, **kw: gpu.map_orswot_apply(S, ops, tm.A,
                                                            out=tm._patterned(N_OBJ, tm.A, tm.OUT_CAPS), **kw),
                     lambda out: out.canonical().a)


def test_end_to_end_map_map(gpu):
    import nested_opgen as ng
    import test_gpu_map_map_apply as tm

    batch, S, _ = ng.reference(0xE32, N_OBJ, tm.A)
    S = S.to("cuda")
    per_obj = [list(ops) or ["nop"] for _, ops in batch]

    def rows(out):
        c = out.canonical()
        inner = {"inner_" + f: np.asarray(v).reshape(N_OBJ, -1) for f, v in c.inner.a.items()}
        return dict(c.a, **inner)

    check_end_to_end(gpu, ref.MAP_MAP, per_obj,
                     lambda ops, **kw: gpu.map_map_apply(S, ops, tm.A,
                                                         out=tm._patterned(N_OBJ, tm.A, ng.OUT_CAPS, ng.OUT_INNER),
                                                         **kw), rows)


# ------------------------------------------------------- read -> op -> wire
def test_read_rm_clocks_to_the_wire(gpu):
    """contains(m).derive_rm_ctx() of a batch of reads, taken as they come out
    of crdt_orswot_read as an Rm batch, leaves the device as Op::Rm blobs."""
    import crdts_hip
    import records
    import test_gpu_read as tr

    tt = _torch()
    A, rng = 16, random.Random(43)
    objs = tr._seeded_orswots(78, 120, A)
    asked = [[rng.choice(sorted(o.entries) + [99]) for _ in range(rng.randrange(0, 4))] for o in objs]
    batch = crdts_hip.OrswotBatch.from_records([records.from_py(o, A) for o in objs], A)
    q = crdts_hip.ReadQueries.from_lists([[("key", m) for m in ms] for ms in asked])
    r = gpu.orswot_read(batch, q, want=("rm",))
    n, d = q.n_q, batch.off.device
    ops = crdts_hip.OrswotOps(q.t[0], tt.full((n,), crdts_hip.OrswotOps.RM, dtype=tt.int32, device=d), q.t[2],
                              tt.zeros(n, dtype=tt.int32, device=d), tt.zeros(n, dtype=tt.int64, device=d),
                              r["rm_end"], r["rm_act"], r["rm_ctr"])
    got = [ref.decode(ref.ORSWOT, b, (1, 0, 8, 0)) for b in blobs_of(*ops.to_bincode(1, 8, engine=gpu))]
    want = [("rm", m, sorted(o.contains_rm_clock(m).dots.items())) for o, ms in zip(objs, asked) for m in ms]
    assert got == want and any(w[2] for w in want) and any(not w[2] for w in want)
