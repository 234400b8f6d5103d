"""CPU: the bincode form of the Orswot, MVReg and Map ops
(tests/ops_bincode_ref.py) against the hand-derived golden blobs, its size
formulas and malformed classes, the four crdt_ops_* entry points' argument
checks (before any device work) and the host logic of the Python mirror."""
import ctypes as C
import random

import numpy as np
import pytest

import ops_bincode_cases as cases
import ops_bincode_ref as ref

NAMES = ["crdt_ops_bincode_clk_lens", "crdt_ops_from_bincode", "crdt_ops_bincode_sizes", "crdt_ops_to_bincode"]
TYPES = (ref.ORSWOT, ref.MVREG, ref.MAP_MVREG, ref.MAP_ORSWOT, ref.MAP_MAP)


# ------------------------------------------------------------ the format
def test_golden_ops_byte_for_byte():
    g = cases.golden()
    seen = set()
    for o in g:
        t, w, blob = ref.TYPES[o["type"]], o["widths"], bytes.fromhex(o["hex"])
        assert ref.encode(t, o["op"], w) == blob, o["name"]
        back = ref.decode(t, blob, w)
        assert ref.canon(back) == ref.canon(o["op"]), o["name"]
        assert ref.encode(t, back, w) == blob, o["name"]
        seen.add((t, ref.kind_of(t, o["op"]), tuple(w)))
    for t in TYPES:  # every variant of every type at all-1, all-8 and the mixed widths
        for k in range(cases.N_KINDS[t]):
            for w in ((1, 1, 1, 1), (8, 8, 8, 8), (1, 2, 4, 8)):
                assert (t, None if t == ref.MVREG else k, w) in seen, (t, k, w)


def test_worked_examples():
    g = {o["name"]: o for o in cases.golden()}
    add = bytes.fromhex("00000000" "03" "0500000000000000" "0900")
    assert len(add) == 15 and bytes.fromhex(g["worked_orswot_add"]["hex"]) == add
    assert ref.encode(ref.ORSWOT, ("add", 3, 5, 9), (1, 0, 2, 0)) == add
    up = bytes.fromhex("02000000" "01" "0700000000000000" "0A" "02000000" "02" "0300000000000000" "0B" "00000000"
                       "0100000000000000" "01" "0700000000000000" "2A")
    assert len(up) == 50 and bytes.fromhex(g["worked_nested_up"]["hex"]) == up
    op = cases.nested_up((1, 7), 10, cases.nested_up((2, 3), 11, cases.nested_put([(1, 7)], 42)))
    assert ref.encode(ref.MAP_MAP, op, (1, 1, 1, 1)) == up
    # the edges the fixtures pin
    assert ref.pairs_of(ref.ORSWOT, g["orswot_rm_empty_clock"]["op"]) == []
    assert len(ref.pairs_of(ref.MVREG, g["mvreg_put_three_pairs"]["op"])) == 3
    assert g["orswot_add_counter_max"]["op"][2] == (1 << 64) - 1
    assert g["orswot_add_actor_max"]["op"][1] == (1 << 32) - 1


def test_size_formulas_and_round_trip():
    from crdts_hip import ops_bincode as ob

    rng = random.Random(11)
    for t in TYPES:
        for w in cases.WIDTH_SETS:
            for _ in range(60):
                op = cases.random_op(rng, t, w)
                blob = ref.encode(t, op, w)
                kind, n = ref.kind_of(t, op), len(ref.pairs_of(t, op))
                assert len(blob) == ref.op_bytes(t, kind, n, w) == ob.op_blob_bytes(t, kind, n, w), (t, w, op)
                assert ref.canon(ref.decode(t, blob, w)) == ref.canon(op)
    # head + clock + tail, spelled out
    assert ref.op_bytes(ref.ORSWOT, 0, 0, (1, 0, 2, 0)) == 15
    assert ref.op_bytes(ref.ORSWOT, 1, 3, (2, 0, 4, 0)) == 4 + 8 + 3 * 10 + 4
    assert ref.op_bytes(ref.MVREG, None, 2, (4, 0, 0, 8)) == 4 + 8 + 2 * 12 + 8
    assert ref.op_bytes(ref.MAP_MVREG, 2, 1, (1, 2, 0, 4)) == 4 + 9 + 2 + 4 + 8 + 9 + 4
    assert ref.op_bytes(ref.MAP_ORSWOT, 2, 0, (1, 1, 1, 0)) == 4 + 9 + 1 + 4 + 9 + 1
    assert ref.op_bytes(ref.MAP_MAP, 2, 1, (1, 1, 1, 1)) == 50 and ref.op_bytes(ref.MAP_MAP, 4, 0, (8, 8, 8, 8)) == 32


@pytest.mark.parametrize("widths", [(1, 1, 1, 1), (8, 8, 8, 8)])
@pytest.mark.parametrize("op_type", TYPES)
def test_malformed_blobs_raise(op_type, widths):
    for op in cases.good_ops(op_type):
        assert ref.canon(ref.decode(op_type, ref.encode(op_type, op, widths), widths)) == ref.canon(op)
    bad = cases.malformed(op_type, widths)
    assert len(bad) >= 15
    for name, blob in bad.items():
        with pytest.raises(ref.FormatError):
            ref.decode(op_type, blob, widths)
            pytest.fail(f"{name}: decoded")


def test_malformed_classes_are_all_present():
    names = set(cases.malformed(ref.MAP_ORSWOT, (8, 8, 8, 8))) | set(cases.malformed(ref.MAP_MAP, (8, 8, 8, 8)))
    for cls in ("ends early", "trailing byte", "shorter than its variant word", "variant above the last",
                "variant with a high byte", "inner variant above the last", "length word 2^61",
                "length word too large by one", "descending actors", "duplicate actor", "zero counter",
                "clock actor 2^32", "dot actor 2^32", "dot mismatch: actor", "dot mismatch: counter",
                "inner dot actor 2^32", "put variant above the last"):
        assert cls in names, cls


def test_encode_rejects_what_the_wire_cannot_say():
    for op, w in ((("add", 256, 1, 0), (1, 0, 1, 0)), (("add", 1, 1, 256), (1, 0, 1, 0)),
                  (("rm", 1, [(2, 1), (1, 1)]), (1, 0, 1, 0)), (("rm", 1, [(1, 0)]), (1, 0, 1, 0)),
                  (("add", 1 << 32, 1, 0), (8, 0, 1, 0))):
        with pytest.raises(ref.FormatError):
            ref.encode(ref.ORSWOT, op, w)
    with pytest.raises(ref.FormatError):
        ref.encode(ref.MVREG, ([(1, 1)], 1 << 16), (1, 0, 0, 2))


def test_host_packing_matches_the_packers():
    """cases.arrays_of (a flat list) against the mirror's arrays_from_lists."""
    import crdts_hip

    rng = random.Random(3)
    for t, cls in ((ref.MVREG, crdts_hip.MVRegOps), (ref.MAP_MVREG, crdts_hip.MapOps),
                   (ref.MAP_ORSWOT, crdts_hip.MapOrswotOps), (ref.MAP_MAP, crdts_hip.MapMapOps)):
        from crdts_hip.ops_bincode import LAYOUT

        ops = cases.random_ops(rng, t, (4, 8, 8, 8), 40)
        got, want = cases.arrays_of(t, ops), cls.arrays_from_lists([ops[:7], [], ops[7:]])
        assert want[0].tolist() == [7, 7, 40]
        for f, x in zip(LAYOUT[cls.__name__][1], want[1:]):
            assert got[f].dtype == x.dtype and got[f].tolist() == x.tolist(), (t, f)


# ------------------------------------------------------- the entry points
def _buf(n=256):
    return C.cast(C.create_string_buffer(n), C.c_void_p)


def _stand_in():
    """A zeroed stand-in for a context: the checks come before its first use."""
    return C.cast(C.create_string_buffer(4096), C.c_void_p)


def _arrays(n_ops=1, n_clk=1, **over):
    from crdts_hip._lib import OP_ARRAYS_FIELDS, OpArraysC

    bufs = {f: _buf() for f in OP_ARRAYS_FIELDS}
    bufs.update(over)
    return OpArraysC(*[bufs[f] for f in OP_ARRAYS_FIELDS], n_ops, n_clk), bufs


def _call(which, ctx, t, w, a, b, n_ops=1):
    """Call `which` of the four (lens, from, sizes, to); b = blobs, off, len,
    lens, err, sizes, out, out_off. Only ever made with arguments the checks
    refuse, or with no ops: nothing here may reach a launch."""
    from crdts_hip._lib import lib

    blobs, off, ln, lens, err, sizes, out, ooff = b
    wp = None if w is None else C.byref(w)
    ap = None if a is None else C.byref(a)
    if which == 0:
        return lib.crdt_ops_bincode_clk_lens(ctx, blobs, 64, off, ln, n_ops, t, wp, lens, None)
    if which == 1:
        return lib.crdt_ops_from_bincode(ctx, blobs, 64, off, ln, t, wp, ap, err, None)
    if which == 2:
        return lib.crdt_ops_bincode_sizes(ctx, t, wp, ap, sizes, None)
    return lib.crdt_ops_to_bincode(ctx, t, wp, ap, out, ooff, 64, None)


def _all(ctx, t, w, a, b, n_ops=1):
    return [_call(k, ctx, t, w, a, b, n_ops) for k in range(4)]


def test_entry_points_exported_and_reject_a_null_ctx():
    """Fails without the feature: the four names are the contract."""
    import crdts_hip
    from crdts_hip._lib import OpWidthsC, lib

    for n in NAMES:
        assert n in crdts_hip.EXPORTS and hasattr(lib, n), n
    a, _ = _arrays()
    b = [_buf() for _ in range(8)]
    for t in TYPES:
        assert _all(None, t, OpWidthsC(1, 1, 1, 1), a, b) == [-1] * 4
    assert lib.crdt_abi_version() == 1


@pytest.mark.parametrize("op_type", TYPES)
def test_argument_checks(op_type):
    from crdts_hip._lib import OpWidthsC
    from crdts_hip.ops_bincode import USED_FIELDS, USED_WIDTHS, WIDTH_NAMES

    ctx = _stand_in()
    good_w = OpWidthsC(1, 2, 4, 8)
    a, bufs = _arrays()
    b = [_buf() for _ in range(8)]
    assert _all(ctx, op_type, None, a, b) == [-1] * 4  # null widths
    assert [_call(k, ctx, op_type, good_w, None, b) for k in (1, 2, 3)] == [-1] * 3  # a null arrays struct
    assert _all(ctx, 5, good_w, a, b) == [-1] * 4 and _all(ctx, 0xFFFFFFFF, good_w, a, b) == [-1] * 4
    z, _ = _arrays(0, 0)
    for k in range(4):  # a width outside {1, 2, 4, 8}: an error only where the type has the field
        for bad in (0, 3, 5, 16):
            w = OpWidthsC(1, 2, 4, 8)
            setattr(w, WIDTH_NAMES[k], bad)
            want = [-1] * 4 if k in USED_WIDTHS[op_type] else [0] * 4  # (no ops: checked all the same)
            assert _all(ctx, op_type, w, z, b, n_ops=0) == want, (k, bad)
    used = USED_FIELDS[op_type] + ("clk_end", "clk_act", "clk_ctr")
    for f in used:  # a null array the type uses (a pair array: with n_clk > 0)
        holed, _ = _arrays(**{f: None})
        assert [_call(k, ctx, op_type, good_w, holed, b) for k in (1, 2, 3)] == [-1] * 3, f
    # a null blob / result array; b[4] (d_op_err) may be null
    for hole, which in ((0, (0, 1)), (1, (0, 1)), (2, (0, 1)), (3, (0,)), (5, (2,)), (6, (3,)), (7, (3,))):
        p = list(b)
        p[hole] = None
        for k in which:
            assert _call(k, ctx, op_type, good_w, a, p) == -1, (hole, k)
    # an output array equal to an input array
    for f in used:
        if f != "clk_end":  # an ingest output that is d_blobs / d_blob_off / d_blob_len, or clk_end (an input there)
            for src in (b[0], b[1], b[2], bufs["clk_end"]):
                al, _ = _arrays(**{f: src, "clk_end": bufs["clk_end"]})
                assert _call(1, ctx, op_type, good_w, al, b) == -1, f
        p = list(b)
        p[5] = p[6] = bufs[f]  # d_sizes / d_out that is an op array
        assert [_call(k, ctx, op_type, good_w, a, p) for k in (2, 3)] == [-1, -1], f
    for which, dst, src in ((0, 3, 0), (0, 3, 1), (0, 3, 2), (1, 4, 1), (1, 4, 0), (3, 6, 7)):
        p = list(b)  # lens == a blob array; op_err == a blob array; out == out_off
        p[dst] = p[src]
        assert _call(which, ctx, op_type, good_w, a, p) == -1, (which, dst, src)
    # n_ops == 0: nothing to do, null arrays included
    z, _ = _arrays(0, 0, **{f: None for f in bufs})
    assert _all(ctx, op_type, good_w, z, [None] * 8, n_ops=0) == [0] * 4


# ------------------------------------------------------- the Python mirror
def test_mirror_host_logic():
    import crdts_hip
    from crdts_hip import ops_bincode as ob

    assert (ob.ORSWOT, ob.MVREG, ob.MAP_MVREG, ob.MAP_ORSWOT, ob.MAP_MAP) == (0, 1, 2, 3, 4)
    assert ob.KIND_BAD == 0xFFFFFFFF
    assert ob.check_widths(ob.ORSWOT, (1, 0, 2, 0)) == (1, 0, 2, 0)
    assert ob.check_widths(ob.MVREG, (8, None, 3, 1)) == (8, 0, 3, 1)  # unused widths are not checked
    for t, w in ((ob.ORSWOT, (1, 1, 3, 1)), (ob.MVREG, (1, 1, 1, 0)), (ob.MAP_MVREG, (1, 5, 1, 1)),
                 (ob.MAP_ORSWOT, (16, 1, 1, 1)), (ob.MAP_MAP, (1, 1, 0, 1)), (7, (1, 1, 1, 1))):
        with pytest.raises(crdts_hip.CrdtError):
            ob.check_widths(t, w)
    assert ob.op_blob_bytes(ob.ORSWOT, 0, 0, (1, 0, 2, 0)) == 15
    assert ob.op_blob_bytes(ob.MAP_MAP, 2, 1, (1, 1, 1, 1)) == 50
    assert ob.op_blob_bytes(ob.MVREG, 99, 0, (1, 0, 0, 1)) == 13  # no kind array: kind is ignored
    for t, kind, n in ((ob.ORSWOT, 2, 0), (ob.MAP_MVREG, 3, 0), (ob.MAP_ORSWOT, 4, 0), (ob.MAP_MAP, 5, 0),
                       (ob.ORSWOT, 0, 1), (ob.MAP_MVREG, 0, 1), (ob.MAP_ORSWOT, 2, 1), (ob.MAP_MAP, 4, 1)):
        with pytest.raises(crdts_hip.CrdtError):  # an unknown kind; pairs under a kind without a clock
            ob.op_blob_bytes(t, kind, n, (1, 1, 1, 1))
    for name in ("ops_clk_lens", "ops_from_bincode", "ops_to_bincode"):
        assert callable(getattr(crdts_hip.Engine, name))
    for cls in (crdts_hip.OrswotOps, crdts_hip.MVRegOps, crdts_hip.MapOps, crdts_hip.MapOrswotOps,
                crdts_hip.MapMapOps):
        assert callable(cls.from_bincode) and callable(cls.to_bincode)
        op_type, fields = ob.LAYOUT[cls.__name__]
        assert set(fields) == set(ob.USED_FIELDS[op_type]) | {"clk_end", "clk_act", "clk_ctr"}
    assert set(ob.USED_FIELDS[ob.MAP_MAP]) | {"clk_end", "clk_act", "clk_ctr"} == set(crdts_hip._lib.OP_ARRAYS_FIELDS)
    assert np.dtype(np.uint32).itemsize * 4 == C.sizeof(crdts_hip._lib.OpWidthsC)
    assert C.sizeof(crdts_hip._lib.OpArraysC) == 13 * 8
