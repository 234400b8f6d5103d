"""CPU: the clocks' bincode form (tests/clock_bincode_ref.py) against the
hand-derived golden blobs, its malformed classes, the nine
crdt_clock_*_bincode* entry points' argument checks (before any device work)
and the host logic of the Python mirror."""
import ctypes as C
import json
import os
import random

import pytest

import clock_bincode_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["crdt_clock_dense_from_bincode", "crdt_clock_dense_bincode_sizes", "crdt_clock_dense_to_bincode",
         "crdt_clock_csr_bincode_lens", "crdt_clock_csr_from_bincode", "crdt_clock_csr_bincode_sizes",
         "crdt_clock_csr_to_bincode", "crdt_clock_ops_from_bincode", "crdt_clock_ops_to_bincode"]


def golden():
    with open(os.path.join(REPO, "tests", "golden", "bincode_clocks.json")) as f:
        return json.load(f)


# ------------------------------------------------------------ the format
def test_golden_states_byte_for_byte():
    g = golden()
    assert len(g["states"]) >= 6
    for s in g["states"]:
        blob = bytes.fromhex(s["hex"])
        clocks = [dict(map(tuple, c)) for c in s["clocks"]]
        assert ref.encode_state(clocks, s["actor_bytes"]) == blob, s["name"]
        back = ref.decode_state(blob, s["actor_bytes"], s["kind"])
        assert back == [sorted(c.items()) for c in clocks], s["name"]
        assert ref.encode_state(back, s["actor_bytes"]) == blob


def test_golden_ops_byte_for_byte():
    for o in golden()["ops"]:
        blob = bytes.fromhex(o["hex"])
        assert ref.encode_op(o["actor"], o["counter"], o["actor_bytes"], o["dir"]) == blob, o["name"]
        assert len(blob) == ref.op_bytes(o["actor_bytes"], o["dir"] is not None)
        assert ref.decode_op(blob, o["actor_bytes"], o["dir"] is not None) == (o["actor"], o["counter"], o["dir"])


def test_issue_blob_sizes():
    g = {s["name"]: bytes.fromhex(s["hex"]) for s in golden()["states"]}
    assert len(g["vclock_u8_two"]) == 26 and len(g["pncounter_u8_p_only"]) == 25
    assert g["vclock_empty"] == bytes(8) and g["pncounter_empty"] == bytes(16)
    o = {s["name"]: bytes.fromhex(s["hex"]) for s in golden()["ops"]}
    assert len(o["dot_u16"]) == 10 and len(o["pn_op_u8_neg"]) == 13


def test_round_trip_random():
    rng = random.Random(5)
    for _ in range(300):
        ab = rng.choice([1, 2, 4, 8])
        kind = rng.choice(["vclock", "gcounter", "pncounter"])
        top = min(1 << (8 * ab), 1 << 32)
        clocks = [{rng.randrange(top): rng.choice([1, (1 << 64) - 1, rng.randrange(1, 1 << 40)])
                   for _ in range(rng.randrange(0, 12))} for _ in range(ref.n_clocks(kind))]
        blob = ref.encode_state(clocks, ab)
        assert len(blob) == 8 * len(clocks) + sum(map(len, clocks)) * (ab + 8)
        assert ref.decode_state(blob, ab, kind) == [sorted(c.items()) for c in clocks]
        row = ref.state_row(clocks, top) if top <= 256 else None
        if row is not None:
            assert ref.row_state(row, top) == clocks


def _q(v):
    return v.to_bytes(8, "little")


MALFORMED = {
    "zero counter": (_q(1) + b"\x01" + _q(0), 1, "vclock", None),
    "descending actors": (_q(2) + b"\x03" + _q(1) + b"\x01" + _q(1), 1, "vclock", None),
    "duplicate actor": (_q(2) + b"\x03" + _q(1) + b"\x03" + _q(2), 1, "vclock", None),
    "actor at the limit": (_q(1) + b"\x10" + _q(1), 1, "vclock", 16),
    "actor 2^32": (_q(1) + _q(1 << 32) + _q(1), 8, "vclock", 1 << 32),
    "ends early": ((_q(1) + b"\x01" + _q(1))[:-1], 1, "vclock", None),
    "ends inside the length word": (_q(0)[:-1], 1, "vclock", None),
    "trailing byte": (_q(1) + b"\x01" + _q(1) + b"\x00", 1, "vclock", None),
    "length word 2^63": (_q(1 << 63) + b"\x01" + _q(1), 1, "vclock", None),
    "length word 2^64-1": (_q((1 << 64) - 1) + b"\x01" + _q(1), 1, "vclock", None),
    "p swallows n": (_q(1) + b"\x01" + _q(1), 1, "pncounter", None),
    "p runs past the blob": (_q(3) + b"\x01" + _q(1) + _q(0), 1, "pncounter", None),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_state_raises(name):
    blob, ab, kind, limit = MALFORMED[name]
    with pytest.raises(ref.FormatError):
        ref.decode_state(blob, ab, kind, actor_limit=limit)


def test_boundary_actor_is_good():
    assert ref.decode_state(_q(1) + b"\x0f" + _q(1), 1, "vclock", actor_limit=16) == [[(15, 1)]]


def test_malformed_ops_raise():
    good = ref.encode_op(7, 1, 1, 1)
    assert ref.decode_op(good, 1, True) == (7, 1, 1)
    for d in (2, 0x100, 0x01000000):
        with pytest.raises(ref.FormatError):
            ref.decode_op(good[:9] + d.to_bytes(4, "little"), 1, True)
    with pytest.raises(ref.FormatError):
        ref.decode_op(ref.encode_op(1 << 32, 1, 8), 8)
    with pytest.raises(ref.FormatError):
        ref.decode_op(good[:-1], 1, True)
    with pytest.raises(ref.FormatError):
        ref.encode_op(1, 1, 1, 2)
    with pytest.raises(ref.FormatError):
        ref.encode_clock({1: 0}, 1)


# ------------------------------------------------------- the entry points
def _contexts():
    """A null context, and a zeroed stand-in for one (the checks come before
    the first use of the context)."""
    return [None, C.cast(C.create_string_buffer(4096), C.c_void_p)]


def _buf(n=256):
    return C.cast(C.create_string_buffer(n), C.c_void_p)


def test_entry_points_exported_and_reject_a_null_ctx():
    """Fails without the feature: the nine names are the contract."""
    import crdts_hip
    from crdts_hip._lib import ClockCsr, ClockCsrOut, lib

    for n in NAMES:
        assert n in crdts_hip.EXPORTS and hasattr(lib, n), n
    a, b, c, d, e = (_buf() for _ in range(5))
    s = ClockCsr(a, b, c, d, 1, 4)
    o = ClockCsrOut(a, b, c, d, 4)
    assert lib.crdt_clock_dense_from_bincode(None, a, 64, b, c, 1, 1, 16, 1, d, None) == -1
    assert lib.crdt_clock_dense_bincode_sizes(None, a, 1, 16, 1, 1, b, None) == -1
    assert lib.crdt_clock_dense_to_bincode(None, a, 1, 16, 1, 1, b, c, 64, None) == -1
    assert lib.crdt_clock_csr_bincode_lens(None, a, 64, b, c, 1, 1, 1, d, None, None) == -1
    assert lib.crdt_clock_csr_from_bincode(None, e, 64, e, e, 1, 1, 1, C.byref(o), None, None) == -1
    assert lib.crdt_clock_csr_bincode_sizes(None, C.byref(s), None, 1, e, None) == -1
    assert lib.crdt_clock_csr_to_bincode(None, C.byref(s), None, 1, e, e, 64, None) == -1
    assert lib.crdt_clock_ops_from_bincode(None, a, 9, 1, 1, 0, b, c, None, None) == -1
    assert lib.crdt_clock_ops_to_bincode(None, a, b, None, 1, 1, 0, c, 9, None) == -1
    assert lib.crdt_abi_version() == 1


def test_dense_argument_checks():
    from crdts_hip._lib import lib

    ctx = _contexts()[1]
    a, b, c, d = (_buf() for _ in range(4))
    f = lib.crdt_clock_dense_from_bincode
    for ab in (0, 3, 5, 16):
        assert f(ctx, a, 64, b, c, 1, ab, 16, 1, d, None) == -1
    assert f(ctx, a, 64, b, c, 1, 1, 0, 1, d, None) == -1  # n_actors == 0
    for nc in (0, 3):
        assert f(ctx, a, 64, b, c, 1, 1, 16, nc, d, None) == -1
    for hole in range(4):
        p = [a, b, c, d]
        p[hole] = None
        assert f(ctx, p[0], 64, p[1], p[2], 1, 1, 16, 1, p[3], None) == -1
    assert f(ctx, a, 64, b, c, 1, 1, 16, 1, a, None) == -1  # rows == blobs
    assert f(ctx, a, 64, b, c, 1, 1, 16, 1, b, None) == -1
    assert f(ctx, None, 0, None, None, 0, 1, 16, 2, None, None) == 0  # nothing to do
    g, h = lib.crdt_clock_dense_bincode_sizes, lib.crdt_clock_dense_to_bincode
    assert g(ctx, a, 1, 16, 1, 3, b, None) == -1 and g(ctx, a, 1, 0, 1, 1, b, None) == -1
    assert g(ctx, a, 1, 16, 3, 1, b, None) == -1 and g(ctx, a, 1, 16, 1, 1, None, None) == -1
    assert g(ctx, a, 1, 16, 1, 1, a, None) == -1 and g(ctx, None, 0, 16, 1, 1, None, None) == 0
    assert h(ctx, a, 1, 16, 1, 7, b, c, 64, None) == -1 and h(ctx, a, 1, 16, 1, 1, None, c, 64, None) == -1
    assert h(ctx, a, 1, 16, 1, 1, b, None, 64, None) == -1 and h(ctx, a, 1, 16, 1, 1, a, c, 64, None) == -1
    assert h(ctx, a, 1, 16, 1, 1, c, c, 64, None) == -1 and h(ctx, None, 0, 16, 2, 8, None, None, 0, None) == 0


def test_csr_argument_checks():
    from crdts_hip._lib import ClockCsr, ClockCsrOut, lib

    ctx = _contexts()[1]
    a, b, c, d, e, x, y, z, w = (_buf() for _ in range(9))
    f = lib.crdt_clock_csr_bincode_lens
    assert f(ctx, a, 64, b, c, 1, 3, 1, d, None, None) == -1
    assert f(ctx, a, 64, b, c, 1, 1, 0, d, None, None) == -1
    assert f(ctx, a, 64, b, c, 1, 1, 2, d, None, None) == -1  # n_clocks 2 needs d_len_n
    assert f(ctx, a, 64, b, c, 1, 1, 2, d, d, None) == -1
    assert f(ctx, a, 64, b, c, 1, 1, 1, b, None, None) == -1  # lens == blob_off
    assert f(ctx, None, 64, b, c, 1, 1, 1, d, None, None) == -1
    assert f(ctx, None, 0, None, None, 0, 1, 2, None, None, None) == 0
    g = lib.crdt_clock_csr_from_bincode
    o, o2 = ClockCsrOut(d, e, x, y, 4), ClockCsrOut(d, z, w, a, 4)
    assert g(ctx, a, 64, b, c, 1, 1, 1, None, None, None) == -1
    assert g(ctx, a, 64, b, c, 1, 1, 2, C.byref(o), None, None) == -1
    assert g(ctx, a, 64, b, c, 1, 2, 3, C.byref(o), None, None) == -1
    assert g(ctx, a, 64, b, c, 1, 1, 1, C.byref(ClockCsrOut(d, None, x, y, 4)), None, None) == -1
    assert g(ctx, a, 64, b, c, 1, 1, 1, C.byref(ClockCsrOut(d, d, x, y, 4)), None, None) == -1  # len == off (an input)
    assert g(ctx, a, 64, b, c, 1, 1, 1, C.byref(ClockCsrOut(d, e, a, y, 4)), None, None) == -1  # act == blobs
    assert g(ctx, a, 64, b, c, 1, 1, 2, C.byref(o), C.byref(o2), None) == -1  # n.ctr == blobs
    assert g(ctx, a, 64, b, c, 1, 1, 2, C.byref(o), C.byref(o), None) == -1
    assert g(ctx, None, 0, None, None, 0, 8, 2, None, None, None) == 0
    s, t = ClockCsr(a, b, c, d, 2, 4), ClockCsr(a, b, c, d, 3, 4)
    h, k = lib.crdt_clock_csr_bincode_sizes, lib.crdt_clock_csr_to_bincode
    assert h(ctx, None, None, 1, e, None) == -1 and h(ctx, C.byref(s), None, 3, e, None) == -1
    assert h(ctx, C.byref(s), C.byref(t), 1, e, None) == -1  # n_obj differ
    assert h(ctx, C.byref(s), None, 1, None, None) == -1 and h(ctx, C.byref(s), None, 1, c, None) == -1
    assert h(ctx, C.byref(ClockCsr(a, None, c, d, 2, 4)), None, 1, e, None) == -1
    assert h(ctx, C.byref(ClockCsr(None, None, None, None, 0, 0)), None, 1, None, None) == 0
    assert k(ctx, None, None, 1, e, x, 64, None) == -1 and k(ctx, C.byref(s), None, 5, e, x, 64, None) == -1
    assert k(ctx, C.byref(s), None, 1, None, x, 64, None) == -1 and k(ctx, C.byref(s), None, 1, e, None, 64, None) == -1
    assert k(ctx, C.byref(s), None, 1, d, x, 64, None) == -1 and k(ctx, C.byref(s), None, 1, e, e, 64, None) == -1
    assert k(ctx, C.byref(ClockCsr(None, None, None, None, 0, 0)), None, 1, None, None, 0, None) == 0


def test_ops_argument_checks():
    from crdts_hip._lib import lib

    ctx = _contexts()[1]
    a, b, c, d = (_buf() for _ in range(4))
    f, g = lib.crdt_clock_ops_from_bincode, lib.crdt_clock_ops_to_bincode
    for ab, wd in ((1, 0), (2, 0), (4, 1), (8, 1)):
        size = ab + 8 + 4 * wd
        assert f(ctx, a, size - 1, 1, ab, wd, b, c, d, None) == -1  # a stride below the op size
        assert g(ctx, b, c, d, 1, ab, wd, a, size - 1, None) == -1
        assert f(ctx, None, size, 0, ab, wd, None, None, None, None) == 0
        assert g(ctx, None, None, None, 0, ab, wd, None, size, None) == 0
    assert f(ctx, a, 16, 1, 3, 0, b, c, None, None) == -1 and g(ctx, b, c, None, 1, 3, 0, a, 16, None) == -1
    assert f(ctx, a, 16, 1, 1, 1, b, c, None, None) == -1  # with_dir needs d_dir
    assert g(ctx, b, c, None, 1, 1, 1, a, 16, None) == -1
    assert f(ctx, None, 16, 1, 1, 0, b, c, None, None) == -1 and f(ctx, a, 16, 1, 1, 0, None, c, None, None) == -1
    assert f(ctx, a, 16, 1, 1, 0, b, None, None, None) == -1
    assert f(ctx, a, 16, 1, 1, 0, a, c, None, None) == -1 and f(ctx, a, 16, 1, 1, 0, b, b, None, None) == -1
    assert f(ctx, a, 16, 1, 1, 1, b, c, b, None) == -1
    assert g(ctx, a, c, None, 1, 1, 0, a, 16, None) == -1 and g(ctx, b, a, None, 1, 1, 0, a, 16, None) == -1
    assert g(ctx, b, c, a, 1, 1, 1, a, 16, None) == -1


# ------------------------------------------------------- the Python mirror
def test_mirror_host_logic():
    import torch

    import crdts_hip
    from crdts_hip import clock_bincode as cb

    assert [cb.n_clocks(k) for k in ("vclock", "gcounter", "pncounter")] == [1, 1, 2]
    with pytest.raises(crdts_hip.CrdtError):
        cb.n_clocks("orswot")
    assert cb.op_blob_bytes(2) == 10 and cb.op_blob_bytes(1, True) == 13
    with pytest.raises(crdts_hip.CrdtError):
        cb.op_blob_bytes(3)
    assert cb.clock_blob_bytes(2, 1) == 26 and cb.clock_blob_bytes(1, 1, "pncounter") == 25
    assert cb.clock_blob_bytes(0, 8, "pncounter") == 16
    off, total = cb.place(torch.tensor([3, 0, 5], dtype=torch.int32))
    assert off.tolist() == [0, 3, 3] and total == 8 and off.dtype == torch.int64
    off, total = cb.place(torch.tensor([3, 0, 5], dtype=torch.int32), gap=2)
    assert off.tolist() == [0, 5, 7] and total == 14
    assert cb.place(torch.zeros(0, dtype=torch.int32))[1] == 0
    assert cb.ops_extent(0, 16, 9) == 0 and cb.ops_extent(3, 16, 9) == 41 and cb.ops_extent(1, 9, 9) == 9
    with pytest.raises(crdts_hip.CrdtError):
        cb.ops_extent(3, 8, 9)
    for name in ("clock_from_bincode", "clock_to_bincode", "clock_csr_from_bincode", "clock_csr_to_bincode",
                 "clock_ops_from_bincode", "clock_ops_to_bincode"):
        assert callable(getattr(crdts_hip.Engine, name))
    assert callable(crdts_hip.ClockOps.from_bincode) and callable(crdts_hip.ClockOps.to_bincode)


def test_mirror_sizes_agree_with_the_restatement():
    from crdts_hip import clock_bincode as cb

    rng = random.Random(9)
    for _ in range(50):
        ab = rng.choice([1, 2, 4, 8])
        kind = rng.choice(["vclock", "pncounter"])
        clocks = [{a: 1 for a in rng.sample(range(200), rng.randrange(0, 9))} for _ in range(ref.n_clocks(kind))]
        assert cb.clock_blob_bytes(sum(map(len, clocks)), ab, kind) == len(ref.encode_state(clocks, ab))
        assert cb.op_blob_bytes(ab, kind == "pncounter") == ref.op_bytes(ab, kind == "pncounter")
