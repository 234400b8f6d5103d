"""CPU: the bincode restatement of MVReg / Map<K, MVReg> (tests/map_bincode_ref.py)
— pinned by hand-derived blobs (tests/golden/bincode_map_mvreg.json), round
trips on every state the KATs and the generators reach, and a FormatError for
every malformed blob the GPU ingest rejects."""
import json
import os
import random
import struct

import pytest

import map_bincode_ref as MB
import map_kat_runner
import map_opgen
import mvreg_opgen
from map_slab import crdts_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bincode_map_mvreg.json")


def _vc(pairs):
    return crdts_ref.VClock([tuple(p) for p in pairs])


def _reg(vals):
    r = crdts_ref.MVReg()
    r.vals = [(_vc(c), v) for c, v in vals]
    return r


def state_of(case):
    st = case["state"]
    if case["kind"] == "mvreg":
        return _reg(st["vals"])
    m = crdts_ref.Map(crdts_ref.MVReg)
    m.clock = _vc(st["clock"])
    for key, ec, vals in st["entries"]:
        m.entries[key] = [_vc(ec), _reg(vals)]
    for c, ks in st["deferred"]:
        m.deferred[_vc(c)] = set(ks)
    return m


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_covers_the_required_states():
    cs = {c["name"]: c for c in golden_cases()}
    assert cs["empty_map"]["hex"] == "00" * 24
    assert len(cs["mvreg_two_concurrent"]["state"]["vals"]) == 2
    two = cs["map_two_keys_one_empty_register"]["state"]
    assert len(two["entries"]) == 2 and any(not e[2] for e in two["entries"])
    for name, w in (("map_two_keys_two_deferred_u8", [1, 1, 1]), ("map_two_keys_two_deferred_u64", [8, 8, 8])):
        assert cs[name]["widths"] == w and len(cs[name]["state"]["deferred"]) == 2
        assert cs[name]["state"]["entries"] == two["entries"]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_golden_blobs(case):
    blob = bytes.fromhex(case["hex"])
    assert "".join(h for _, h in case["layout"]) == case["hex"]
    s = state_of(case)
    if case["kind"] == "mvreg":
        assert MB.encode_mvreg(s, *case["widths"]) == blob
        assert MB.mvreg_equal(MB.decode_mvreg(blob, *case["widths"]), s)
    else:
        assert MB.encode_map_mvreg(s, *case["widths"]) == blob
        assert MB.map_equal(MB.decode_map_mvreg(blob, *case["widths"]), s)


class _RecMaps(map_kat_runner.PyMapBackend):
    """The Python backend, keeping every Map<_, MVReg> state an apply or a merge
    leaves (a nested map's inner maps are such maps too)."""

    def __init__(self):
        self.seen = []

    def _keep(self, m):
        if m.factory is crdts_ref.MVReg:
            self.seen.append(m.clone())
        elif m.factory is not crdts_ref.Orswot:
            for _, v in m.entries.values():
                self.seen.append(v.clone())

    def apply_up_put(self, m, *a):
        super().apply_up_put(m, *a)
        self._keep(m)

    def apply_rm(self, m, *a):
        super().apply_rm(m, *a)
        self._keep(m)

    def apply_nested_put(self, m, *a):
        super().apply_nested_put(m, *a)
        self._keep(m)

    def apply_raw(self, m, op):
        super().apply_raw(m, op)
        self._keep(m)

    def merge(self, dst, src):
        super().merge(dst, src)
        self._keep(dst)


def kat_map_states():
    be = _RecMaps()
    for nested in (False, True):
        for case in map_kat_runner.load_cases(nested):
            map_kat_runner.run_case(case, be)
    return be.seen


class _RecRegs(mvreg_opgen.PyBackend):
    def __init__(self):
        self.seen = []

    def apply(self, reg, op):
        super().apply(reg, op)
        self.seen.append(reg.clone())

    def merge(self, reg, other):
        super().merge(reg, other)
        self.seen.append(reg.clone())


def kat_mvreg_states():
    be = _RecRegs()
    for case in mvreg_opgen.load_kats():
        mvreg_opgen.run_kat(case, be)
    return be.seen


def gen_map_states(seed, n, A, keys=map_opgen.KEYS, n_ops=12):
    """The maps map_opgen.gen_batch's objects end in (pre, then the stream)."""
    out = []
    for pre, ops in map_opgen.gen_batch(seed, n, A, keys, n_ops):
        m = crdts_ref.Map(crdts_ref.MVReg)
        for op in pre + ops:
            map_opgen.apply_op(m, op)
        out.append(m)
    return out


def _roundtrip_maps(states, widths, rng):
    for s in states:
        for r in (None, rng):
            assert MB.map_equal(MB.decode_map_mvreg(MB.encode_map_mvreg(s, *widths, rng=r), *widths), s)


def _roundtrip_regs(states, widths, rng):
    for s in states:
        for r in (None, rng):
            assert MB.mvreg_equal(MB.decode_mvreg(MB.encode_mvreg(s, *widths, rng=r), *widths), s)


def test_roundtrip_kat_map_states():
    states = kat_map_states()
    assert len(states) > 20 and any(s.deferred for s in states)
    _roundtrip_maps(states, (8, 8, 8), random.Random(1))
    _roundtrip_maps(states, (1, 1, 1), random.Random(2))  # the reference's own test types are u8


def test_roundtrip_kat_mvreg_states():
    states = kat_mvreg_states()
    assert len(states) > 10
    _roundtrip_regs(states, (8, 8), random.Random(3))


def test_roundtrip_generated_maps():
    states = gen_map_states(7, 2000, 16)
    assert sum(len(s.deferred) >= 2 for s in states) >= 20
    _roundtrip_maps(states, (1, 8, 8), random.Random(4))


def test_roundtrip_generated_registers():
    rng = random.Random(5)
    states = [mvreg_opgen.random_reg(rng, 16, 6, 1 << 40, val0=1000 * i) for i in range(2000)]
    _roundtrip_regs(states, (1, 8), random.Random(6))
    _roundtrip_regs(states[:200], (8, 4), random.Random(6))


def test_shuffled_deferred_order_changes_bytes_not_state():
    c = next(c for c in golden_cases() if c["name"] == "map_two_keys_two_deferred_u8")
    s, w = state_of(c), c["widths"]
    blobs = {MB.encode_map_mvreg(s, *w, rng=random.Random(k)) for k in range(16)}
    assert len(blobs) == 2 and bytes.fromhex(c["hex"]) in blobs
    assert all(MB.map_equal(MB.decode_map_mvreg(b, *w), s) for b in blobs)


def malformed_map_blobs():
    """name -> (blob, widths): one of every malformed kind, from the golden map
    with two deferred clocks at u8 widths."""
    c = next(c for c in golden_cases() if c["name"] == "map_two_keys_two_deferred_u8")
    w = tuple(c["widths"])
    good = bytes.fromhex(c["hex"])
    s = state_of(c)
    out = {"one_byte_short": good[:-1], "one_byte_extra": good + b"\0"}
    zc = bytearray(good)
    zc[9:17] = bytes(8)  # the map clock's first counter
    out["zero_counter"] = bytes(zc)
    # the two entries swapped: keys 9, 5
    e5 = good[34:34 + 1 + 17 + 8 + 8 + 9 + 1]
    e9 = good[34 + len(e5):34 + len(e5) + 1 + 17 + 8]
    assert e5[0] == 5 and e9[0] == 9 and MB.encode_map_mvreg(s, *w).startswith(good[:34] + e5 + e9)
    out["swapped_keys"] = good[:34] + e9 + e5 + good[34 + len(e5) + len(e9):]
    blob = bytearray(MB.encode_map_mvreg(s, *w))
    # rewrite the second deferred clock [(1,3)] -> {5} as a copy of the first ([(0,4),(1,1)] -> {5,9})
    d0 = 34 + len(e5) + len(e9) + 8
    first = bytes(blob[d0:d0 + 8 + 18 + 8 + 2])
    out["duplicate_deferred_clock"] = bytes(blob[:d0]) + first + first
    huge = bytearray(good)
    huge[0:8] = struct.pack("<Q", 1 << 63)
    out["length_word_2_63"] = bytes(huge)
    return {k: (v, w) for k, v in out.items()}


WHY = {"one_byte_short": "truncated|length word", "one_byte_extra": "trailing", "zero_counter": "zero counter",
       "swapped_keys": "^keys not strictly", "duplicate_deferred_clock": "duplicate deferred",
       "length_word_2_63": "length word"}


@pytest.mark.parametrize("name", sorted(WHY))
def test_malformed_map_blobs_raise(name):
    blob, w = malformed_map_blobs()[name]
    with pytest.raises(MB.FormatError, match=WHY[name]):
        MB.decode_map_mvreg(blob, *w)


@pytest.mark.parametrize("name", ["one_byte_short", "one_byte_extra", "zero_counter", "length_word_2_63"])
def test_malformed_mvreg_blobs_raise(name):
    c = next(c for c in golden_cases() if c["kind"] == "mvreg")
    good = bytearray.fromhex(c["hex"])
    bad = {"one_byte_short": good[:-1], "one_byte_extra": good + b"\0",
           "zero_counter": good[:17] + bytes(8) + good[25:],
           "length_word_2_63": struct.pack("<Q", 1 << 63) + good[8:]}[name]
    with pytest.raises(MB.FormatError, match=WHY[name]):
        MB.decode_mvreg(bytes(bad), *c["widths"])
