"""CPU: the bincode restatement of Map<K, Orswot> and of the nested map
(tests/nested_bincode_ref.py) — pinned by hand-derived blobs
(tests/golden/bincode_map_orswot.json, bincode_map_map.json), round trips with
every unordered container shuffled on every state the Map KATs and the
generators reach, the generated batches' coverage floors, and a FormatError
for every malformed blob the GPU ingest rejects."""
import json
import os
import random

import pytest

import map_kat_runner
import map_truncgen
import nested_bincode_cases as NC
import nested_bincode_ref as NB
from map_slab import crdts_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODEC = {"map_orswot": (NB.encode_map_orswot, NB.decode_map_orswot, NB.map_orswot_equal),
         "map_map": (NB.encode_map_map, NB.decode_map_map, NB.map_map_equal)}


def _vc(pairs):
    return crdts_ref.VClock([tuple(p) for p in pairs])


def _mvreg_map(st):
    m = crdts_ref.Map(crdts_ref.MVReg)
    m.clock = _vc(st["clock"])
    for key, ec, vals in st["entries"]:
        r = crdts_ref.MVReg()
        r.vals = [(_vc(c), v) for c, v in vals]
        m.entries[key] = [_vc(ec), r]
    for c, ks in st["deferred"]:
        m.deferred[_vc(c)] = set(ks)
    return m


def state_of(case):
    st = case["state"]
    if case["kind"] == "map_orswot":
        m = crdts_ref.Map(crdts_ref.Orswot)
        for key, ec, v in st["entries"]:
            o = crdts_ref.Orswot()
            o.clock = _vc(v["clock"])
            o.entries = {x: _vc(c) for x, c in v["members"]}
            o.deferred = {_vc(c): set(xs) for c, xs in v["deferred"]}
            m.entries[key] = [_vc(ec), o]
    else:
        m = map_kat_runner.nested_map()
        for key, ec, v in st["entries"]:
            m.entries[key] = [_vc(ec), _mvreg_map(v)]
    m.clock = _vc(st["clock"])
    for c, ks in st["deferred"]:
        m.deferred[_vc(c)] = set(ks)
    return m


def golden_cases(which=("bincode_map_orswot.json", "bincode_map_map.json")):
    out = []
    for name in which:
        with open(os.path.join(GOLDEN, name)) as f:
            out += json.load(f)["cases"]
    return out


def test_golden_covers_the_required_states():
    for name in ("bincode_map_orswot.json", "bincode_map_map.json"):
        cs = {c["name"]: c for c in golden_cases((name,))}
        assert len(cs) >= 5
        assert cs["empty_map"]["hex"] == "00" * 24
        assert any(not c["canonical"] for c in cs.values())
    o = {c["name"]: c for c in golden_cases(("bincode_map_orswot.json",))}
    # test_reset_remove_semantics (test/orswot.rs:270-307): the KAT's own end state
    (case,) = [c for c in map_kat_runner.load_cases() if c["name"] == "test_reset_remove_semantics"]
    end = map_kat_runner.run_case(case, map_kat_runner.PyMapBackend())
    assert NB.map_orswot_equal(state_of(o["reset_remove_semantics"]), end["m1"])
    assert sorted(end["m1"].entries[101][1].entries) == [2]
    a, b = o["two_members_nested_and_map_deferred"], o["two_members_out_of_order"]
    assert a["state"] == b["state"] and a["hex"] != b["hex"] and len(a["hex"]) == len(b["hex"])
    # a TestMap KAT state with an inner deferred remove
    m = {c["name"]: c for c in golden_cases(("bincode_map_map.json",))}
    (case,) = [c for c in map_kat_runner.load_cases(True) if c["name"] == "test_op_exchange_same_as_merge_quickcheck1"]
    end = map_kat_runner.run_case(case, map_kat_runner.PyMapBackend())["m1"]
    map_kat_runner.apply_raw(end, {"up": {"dot": [91, 10], "key": 216, "op": {"rm": {"clock": [[38, 5]], "key": 37}}}})
    assert end.entries[216][1].deferred
    assert NB.map_map_equal(state_of(m["kat_op_exchange_then_inner_deferred_remove"]), end)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["kind"] + "-" + c["name"])
def test_golden_blobs(case):
    enc, dec, eq = CODEC[case["kind"]]
    blob = bytes.fromhex(case["hex"])
    assert "".join(h for _, h in case["layout"]) == case["hex"]
    s = state_of(case)
    assert eq(dec(blob, *case["widths"]), s)
    assert (enc(s, *case["widths"]) == blob) == case["canonical"]
    assert len(enc(s, *case["widths"])) == len(blob)


class _Rec(map_kat_runner.PyMapBackend):
    """The Python backend, keeping every state an apply or a merge leaves."""

    def __init__(self):
        self.seen = []

    def _keep(self, m):
        self.seen.append(m.clone())

    def apply_up_add(self, m, *a):
        super().apply_up_add(m, *a)
        self._keep(m)

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


def kat_states(kind):
    """Every Map<_, Orswot> ("map_orswot") or TestMap ("map_map") state the Map KATs reach."""
    be = _Rec()
    for case in map_kat_runner.load_cases(kind == "map_map"):
        map_kat_runner.run_case(case, be)
    return [m for m in be.seen if kind == "map_map" or m.factory is crdts_ref.Orswot]


def _roundtrip(kind, states, widths, rng):
    enc, dec, eq = CODEC[kind]
    for s in states:
        for r in (None, rng):
            assert eq(dec(enc(s, *widths, rng=r), *widths), s)


@pytest.mark.parametrize("kind", ["map_orswot", "map_map"])
def test_roundtrip_kat_states(kind):
    states = kat_states(kind)
    assert len(states) >= (5 if kind == "map_orswot" else 10)  # one KAT has Orswot values: five states
    n = 3 if kind == "map_orswot" else 4
    _roundtrip(kind, states, (8,) * n, random.Random(1))
    _roundtrip(kind, states, (1,) * n, random.Random(2))  # the reference's own test types are u8


def orswot_states():
    return map_truncgen.states_of("orswot", 11, 2000, 16)


def nested_states():
    return map_truncgen.states_of("nested", 12, 2000, 16)


def test_generated_orswot_maps_roundtrip_and_cover():
    states = orswot_states()
    sets = lambda m: [o for _, o in m.entries.values()]  # noqa: E731
    # floors: half of what seed 11 gives (390, 267, 894, 401)
    assert sum(len(m.deferred) >= 2 for m in states) >= 195
    assert sum(any(o.deferred for o in sets(m)) for m in states) >= 133
    assert sum(any(len(o.entries) >= 2 for o in sets(m)) for m in states) >= 447
    assert sum(any(len(c.dots) >= 2 for o in sets(m) for c in o.entries.values()) for m in states) >= 200
    _roundtrip("map_orswot", states, (1, 8, 8), random.Random(4))


def test_generated_nested_maps_roundtrip_and_cover():
    states = nested_states()
    inner = lambda m: [v for _, v in m.entries.values()]  # noqa: E731
    # floors: half of what seed 12 gives (179, 211, 142)
    assert sum(len(m.deferred) >= 2 for m in states) >= 89
    assert sum(any(v.deferred for v in inner(m)) for m in states) >= 105
    assert sum(any(len(r.vals) >= 2 for v in inner(m) for _, r in v.entries.values()) for m in states) >= 71
    _roundtrip("map_map", states, (1, 8, 8, 8), random.Random(5))


def test_shuffle_changes_bytes_not_state():
    for case in golden_cases():
        if case["name"] not in ("two_members_nested_and_map_deferred", "empty_inner_map_two_outer_deferred"):
            continue
        enc, dec, eq = CODEC[case["kind"]]
        s, w = state_of(case), case["widths"]
        blobs = {enc(s, *w, rng=random.Random(k)) for k in range(32)}
        assert len(blobs) == (8 if case["kind"] == "map_orswot" else 2) and bytes.fromhex(case["hex"]) in blobs
        assert all(eq(dec(b, *w), s) for b in blobs)


def _malformed():
    return [(kind, name) for kind in ("orswot", "nested") for name in sorted(NC.malformed(kind, 16))]


def _decode(kind, blob):
    dec = NB.decode_map_orswot if kind == "orswot" else NB.decode_map_map
    return dec(blob, *NC.WIDTHS[kind])


@pytest.mark.parametrize("kind", ["orswot", "nested"])
def test_good_blob_and_length_positions(kind):
    blob, lens = NC.raw(kind, NC.WIDTHS[kind], NC.GOOD[kind])
    _decode(kind, blob)
    assert {label for _, label in lens} == NC.LENGTH_LABELS[kind]


@pytest.mark.parametrize("kind,name", _malformed())
def test_malformed_blobs_raise(kind, name):
    blob, why = NC.malformed(kind, 16)[name]
    if why is None:  # an actor >= n_actors: the restatement knows no n_actors
        _decode(kind, blob)
        return
    with pytest.raises(NB.FormatError, match=why):
        _decode(kind, blob)


def test_over_capacity_blobs_are_well_formed():
    caps = {"orswot": dict(kcap=2, mcap=3, vdcap=2, vscap=3, dcap=2, scap=3), "nested": ((2, 2, 3), (2, 3, 2, 3))}
    for kind in caps:
        blobs = NC.over_capacity(kind, caps[kind])
        assert len(blobs) == (6 if kind == "orswot" else 7)
        for blob in blobs.values():
            _decode(kind, blob)
