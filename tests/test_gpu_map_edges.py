"""GPU parity of the nine Map kernels at u64 and key edges:
crdt_map_{mvreg,orswot,map}_merge, _truncate and _apply on the batches of
tests/map_edge_cases.py — op-simulated states whose counters, keys, members,
inner keys and values a monotone lift (tests/map_lift.py) has moved onto the
edges of u64: counters around 2^32, 2^63 and at 2^64 - 1, counters that differ
in one word only, keys 0 and 2^64 - 1 (the key walks' "side exhausted"
sentinel), keys that share a word, keys on both sides of 2^63.
tests/test_map_lift.py proves without a GPU that the lift commutes with every
oracle used here and that these inputs tell a right kernel from the wrong
ones of map_lift.VCLOCK_MUTANTS and map_lift.KEY_MUTANTS.

Bar: canonical-form exact against each entry point's own oracle, no object
left out; the output slab pre-filled with a pattern; merges in both
orientations; every launch made twice on one engine."""
import numpy as np
import pytest

import map_edge_cases as mc
import map_tiergen as mt

pytestmark = pytest.mark.gpu
PATTERN = 0x5A5A5A5A
WIDTHS = (16, 100)
MERGE_WIDTHS = mc.MERGE_WIDTHS


def _arrays(kind, S):
    return list(S.a.values()) + (list(S.inner.a.values()) if kind == "nested" else [])


def _patterned(kind, n, A, caps):
    out = mc.alloc(kind, n, A, caps, device="cuda")
    for v in _arrays(kind, out):
        v.fill_(PATTERN)
    return out


def _same(kind, got, exp, what):
    bad = mc.rows_differ(kind, got, exp)
    assert bad.size == 0, f"{what}: {bad.size} / {exp.a['n_keys'].shape[0]} objects differ, first {bad[:5].tolist()}"


def _merge_twice(gpu, kind, S, O, exp, A, what):
    """self ⊔ other into a pre-filled output of the summed capacities (the oracle's), twice on one engine."""
    fn = {"mvreg": gpu.map_mvreg_merge, "orswot": gpu.map_orswot_merge, "nested": gpu.map_map_merge}[kind]
    Sd, Od = S.to("cuda"), O.to("cuda")
    for k in range(2):
        out = _patterned(kind, int(S.a["n_keys"].shape[0]), A, mc.caps_of(kind, exp))
        _same(kind, fn(Sd, Od, A, out=out), exp, f"{what}, launch {k}")


# ------------------------------------------------------------------ value batches
@pytest.mark.parametrize("A", MERGE_WIDTHS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_merge_edges(gpu, oracle, kind, A):
    """The replica pairs of the existing random-parity tests (plus a third
    replica's removes at and ahead of the merged clock), lifted, at one slot
    per lane (2, 16, 63, 64 actors) and two (65, 100, 128)."""
    c = mc.merge_case(kind, A)
    mc.assert_merge_batch(kind, A)
    _merge_twice(gpu, kind, c["S"], c["O"], c["SO"], A, f"{kind} A={A} self ⊔ other")
    _merge_twice(gpu, kind, c["O"], c["S"], c["OS"], A, f"{kind} A={A} other ⊔ self")


@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_truncate_edges(gpu, kind, A):
    """States and truncating clocks of tests/map_truncgen.py under one lift:
    the clock's counters sit below, at and above the states' on the same edges."""
    import torch

    c = mc.truncate_case(kind, A)
    fn = {"mvreg": gpu.map_mvreg_truncate, "orswot": gpu.map_orswot_truncate, "nested": gpu.map_map_truncate}[kind]
    S, rows = c["S"].to("cuda"), torch.from_numpy(c["rows"].view(np.int64)).cuda()
    assert (c["rows"] >= np.uint64(2**63)).any() and mc.rows_differ(kind, c["S"], c["E"]).size > 0.6 * len(c["states"])
    for k in range(2):
        out = _patterned(kind, len(c["states"]), A, c["caps"])
        _same(kind, fn(S, rows, A, out=out), c["E"], f"{kind} A={A} truncate, launch {k}")


@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_apply_edges(gpu, oracle, kind, A):
    """The op streams of map_opgen / map_orswot_opgen / nested_opgen with
    their start states under one lift: dots at, below and above the clock's
    counter on the edges, removes whose clocks tie with entry clocks there."""
    import crdts_hip

    c = mc.apply_case(kind, A)
    ops = {"mvreg": crdts_hip.MapOps, "orswot": crdts_hip.MapOrswotOps, "nested": crdts_hip.MapMapOps}[kind] \
        .from_lists(c["ops"])
    fn = {"mvreg": gpu.map_mvreg_apply, "orswot": gpu.map_orswot_apply, "nested": gpu.map_map_apply}[kind]
    S = c["S"].to("cuda")
    assert mc.rows_differ(kind, c["E"], mc.apply_case(kind, A, lifted=False)["E"]).size > 0.9 * len(c["ops"])
    for k in range(2):
        out = _patterned(kind, len(c["ops"]), A, c["caps"][1])
        _same(kind, fn(S, ops, A, out=out), c["E"], f"{kind} A={A} apply, launch {k}")


# ------------------------------------------------------------------ tier batches
@pytest.mark.parametrize("name", list(mt.TIER_BATCHES))
def test_merge_tier_edges(gpu, oracle, name):
    """The merge launchers' boundaries (map_tiergen.TIER_BATCHES), lifted too,
    each at its limit and one past it: the Map<MVReg> value-row stage on and
    off at mcap * A = 128 | 129 (A = 16, 64, 1) with keys that fill it exactly
    and keys at 64 | 65 rows; the deferred-set stage at 128 | 129 u64; 63 / 64
    / 65 keys a side; 64 deferred clocks a side, all surviving; 128 kept
    values a side in one key; the Map<Orswot> workspace at 64 KB with its
    members, nested deferred clocks and member sets full, and its map
    deferred sets staged, past the staging limit, and pushed out by the
    workspace; the nested map's outer keys of one side, of both with an empty
    and a non-empty truncating row, its outer deferred stage, 63 / 64 / 65
    outer keys; 64 | 65 actors. Every batch asserts its tier census
    (map_lift.tier_*, map_tiergen.EXPECT)."""
    c = mt.tier_case(name)
    mt.assert_tiers(name)
    _merge_twice(gpu, c["kind"], c["S"], c["O"], c["SO"], c["A"], f"{name} self ⊔ other")
    _merge_twice(gpu, c["kind"], c["O"], c["S"], c["OS"], c["A"], f"{name} other ⊔ self")
