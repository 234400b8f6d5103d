"""GPU parity: crdt_mvreg_apply, crdt_mvreg_truncate and crdt_mvreg_read_clock
(rust-crdt_amd/csrc/mvreg_apply.hip) on the edge batches of
tests/mvreg_op_edges.py: counters on the u64 edges, every launch tier on both
sides of its boundary, op lists past the 64 staged headers, registers that
fill to out_cap with holes below, poison in the unused input slots. Whole
arrays are exact against the answers made with the batches (n, clk and val,
the zero-filled unused slots included), the outputs are pre-filled with a
pattern, every launch runs twice on the one engine, the status is clean and no
object is left out. Each test asserts the tier and the census of its batch
before it launches. That these batches tell a subtly wrong kernel from a right
one is tests/test_mvreg_op_edges.py's, without a GPU."""
import numpy as np
import pytest

import mvreg_op_edges as me
from test_gpu_mvreg_ops import PATTERN, _assert_slab, _dev, _host, _patterned
from test_mvreg_op_edges import CHAIN, COMPACT, FLOOR

pytestmark = pytest.mark.gpu


def _ops(P):
    import crdts_hip

    return crdts_hip.MVRegOps.from_arrays(*me.op_arrays(P))


def _copy(slab):
    return tuple(x.copy() for x in slab)  # (the shared batches are read-only)


def _apply_twice(gpu, S, P, E, A, out_cap, what):
    dS, ops = _dev(_copy(S)), _ops(P)
    for run in (1, 2):
        got = _host(gpu.mvreg_apply(dS, ops, A, out=_patterned(len(S[0]), out_cap, A)))
        gpu.status()
        _assert_slab(got, E, what=f"{what} apply, run {run}")
    _assert_slab(_host(dS), S, what=f"{what}: the input")  # not in place


def _census(b):
    """The tier and what the batch causes, before the launch."""
    c, name = b["census"], b["name"]
    assert b["tier"] == me.tier(b["A"], b["out_cap"]) and c["peak"] <= b["out_cap"]
    assert name.split("-")[0] in (f"A{b['A']}", "chain", "compact")
    if name in CHAIN:
        assert b["tier"] == "W4" and c["reloads"] >= 3 * FLOOR and min(c["staged"], c["unstaged"]) >= 1000
    if name in COMPACT:
        assert c["compact_mid"] >= 150 and c["peak"] == b["out_cap"]
        assert (b["tier"] == "general") == (name in ("compact-A5-cap70", "compact-A200-cap40"))
    if name == "A8-cap100":
        assert b["tier"] == "general" and c["over_64_used"] >= FLOOR


@pytest.mark.parametrize("name", me.NAMES)
def test_mvreg_apply_edges(gpu, name):
    b = me.batch(name)
    _census(b)
    _apply_twice(gpu, b["S"], b["P"], b["E"], b["A"], b["out_cap"], name)


@pytest.mark.parametrize("name", me.NAMES)
def test_mvreg_truncate_edges(gpu, name):
    """The truncating clocks are made of each register's own rows (its read
    clock, a stored row, a row with a hot slot one up or one down, all zero)."""
    b = me.batch(name)
    A, n, scap = b["A"], b["n"], b["scap"]
    T, E = me.truncate_batch(name)
    forms = {me.truncate_form(int(k), A) for k in b["S"][0]}
    assert (forms == {"lane_element"}) == (scap <= 64) and (len(forms) == 2 or name != "A8-cap100")
    assert (E[0] == 0).sum() >= FLOOR and (E[0] == b["S"][0]).sum() >= FLOOR and len(set(E[0].tolist())) >= 3
    dS, dT = _dev(_copy(b["S"])), _dev((T.copy(),))[0]
    for run in (1, 2):
        got = _host(gpu.mvreg_truncate(dS, dT, A, out=_patterned(n, scap, A)))
        gpu.status()
        _assert_slab(got, E, what=f"{name} truncate, run {run}")


@pytest.mark.parametrize("name", me.NAMES)
def test_mvreg_read_clock_edges(gpu, name):
    """The unused slots hold the poison word, above every counter but 2^64 - 1."""
    import torch

    b = me.batch(name)
    E = me.read_batch(name)
    assert (b["S"][0] == 0).any() or name in COMPACT
    dS = _dev(_copy(b["S"]))
    for run in (1, 2):
        out = torch.full((b["n"], b["A"]), PATTERN, dtype=torch.int64, device="cuda:0")
        got = gpu.mvreg_read_clock(dS, b["A"], out=out).cpu().numpy().view(np.uint64)
        gpu.status()
        bad = np.nonzero((got != E).any(axis=1))[0]
        assert bad.size == 0, f"{name} read clock, run {run}: {bad.size} objects differ, first {bad[:5].tolist()}"


def test_mvreg_apply_every_wave_three_objects(gpu):
    """The fast kernel loads an object's op bounds two objects ahead and its
    slots, values and op headers one ahead: here every wave of its largest
    grid (256 / W blocks of W waves per CU) takes at least three objects."""
    import torch

    b = me.batch(me.TILED)
    _census(b)
    assert b["tier"] == "W4"
    waves = me.fast_grid_waves(torch.cuda.get_device_properties(0).multi_processor_count)
    n = 3 * waves + 5
    assert (n + 3) // 4 > waves // 4 and n // waves >= 3  # more blocks wanted than the grid's cap
    S, P, E = me.tile(b, n)
    _apply_twice(gpu, S, P, E, b["A"], b["out_cap"], f"{me.TILED} x {n}")
