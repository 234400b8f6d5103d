"""CPU: the ground the batched Map::truncate tests stand on
(tests/test_gpu_map_truncate.py; crdt_map_mvreg_truncate,
crdt_map_orswot_truncate, crdt_map_map_truncate).

 - the generated batches (tests/map_truncgen.py) exercise every branch of
   Causal::truncate (src/map.rs:131-158) and of the nested values' truncates;
 - the restatement's Map.truncate (oracle/crdts_ref.py) is pinned on the C++
   oracle for every `below` object of the two flat types: with T <= the map
   clock nothing is deferred, so apply_rm(key, T) on every key is exactly the
   entry part of truncate (src/map.rs:343-349 against :134-141);
 - the new entry points validate their arguments without a GPU."""
import ctypes as C

import numpy as np
import pytest

import map_opgen
import map_orswot_opgen
import map_slab
import map_truncgen as tg
import oracle_ffi

A = 16
SEED, CLOCK_SEED = 11, 5
N = {"mvreg": 2000, "orswot": 2000, "nested": 500}

ALL_TYPES = ("entry_dropped", "entry_changed", "entry_unchanged", "entry_emptied", "def_dropped", "def_changed",
             "clock_partly")
PER_TYPE = {"mvreg": (), "orswot": ("member_dropped", "vdef_retired", "member_reduced"),
            "nested": ("inner_entry_dropped", "inner_def_changed")}
MAP_LEVEL = ("clock", "n_def", "dclock", "dset_n", "dset")
# whether the generated batch reaches the deferred collapse (two deferred clocks
# made equal); where it does not, the hand-built cases of the GPU file are the
# only cover
COLLAPSE = {"mvreg": True, "orswot": True, "nested": False}


def _batch(kind):
    states = tg.states_of(kind, SEED, N[kind], A)
    modes, clocks = tg.draw(CLOCK_SEED, states, A)
    return states, modes, clocks


@pytest.mark.parametrize("kind", ["mvreg", "orswot", "nested"])
def test_generator_coverage(kind):
    states, modes, clocks = _batch(kind)
    tot = {}
    for m, T in zip(states, clocks):
        for k, v in tg.events(m, T).items():
            tot[k] = tot.get(k, 0) + v
    for name in ALL_TYPES + PER_TYPE[kind]:
        assert tot[name] > 0, (kind, name, tot)
    if COLLAPSE[kind]:
        assert tot["collapse"] > 0, tot
    else:
        assert tot["collapse"] == 0, tot
    for mode in tg.MODES:
        assert modes.count(mode) > 0, mode
    assert modes.count("below") >= N[kind] // 2


def test_clock_modes():
    states, modes, clocks = _batch("mvreg")
    for m, mode, T in zip(states, modes, clocks):
        if mode == "below":
            assert T <= m.clock
        elif mode == "empty":
            assert T.is_empty()
        elif mode == "all":
            assert all(T.get(a) == tg.ALL for a in range(A))
    assert any(not (T <= m.clock) for m, mode, T in zip(states, modes, clocks) if mode == "mixed")


def test_empty_clock_is_identity_on_the_restatement():
    """prop_truncate_with_empty_vclock_is_nop (test/map.rs:732), all three types."""
    for kind in ("mvreg", "orswot", "nested"):
        for m in tg.states_of(kind, SEED, 200, A):
            assert tg.truncated(m, map_slab.crdts_ref.VClock()) == m


@pytest.mark.parametrize("kind", ["mvreg", "orswot"])
def test_restatement_pinned_on_the_oracle(kind):
    batch = (tg.mvreg_batch if kind == "mvreg" else tg.orswot_batch)(SEED, N[kind], A)
    states = [m for _, m in batch]
    modes, clocks = tg.draw(CLOCK_SEED, states, A)
    gen = map_opgen if kind == "mvreg" else map_orswot_opgen
    caps = tg.KINDS[kind]["caps"](states)
    capd = caps if kind == "orswot" else dict(zip(("kcap", "mcap", "dcap", "scap"), caps))
    pack = tg.KINDS[kind]["pack"]
    checked = 0
    for (ops, m), mode, T in zip(batch, modes, clocks):
        if mode != "below":
            continue
        h = oracle_ffi.OracleMap(kind)
        for op in ops:
            gen.apply_op_oracle(h, op)
        for key in sorted(m.entries):
            h.apply_rm(key, tg.pairs(T))
        got = h.slab(A, capd).canonical().a
        exp = pack([tg.truncated(m, T)], A, caps).canonical().a
        old = pack([m], A, caps).canonical().a
        for f in got:
            if f in MAP_LEVEL:  # the map clock and the deferred sets: unchanged
                assert np.array_equal(got[f], old[f]), (f, mode)
            else:  # keys, entry clocks, nested values: the restatement's truncate
                assert np.array_equal(got[f], exp[f]), (f, mode)
        checked += 1
    assert checked >= N[kind] // 2


# ------------------------------------------------------------------ validation without a GPU
def _lib():
    import crdts_hip

    return crdts_hip._lib.lib


def test_new_names_are_exported():
    import crdts_hip

    for name in ("crdt_map_mvreg_truncate", "crdt_map_orswot_truncate", "crdt_map_map_truncate_scratch_bytes",
                 "crdt_map_map_truncate"):
        assert name in crdts_hip.EXPORTS
        assert hasattr(_lib(), name)


def test_null_ctx_is_einval():
    import crdts_hip

    L = _lib()
    clk = np.zeros((1, A), np.uint64)
    p = C.c_void_p(clk.ctypes.data)
    S = crdts_hip.MapSlab.alloc(1, A, 2, 2, 2, 2)
    R = crdts_hip.MapSlab.alloc(1, A, 2, 2, 2, 2)
    s, r = S.cstruct(), R.cstruct()
    assert L.crdt_map_mvreg_truncate(None, C.byref(s), p, C.byref(r), 1, A, None) == crdts_hip.CRDT_EINVAL
    caps = map_orswot_opgen.caps(2)
    S = crdts_hip.MapOrswotSlab.alloc(1, A, **caps)
    R = crdts_hip.MapOrswotSlab.alloc(1, A, **caps)
    s, r = S.cstruct(), R.cstruct()
    assert L.crdt_map_orswot_truncate(None, C.byref(s), p, C.byref(r), 1, A, None) == crdts_hip.CRDT_EINVAL
    S = crdts_hip.MapMapSlab.alloc(1, A, 2, 2, 2, (2, 2, 2, 2))
    R = crdts_hip.MapMapSlab.alloc(1, A, 2, 2, 2, (2, 2, 2, 2))
    s, r = S.cstruct(), R.cstruct()
    sc = np.zeros(64, np.uint64)
    assert L.crdt_map_map_truncate(None, C.byref(s), p, C.byref(r), 1, A, C.c_void_p(sc.ctypes.data), sc.nbytes,
                                   None) == crdts_hip.CRDT_EINVAL
    assert L.crdt_map_map_truncate_scratch_bytes(None, 1, A) == 0
    assert L.crdt_map_map_truncate_scratch_bytes(C.byref(r), 100, A) >= 100 * 2 * 8
