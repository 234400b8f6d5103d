"""GPU parity: Causal::truncate of the three Map types, batched
(crdt_map_mvreg_truncate, crdt_map_orswot_truncate, crdt_map_map_truncate;
rust-crdt_amd/csrc/map_truncate.hip) — slab-row exact against the Python
restatement's Map.truncate (oracle/crdts_ref.py, src/map.rs:131-158; pinned on
the C++ oracle by tests/test_map_truncate_ref.py) over generated batches
(tests/map_truncgen.py), the kernel's own properties, the actor-width
boundaries, structures past one wave's lanes, hand-built deferred reorder /
collapse cases, composition with the merge and apply kernels, and the calls'
error contract (include/crdts_hip.h)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import map_slab
import map_truncgen as tg
import nested_opgen as ng
from map_slab import crdts_ref

pytestmark = pytest.mark.gpu
A = 16
SEED, CLOCK_SEED = 11, 5
PATTERN = 0x5A5A5A5A
KINDS = ("mvreg", "orswot", "nested")
N = {"mvreg": 2000, "orswot": 2000, "nested": 500}
VC = crdts_ref.VClock


# ------------------------------------------------------------------ per-type plumbing
def _alloc(kind, n, n_actors, caps, device=None):
    import crdts_hip

    if kind == "mvreg":
        return crdts_hip.MapSlab.alloc(n, n_actors, *caps, device=device)
    if kind == "orswot":
        return crdts_hip.MapOrswotSlab.alloc(n, n_actors, device=device, **caps)
    return crdts_hip.MapMapSlab.alloc(n, n_actors, *caps[0], caps[1], device=device)


def _arrays(kind, S):
    return list(S.a.values()) + (list(S.inner.a.values()) if kind == "nested" else [])


def _patterned(kind, n, n_actors, caps):
    """A device output slab holding a pattern: the kernels write only the used slots."""
    out = _alloc(kind, n, n_actors, caps, device="cuda")
    for v in _arrays(kind, out):
        v.fill_(PATTERN)
    return out


def _grown(kind, caps, by=3):
    if kind == "mvreg":
        return tuple(c + by for c in caps)
    if kind == "orswot":
        return {k: c + by for k, c in caps.items()}
    return tuple(c + by for c in caps[0]), tuple(c + by for c in caps[1])


def _rows_dev(clocks, n_actors):
    import torch

    return torch.from_numpy(tg.clock_rows(clocks, n_actors).view(np.int64)).cuda()


def _truncate(gpu, kind, S, clocks, n_actors, caps, out=None, **kw):
    """S (host or device) truncated by `clocks` into a patterned slab of `caps`."""
    S = S if hasattr(S.a["clock"], "data_ptr") else S.to("cuda")
    n = int(S.a["n_keys"].shape[0])
    out = out if out is not None else _patterned(kind, n, n_actors, caps)
    fn = {"mvreg": gpu.map_mvreg_truncate, "orswot": gpu.map_orswot_truncate, "nested": gpu.map_map_truncate}[kind]
    return fn(S, _rows_dev(clocks, n_actors), n_actors, out=out, **kw)


def _pack(kind, states, n_actors, caps):
    return tg.KINDS[kind]["pack"](states, n_actors, caps)


def _from_row(kind, S, i):
    return {"mvreg": map_slab.mvreg_map_from_row, "orswot": map_slab.orswot_map_from_row,
            "nested": map_slab.nested_map_from_row}[kind](S, i)


def _assert_rows(kind, got, exp, rows=None, what=""):
    """Canonical forms (slots past the counts zeroed) equal on `rows`."""
    if kind == "nested":
        return ng.assert_rows(got, exp, rows=rows, what=what)
    g, e = got.canonical(), exp.canonical()
    n = int(e.a["n_keys"].shape[0])
    rows = np.arange(n) if rows is None else np.asarray(rows)
    for f in e.a:
        d = (np.asarray(g.a[f]) != np.asarray(e.a[f])).reshape(n, -1).any(axis=1)[rows]
        bad = rows[np.nonzero(d)[0]]
        assert bad.size == 0, f"{what} {f}: {bad.size} objects differ, first {bad[:5].tolist()}"


def _pat(v):
    return np.asarray(v) == np.asarray(PATTERN).astype(v.dtype)


def _assert_pattern_kept(kind, got):
    """Every slot past a count still holds the pattern the slab was filled with."""
    import crdts_hip

    h = got.host()
    if kind != "nested":
        for f, m in h.used_masks().items():
            assert _pat(h.a[f])[~m].all(), f
        return
    a = h.a
    key = np.arange(h.kcap)[None, :] < a["n_keys"][:, None]
    dfr = np.arange(h.dcap)[None, :] < a["n_def"][:, None]
    dset = dfr[..., None] & (np.arange(h.scap)[None, None, :] < a["dset_n"][..., None])
    for f, m in (("keys", key), ("eclock", key[..., None]), ("dclock", dfr[..., None]), ("dset_n", dfr),
                 ("dset", dset)):
        assert _pat(a[f])[~np.broadcast_to(m, a[f].shape)].all(), f
    used = key.reshape(-1)
    for f, v in h.inner.a.items():
        assert _pat(v)[~used].all(), f"inner {f}: rows of unused key slots"
    sub = crdts_hip.MapSlab({f: v[used] for f, v in h.inner.a.items()}, *h.inner_caps)
    for f, m in sub.used_masks().items():
        assert _pat(sub.a[f])[~m].all(), f"inner {f}"


@functools.lru_cache(maxsize=None)
def _reference(kind, n, n_actors, seed=SEED, wide=False):
    """(states, modes, clocks, caps, S, E): the generated states, their clocks,
    the packed rows and the restatement's truncated rows — computed once."""
    states = tg.states_of(kind, seed, n, n_actors, wide)
    modes, clocks = tg.draw(CLOCK_SEED, states, n_actors)
    caps = tg.KINDS[kind]["caps"](states)
    S = _pack(kind, states, n_actors, caps)
    E = _pack(kind, [tg.truncated(m, T) for m, T in zip(states, clocks)], n_actors, caps)
    return states, modes, clocks, caps, S, E


# ------------------------------------------------------------------ 1. generated batch
@pytest.mark.parametrize("kind", KINDS)
def test_generated_batch(gpu, kind):
    """All four clock modes mixed, out capacities equal to self's: every row is
    the restatement's, the status is clean, unused slots keep the pattern."""
    states, modes, clocks, caps, S, E = _reference(kind, N[kind], A)
    assert all(modes.count(m) for m in tg.MODES)
    got = _truncate(gpu, kind, S, clocks, A, caps)
    _assert_rows(kind, got, E)
    _assert_pattern_kept(kind, got)
    h = got.host()
    for i in range(0, N[kind], 97):  # and read back as states
        assert _from_row(kind, h, i) == tg.truncated(states[i], clocks[i])


# ------------------------------------------------------------------ 2. properties on the kernel
@pytest.mark.parametrize("kind", KINDS)
def test_empty_clock_is_identity(gpu, kind):
    """prop_truncate_with_empty_vclock_is_nop (test/map.rs:732)."""
    states, _, _, caps, S, _ = _reference(kind, N[kind], A)
    got = _truncate(gpu, kind, S, [VC()] * len(states), A, caps)
    _assert_rows(kind, got, S)
    _assert_pattern_kept(kind, got)


@pytest.mark.parametrize("kind", KINDS)
def test_all_clock_empties_the_map(gpu, kind):
    states, _, _, caps, S, _ = _reference(kind, N[kind], A)
    assert (S.a["n_keys"] > 0).any() and (S.a["n_def"] > 0).any()
    T = VC([(a, tg.ALL) for a in range(A)])
    h = _truncate(gpu, kind, S, [T] * len(states), A, caps).host()
    assert not h.a["n_keys"].any() and not h.a["n_def"].any() and not h.a["clock"].any()


@pytest.mark.parametrize("kind", KINDS)
def test_truncate_twice(gpu, kind):
    """truncate(truncate(m, T1), T2): the second call reads the first call's
    output, whose unused slots hold the pattern."""
    states, _, c1, caps, S, _ = _reference(kind, N[kind], A)
    mid = [tg.truncated(m, T) for m, T in zip(states, c1)]
    _, c2 = tg.draw(CLOCK_SEED + 1, mid, A)
    E = _pack(kind, [tg.truncated(m, T) for m, T in zip(mid, c2)], A, caps)
    first = _truncate(gpu, kind, S, c1, A, caps)
    got = _truncate(gpu, kind, first, c2, A, caps)
    _assert_rows(kind, got, E)
    _assert_pattern_kept(kind, got)


# ------------------------------------------------------------------ 3. actor widths
@pytest.mark.parametrize("n_actors", [1, 64, 65, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_actor_widths(gpu, kind, n_actors):
    """One slot per lane up to 64 actors, two from 65."""
    states, modes, clocks, caps, S, E = _reference(kind, 200, n_actors, 0xB0 + n_actors, n_actors > 16)
    assert S.a["clock"][:, n_actors - 1].any()
    assert n_actors <= 64 or S.a["clock"][:, 64:].any()
    got = _truncate(gpu, kind, S, clocks, n_actors, caps)
    _assert_rows(kind, got, E)
    _assert_pattern_kept(kind, got)


# ------------------------------------------------------------------ 4. past one wave's lanes
def _clk(rng, n_actors=A, lo=1, hi=9, k=3):
    return VC([(a, rng.randrange(lo, hi)) for a in sorted(rng.sample(range(n_actors), k))])


def _deferred(rng, n, keys):
    d = {}
    while len(d) < n:
        d[_clk(rng)] = set(rng.sample(keys, rng.randrange(1, 4)))
    return d


def _big_mvreg(rng, nk, nd=40, nv=3):
    m = crdts_ref.Map(crdts_ref.MVReg)
    m.clock = VC([(a, 9) for a in range(A)])
    for key in range(100, 100 + nk):
        r = crdts_ref.MVReg()
        r.vals = [(_clk(rng), 1000 * key + v) for v in range(rng.randrange(1, nv + 1))]
        m.entries[key] = [_clk(rng), r]
    m.deferred = _deferred(rng, nd, list(range(90, 100 + nk)))
    return m


def _big_orswot(rng, nk, big_key_members=70, nd=70):
    m = crdts_ref.Map(crdts_ref.Orswot)
    m.clock = VC([(a, 9) for a in range(A)])
    for key in range(100, 100 + nk):
        o = crdts_ref.Orswot()
        o.clock = VC([(a, 8) for a in range(A)])
        members = range(1, 1 + (big_key_members if key == 101 else rng.randrange(0, 4)))
        o.entries = {x: _clk(rng) for x in members}
        o.deferred = _deferred(rng, 3 if key <= 102 else rng.randrange(0, 2), list(range(1, 80)))
        m.entries[key] = [_clk(rng), o]
    m.deferred = _deferred(rng, nd, list(range(90, 100 + nk)))
    return m


def _big_nested(rng, nk, inner_keys=70):
    m = crdts_ref.Map(lambda: crdts_ref.Map(crdts_ref.MVReg))
    m.clock = VC([(a, 9) for a in range(A)])
    for key in range(100, 100 + nk):
        m.entries[key] = [_clk(rng), _big_mvreg(rng, inner_keys if key == 101 else rng.randrange(0, 3), nd=3, nv=2)]
    m.deferred = _deferred(rng, 5, list(range(90, 100 + nk)))
    return m


def _big_case(kind):
    """(states, clocks): maps of 70 and 130 keys (nested: 70 outer keys, one
    inner map of 70) and clocks that drop some entries and deferred clocks and
    reduce others; the last clock is empty."""
    rng = random.Random(0x70)
    build = {"mvreg": _big_mvreg, "orswot": _big_orswot, "nested": _big_nested}[kind]
    states = [build(rng, nk) for nk in ((70, 70) if kind == "nested" else (70, 130, 70, 130))]
    clocks = [VC([(a, rng.randrange(1, 10)) for a in range(A) if rng.random() < 0.7]) for _ in states]
    clocks[-1] = VC()
    return states, clocks


@pytest.mark.parametrize("kind", KINDS)
def test_past_one_waves_lanes(gpu, kind):
    """Map<MVReg>: several values per entry and 40 deferred clocks; Map<Orswot>:
    a key with 70 members, nested deferred clocks and 70 map deferred clocks."""
    states, clocks = _big_case(kind)
    exp = [tg.truncated(m, T) for m, T in zip(states, clocks)]
    assert any(0 < len(e.entries) < len(m.entries) for m, e in zip(states, exp))
    assert any(0 < len(e.deferred) < len(m.deferred) for m, e in zip(states, exp))
    caps = tg.KINDS[kind]["caps"](states)
    got = _truncate(gpu, kind, _pack(kind, states, A, caps), clocks, A, caps)
    _assert_rows(kind, got, _pack(kind, exp, A, caps))
    _assert_pattern_kept(kind, got)


# ------------------------------------------------------------------ 5. hand-built deferred cases
# CLOCK ORDER before the subtract: D1 < D2 < D3 < D4 < D5
D1, D2, D3, D4, D5 = [(0, 3), (1, 4)], [(0, 5), (1, 1)], [(0, 6)], [(1, 4)], [(2, 1)]
T_HAND = [(0, 5), (2, 1)]
# less T: D1 -> {1:4}, D2 -> {1:1}, D3 -> {0:6}, D4 -> {1:4}, D5 -> empty (dropped).
#  - reorder: D2 < D3 before, {0:6} < {1:1} after;
#  - collapse: D1 and D4 both become {1:4}: D4 is the later one, its set is kept.
HAND_SETS = {1: {7, 8}, 2: {2}, 3: {3}, 4: {9}, 5: {5}}
HAND_EXPECT = [([(0, 6)], {3}), ([(1, 1)], {2}), ([(1, 4)], {9})]  # CLOCK ORDER


def _hand_deferred():
    return {VC(d): set(HAND_SETS[i + 1]) for i, d in enumerate((D1, D2, D3, D4, D5))}


def _hand_map(kind, level):
    inner = crdts_ref.Map(crdts_ref.MVReg)
    inner.clock = VC([(0, 9), (1, 9)])
    r = crdts_ref.MVReg()
    r.vals = [(VC([(0, 9)]), 1)]
    inner.entries[4] = [VC([(0, 9)]), r]
    if kind == "mvreg":
        m = inner
    elif kind == "orswot":
        m = crdts_ref.Map(crdts_ref.Orswot)
        m.clock = VC([(0, 9)])
        o = crdts_ref.Orswot()
        o.clock = VC([(0, 9)])
        o.entries[1] = VC([(0, 9)])
        m.entries[4] = [VC([(0, 9)]), o]
    else:
        m = crdts_ref.Map(lambda: crdts_ref.Map(crdts_ref.MVReg))
        m.clock = VC([(0, 9), (1, 9)])
        m.entries[6] = [VC([(1, 9)]), inner]
    (inner if level == "inner" else m).deferred = _hand_deferred()
    return m


@pytest.mark.parametrize("kind,level", [("mvreg", "map"), ("orswot", "map"), ("nested", "map"), ("nested", "inner")])
def test_hand_built_deferred_reorder_and_collapse(gpu, kind, level):
    m, T = _hand_map(kind, level), VC(T_HAND)
    caps = tg.KINDS[kind]["caps"]([m])
    got = _truncate(gpu, kind, _pack(kind, [m], A, caps), [T], A, caps).host()
    out = _from_row(kind, got, 0)
    d = (out.entries[6][1] if level == "inner" else out).deferred
    # stated by hand, in the slab's order
    assert [(tg.pairs(c), d[c]) for c in crdts_ref.clock_order(list(d))] == HAND_EXPECT
    g = (got.inner if level == "inner" else got).a
    assert int(g["n_def"][0]) == 3 and g["dclock"][0, :3, :2].tolist() == [[6, 0], [0, 1], [0, 4]]
    assert g["dset_n"][0, :3].tolist() == [1, 1, 1] and g["dset"][0, :3, 0].tolist() == [3, 2, 9]
    # and the restatement agrees on the whole row
    _assert_rows(kind, got, _pack(kind, [tg.truncated(m, T)], A, caps))


# ------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("kind", KINDS)
def test_truncate_then_merge(gpu, kind):
    """The truncated slabs merged with an untouched partner batch through
    crdt_map_*_merge equal the restatement's truncate-then-merge."""
    states, _, clocks, caps, S, _ = _reference(kind, N[kind], A)
    partners = tg.states_of(kind, SEED + 1, N[kind], A)
    pcaps = tg.KINDS[kind]["caps"](partners)
    exp = []
    for m, T, p in zip(states, clocks, partners):
        e = tg.truncated(m, T)
        e.merge(p)
        exp.append(e)
    tr = _truncate(gpu, kind, S, clocks, A, caps)
    O = _pack(kind, partners, A, pcaps).to("cuda")
    if kind == "mvreg":
        ocaps = tuple(a + b for a, b in zip(caps, pcaps))
        got = gpu.map_mvreg_merge(tr, O, A)
    elif kind == "orswot":
        ocaps = {k: caps[k] + pcaps[k] for k in caps}
        got = gpu.map_orswot_merge(tr, O, A)
    else:
        ocaps = tuple(tuple(a + b for a, b in zip(x, y)) for x, y in zip(caps, pcaps))
        got = gpu.map_map_merge(tr, O, A)
    _assert_rows(kind, got, _pack(kind, exp, A, ocaps))


def test_outer_rm_against_inner_truncate(gpu):
    """For `below` clocks, crdt_map_map_apply with one outer Rm{T, key} leaves at
    `key` an inner map equal to crdt_map_mvreg_truncate of that inner map by T:
    two kernels against each other, and against the restatement."""
    import crdts_hip

    states, modes, clocks, caps, S, _ = _reference("nested", N["nested"], A)
    (Sk, _, _), icaps = caps
    n = len(states)
    pick = [i for i in range(n) if modes[i] == "below" and states[i].entries]
    assert len(pick) > 100
    keys = {i: sorted(states[i].entries)[i % len(states[i].entries)] for i in pick}
    ops = [[{"rm": {"clock": [list(p) for p in tg.pairs(clocks[i])], "key": keys[i]}}] if i in keys else []
           for i in range(n)]
    out = _patterned("nested", n, A, caps)
    applied = gpu.map_map_apply(S.to("cuda"), crdts_hip.MapMapOps.from_lists(ops), A, out=out).host()
    # every inner row of self truncated by its object's clock
    inner_T = [clocks[r // Sk] for r in range(n * Sk)]
    trunc = _truncate(gpu, "mvreg", S.inner, inner_T, A, icaps).host()
    ca, ct = applied.inner.canonical(), trunc.canonical()
    checked = 0
    for i in pick:
        key, T = keys[i], clocks[i]
        ec = states[i].entries[key][0].clone()
        ec.subtract(T)
        after = _from_row("nested", applied, i)
        if ec.is_empty():
            assert key not in after.entries
            continue
        k = sorted(states[i].entries).index(key)
        k2 = sorted(after.entries).index(key)
        a_row, t_row = i * Sk + k2, i * Sk + k
        assert map_slab.rows_equal(ca, a_row, ct, t_row), i
        assert _from_row("mvreg", trunc, t_row) == tg.truncated(states[i].entries[key][1], T)
        checked += 1
    assert checked > 50


# ------------------------------------------------------------------ 7. capacities
@pytest.mark.parametrize("kind", KINDS)
def test_larger_out_capacities(gpu, kind):
    states, _, clocks, caps, S, _ = _reference(kind, N[kind], A)
    big = _grown(kind, caps)
    got = _truncate(gpu, kind, S, clocks, A, big)
    _assert_rows(kind, got, _pack(kind, [tg.truncated(m, T) for m, T in zip(states, clocks)], A, big))
    _assert_pattern_kept(kind, got)


# ------------------------------------------------------------------ 8. errors
def _call(gpu, kind, s, clk, r, n, n_actors, scratch=None, scratch_bytes=None, ctx="ctx"):
    """The C entry point itself; s / r: ctypes slab structs or None."""
    import crdts_hip

    L = crdts_hip._lib.lib
    ctx = gpu.ctx if ctx == "ctx" else None
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    p = C.c_void_p(clk.data_ptr()) if clk is not None else None
    if kind == "mvreg":
        return L.crdt_map_mvreg_truncate(ctx, ref(s), p, ref(r), n, n_actors, None)
    if kind == "orswot":
        return L.crdt_map_orswot_truncate(ctx, ref(s), p, ref(r), n, n_actors, None)
    sp = C.c_void_p(scratch.data_ptr()) if scratch is not None else None
    return L.crdt_map_map_truncate(ctx, ref(s), p, ref(r), n, n_actors, sp,
                                   scratch.numel() if scratch_bytes is None else scratch_bytes, None)


def _with(struct, **fields):
    """A copy of a ctypes slab struct with fields replaced ('inner.kcap' reaches the inner slab)."""
    c = type(struct).from_buffer_copy(struct)
    for f, v in fields.items():
        tgt = c
        *path, leaf = f.split(".")
        for p in path:
            tgt = getattr(tgt, p)
        setattr(tgt, leaf, v)
    return c


SELF_LIMITS = {"mvreg": dict(kcap=4096, mcap=128, dcap=64, scap=4096),
               "orswot": dict(kcap=4096, mcap=256, vdcap=256, vscap=256, dcap=256, scap=4096),
               "nested": {"kcap": 4096, "dcap": 64, "scap": 4096, "inner.kcap": 4096, "inner.mcap": 128,
                          "inner.dcap": 64, "inner.scap": 4096}}


@pytest.mark.parametrize("kind", KINDS)
def test_einval(gpu, kind):
    import torch

    import crdts_hip

    EINVAL = crdts_hip.CRDT_EINVAL
    caps = {"mvreg": (2, 2, 2, 2), "orswot": dict(kcap=2, mcap=2, vdcap=2, vscap=2, dcap=2, scap=2),
            "nested": ((2, 2, 2), (2, 2, 2, 2))}[kind]
    S, R = _alloc(kind, 2, A, caps, device="cuda"), _alloc(kind, 2, A, caps, device="cuda")
    s, r = S.cstruct(), R.cstruct()
    clk = torch.zeros((2, A), dtype=torch.int64, device="cuda")
    sc = torch.zeros(4096, dtype=torch.uint8, device="cuda") if kind == "nested" else None
    call = lambda s_=s, r_=r, clk_=clk, n=2, a=A, **kw: _call(gpu, kind, s_, clk_, r_, n, a,  # noqa: E731
                                                              scratch=kw.pop("scratch", sc), **kw)
    assert call() == crdts_hip.CRDT_OK  # the baseline every case below departs from
    gpu.status()
    assert call(ctx=None) == EINVAL
    assert call(s_=None) == EINVAL and call(r_=None) == EINVAL and call(clk_=None) == EINVAL
    assert call(a=0) == EINVAL and call(a=129) == EINVAL
    for f, lim in SELF_LIMITS[kind].items():  # self outside the merge's per-side limits
        assert call(s_=_with(s, **{f: 0})) == EINVAL, f
        assert call(s_=_with(s, **{f: lim + 1}), r_=_with(r, **{f: lim + 1})) == EINVAL, f
        assert call(r_=_with(r, **{f: 1})) == EINVAL, f  # out below self's
        assert call(r_=_with(r, **{f: 2 * lim + 1})) == EINVAL, f  # out above the apply's limit
    arrays = [f for f, _ in type(s)._fields_ if f not in SELF_LIMITS[kind] and f != "inner" and not f.endswith("cap")]
    for f in arrays:  # a null slab array
        assert call(s_=_with(s, **{f: None})) == EINVAL, f
        assert call(r_=_with(r, **{f: None})) == EINVAL, f
    if kind == "nested":
        assert call(s_=_with(s, **{"inner.keys": None})) == EINVAL
        assert call(r_=_with(r, **{"inner.mv_val": None})) == EINVAL
    assert call(r_=s) == EINVAL  # in place
    if kind == "nested":
        need = crdts_hip._lib.lib.crdt_map_map_truncate_scratch_bytes(C.byref(r), 2, A)
        assert 2 * 2 * 8 <= need <= sc.numel()
        assert call(scratch=None, scratch_bytes=0) == EINVAL
        assert call(scratch_bytes=need - 1) == EINVAL
        assert call(scratch_bytes=need) == crdts_hip.CRDT_OK
    if kind == "orswot":
        # the per-wave workspace is one nested set of SELF's capacities, by the apply's formula
        over = dict(mcap=256, vdcap=64, vscap=64)    # 8 * (256 * 17 + 64 * 80) + 4 * 384 = 77312 > 60672
        assert call(s_=_with(s, **over), r_=_with(r, **over)) == EINVAL
        ok = dict(mcap=200, vdcap=32, vscap=32)      # 8 * (200 * 17 + 32 * 48) + 4 * 264 = 40544
        assert call(s_=_with(s, **ok), r_=_with(r, **ok), n=0) == crdts_hip.CRDT_OK
        # out's own capacities do not count
        assert call(r_=_with(r, mcap=512, vdcap=512, vscap=512), n=0) == crdts_hip.CRDT_OK
    # n_obj == 0 is OK with null arrays
    null = _with(s, **{f: None for f in arrays})
    assert call(s_=null, r_=_with(r, **{f: None for f in arrays}), clk_=None, n=0, scratch=None,
                scratch_bytes=0) == crdts_hip.CRDT_OK
    gpu.status()


def _head(kind, X, n):
    """The first n objects of a host slab, copied."""
    import crdts_hip

    a = {f: np.array(v[:n]) for f, v in X.a.items()}
    if kind == "mvreg":
        return crdts_hip.MapSlab(a, X.kcap, X.mcap, X.dcap, X.scap)
    if kind == "orswot":
        return crdts_hip.MapOrswotSlab(a, X.caps)
    inner = crdts_hip.MapSlab({f: np.array(v[:n * X.kcap]) for f, v in X.inner.a.items()}, *X.inner_caps)
    return crdts_hip.MapMapSlab(a, X.kcap, X.dcap, X.scap, inner)


@pytest.mark.parametrize("kind,where", [("mvreg", "n_keys"), ("orswot", "n_keys"), ("nested", "n_keys"),
                                        ("nested", "inner_mv_n")])
def test_noncanonical_object(gpu, kind, where):
    """One object in 64 with a count above its capacity latches CRDT_ENONCANON;
    the other 63 rows are exact."""
    import crdts_hip

    states, _, clocks, caps, S, E = _reference(kind, N[kind], A)
    n, bad = 64, 13
    S64, E64 = _head(kind, S, n), _head(kind, E, n)
    if where == "n_keys":
        S64.a["n_keys"][bad] = S64.a["keys"].shape[1] + 1
    else:  # a surviving key whose inner map holds an entry: the second launch visits it
        bad, k = next((i, k) for i in range(n) for k in range(int(S64.a["n_keys"][i]))
                      if S64.a["keys"][i, k] in E64.a["keys"][i, :int(E64.a["n_keys"][i])]
                      and S64.inner.a["n_keys"][i * S64.kcap + k] > 0)
        S64.inner.a["mv_n"][bad * S64.kcap + k, 0] = S64.inner.mcap + 1
    got = _truncate(gpu, kind, S64, clocks[:n], A, caps, check_status=False)
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    _assert_rows(kind, got, E64, rows=[i for i in range(n) if i != bad], what=where)
    gpu.status()  # the latch is cleared: the context is usable again
