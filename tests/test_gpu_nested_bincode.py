"""GPU parity of the bincode codec of Map<K, Orswot<M, A>, A> and of the nested
map Map<K, Map<K2, MVReg<V, A>, A>, A> (crdt_map_orswot_{from,to}_bincode,
crdt_map_map_{from,to}_bincode) against the format restatement
(tests/nested_bincode_ref.py) and the slab renderings of tests/map_slab.py:
byte-exact slabs from blobs whose unordered containers are shuffled and which
lie at any byte alignment, byte-exact blobs from slabs, every integer width,
the edges of the capacities, of the rank loops and of the LDS stage window,
malformed input, and blobs -> merge -> blobs on the device against the
restatement's merge."""
import ctypes as C
import random

import numpy as np
import pytest

import map_slab
import map_truncgen
import nested_bincode_cases as NC
import nested_bincode_ref as NB
from map_slab import crdts_ref

pytestmark = pytest.mark.gpu

A16 = 16
PATTERN = 0x5A5A5A5A
LDS_WINDOW = 4096        # the ingest kernels' per-wave stage window (csrc/map_bincode.hip, kStage)
U64MAX = (1 << 64) - 1
KINDS = ("orswot", "nested")
W8 = {"orswot": (8, 8, 8), "nested": (8, 8, 8, 8)}


# ------------------------------------------------------------------ the two types behind one face
def enc(kind, m, w, rng=None):
    return (NB.encode_map_orswot if kind == "orswot" else NB.encode_map_map)(m, *w, rng=rng)


def dec(kind, blob, w):
    return (NB.decode_map_orswot if kind == "orswot" else NB.decode_map_map)(blob, *w)


def caps_of(kind, states):
    return map_truncgen.KINDS[kind]["caps"](states)


def alloc(kind, n, A, caps, device=None):
    import crdts_hip

    if kind == "orswot":
        return crdts_hip.MapOrswotSlab.alloc(n, A, device=device, **caps)
    return crdts_hip.MapMapSlab.alloc(n, A, *caps[0], caps[1], device=device)


def pack(kind, states, A, caps):
    S = alloc(kind, len(states), A, caps)
    put = map_slab.orswot_map_to_row if kind == "orswot" else map_slab.nested_map_to_row
    for i, m in enumerate(states):
        put(m, S, i, A, zero=False)
    return S


def patterned(kind, n, A, caps):
    out = alloc(kind, n, A, caps, device="cuda:0")
    for v in list(out.a.values()) + (list(out.inner.a.values()) if kind == "nested" else []):
        v.fill_(PATTERN)
    return out


def ingest(gpu, kind, t, bo, bl, A, w, **kw):
    f = gpu.map_orswot_from_bincode if kind == "orswot" else gpu.map_map_from_bincode
    return f(t, bo, bl, A, *w, **kw)


def egest(gpu, kind, S, A, w, **kw):
    f = gpu.map_orswot_to_bincode if kind == "orswot" else gpu.map_map_to_bincode
    return f(S, A, *w, **kw)


def arrays(kind, S):
    """field -> host array with the object as its first axis (the nested map's inner rows folded under it)."""
    h = S.host()
    a = dict(h.a)
    if kind == "nested":
        n = len(a["n_keys"])
        for f, v in h.inner.a.items():
            a["inner." + f] = v.reshape((n, S.kcap) + v.shape[1:])
    return a


def masks(kind, S):
    """field -> the slots the state uses, shaped as arrays()."""
    if kind == "orswot":
        return S.used_masks()
    h = S.host()
    a = h.a
    n = len(a["n_keys"])
    key = np.arange(S.kcap)[None, :] < a["n_keys"][:, None]
    dfr = np.arange(S.dcap)[None, :] < a["n_def"][:, None]
    dset = dfr[..., None] & (np.arange(S.scap)[None, None, :] < a["dset_n"][..., None])
    per = {"clock": np.ones(a["clock"].shape, bool), "n_keys": np.ones(n, bool), "n_def": np.ones(n, bool), "keys": key,
           "eclock": key[..., None], "dclock": dfr[..., None], "dset_n": dfr, "dset": dset}
    out = {f: np.broadcast_to(m, a[f].shape) for f, m in per.items()}
    for f, m in h.inner.used_masks().items():
        m = m.reshape((n, S.kcap) + m.shape[1:])
        out["inner." + f] = m & key.reshape((n, S.kcap) + (1,) * (m.ndim - 2))
    return out


def differing(kind, got, exp, skip=()):
    """Objects whose used slots differ (got: a device slab; exp: a host slab, zero past its counts)."""
    g, e, mk = arrays(kind, got), arrays(kind, exp), masks(kind, got)
    bad = set()
    for f in e:
        d = (np.where(mk[f], g[f], 0) != e[f]).reshape(len(e["n_keys"]), -1).any(axis=1)
        bad |= set(np.nonzero(d)[0].tolist())
    return sorted(bad - set(skip))


def untouched(kind, got, skip=()):
    """Only the used slots are written: every other slot of a patterned output keeps the pattern."""
    g, mk = arrays(kind, got), masks(kind, got)
    keep = np.ones(len(g["n_keys"]), bool)
    keep[list(skip)] = False
    return all((g[f][keep][~mk[f][keep]] == PATTERN).all() for f in g)


def upload(blobs, rng=None):
    """Concatenate with 0-5 junk bytes between blobs (any alignment)."""
    import torch

    buf, off, ln = bytearray(), [], []
    for b in blobs:
        if rng is not None:
            buf += bytes(rng.randrange(256) for _ in range(rng.randrange(6)))
        off.append(len(buf))
        ln.append(len(b))
        buf += b
    t = torch.frombuffer(bytearray(buf) or bytearray(1), dtype=torch.uint8).to("cuda:0")
    return t, torch.tensor(off, dtype=torch.int64, device="cuda:0"), torch.tensor(ln, dtype=torch.int64, device="cuda:0")


def blobs_of(out, off, lens):
    host = out.cpu().numpy()
    return [host[a:a + b].tobytes() for a, b in zip(off.cpu().numpy(), lens.cpu().numpy())]


def ingest_patterned(gpu, kind, blobs, A, w, caps, rng=None, check_status=True):
    t, bo, bl = upload(blobs, rng)
    return ingest(gpu, kind, t, bo, bl, A, w, out=patterned(kind, len(blobs), A, caps), check_status=check_status)


class _Reverse:
    """An `rng` for the encoders: every unordered container in descending order."""

    def shuffle(self, x):
        x.reverse()


# ------------------------------------------------------------------ states from plain lists
def spec_of(kind, m):
    """A state as nested_bincode_cases' plain lists, every container in canonical order."""
    pairs = lambda c: sorted(c.dots.items())  # noqa: E731
    defs = lambda d: [(pairs(c), sorted(d[c])) for c in crdts_ref.clock_order(list(d))]  # noqa: E731

    def value(v):
        if kind == "orswot":
            return (pairs(v.clock), [(x, pairs(v.entries[x])) for x in sorted(v.entries)], defs(v.deferred))
        return (pairs(v.clock), [(k, pairs(v.entries[k][0]), [(pairs(c), x) for c, x in v.entries[k][1].vals])
                                 for k in sorted(v.entries)], defs(v.deferred))

    return (pairs(m.clock), [(k, pairs(m.entries[k][0]), value(m.entries[k][1])) for k in sorted(m.entries)],
            defs(m.deferred))


def state_of(kind, spec, w=None):
    w = w or W8[kind]
    return dec(kind, NC.raw(kind, w, spec)[0], w)


def _spread(values, width):
    """Distinct values -> the same count of values inside `width` bytes, ascending, its largest included."""
    top = (1 << (8 * width)) - 1
    vs = sorted(values)
    return {v: (top if i == len(vs) - 1 and len(vs) > 1 else 3 + 7 * i) for i, v in enumerate(vs)}


def narrowed(kind, states, w):
    """The same states with every key, member / inner key and value inside the widths (order kept)."""
    specs = [spec_of(kind, m) for m in states]
    keys = {k for s in specs for k, _, _ in s[1]} | {k for s in specs for _, ks in s[2] for k in ks}
    inner = {x for s in specs for _, _, v in s[1] for x in [e[0] for e in v[1]] + [y for _, ys in v[2] for y in ys]}
    fk, fx = _spread(keys, w[1]), _spread(inner, w[2])
    mask = (1 << (8 * w[3])) - 1 if kind == "nested" else 0
    dd = lambda d, f: [(c, [f[x] for x in xs]) for c, xs in d]  # noqa: E731

    def value(v):
        if kind == "orswot":
            return (v[0], [(fx[x], c) for x, c in v[1]], dd(v[2], fx))
        return (v[0], [(fx[k], ec, [(c, x & mask) for c, x in vals]) for k, ec, vals in v[1]], dd(v[2], fx))

    return [state_of(kind, (s[0], [(fk[k], ec, value(v)) for k, ec, v in s[1]], dd(s[2], fk)), w) for s in specs]


_BATCH = {}


def batch(kind):
    """The 2 000 generated maps at A = 16 (shared, unchanged): states, blobs with
    every unordered container shuffled, canonical blobs, caps, the expected slab."""
    if kind not in _BATCH:
        states = map_truncgen.states_of(kind, 11 if kind == "orswot" else 12, 2000, A16)
        w = (1,) + W8[kind][1:]
        rng = random.Random(13)
        caps = caps_of(kind, states)
        _BATCH[kind] = dict(states=states, w=w, caps=caps, blobs=[enc(kind, s, w, rng) for s in states],
                            canon=[enc(kind, s, w) for s in states], slab=pack(kind, states, A16, caps))
    return _BATCH[kind]


# ------------------------------------------------------------------ 1. generated batches
@pytest.mark.parametrize("kind", KINDS)
def test_ingest_generated(gpu, kind):
    b = batch(kind)
    # presented out of order (the nested map: about half of its ~180 maps with two outer deferred clocks)
    assert sum(x != y for x, y in zip(b["blobs"], b["canon"])) > (500 if kind == "orswot" else 50)
    got = ingest_patterned(gpu, kind, b["blobs"], A16, b["w"], b["caps"], random.Random(14))
    bad = differing(kind, got, b["slab"])
    assert not bad, f"{len(bad)} maps differ; first {bad[0]}: {b['states'][bad[0]].canonical()}"
    assert untouched(kind, got)


@pytest.mark.parametrize("kind", KINDS)
def test_egest_and_round_trip(gpu, kind):
    b = batch(kind)
    out, off, lens = egest(gpu, kind, b["slab"].to("cuda:0"), A16, b["w"])
    got = blobs_of(out, off, lens)
    bad = [i for i, (g, e) in enumerate(zip(got, b["canon"])) if g != e]
    assert not bad, f"{len(bad)} blobs differ; first {bad[0]}"
    back = ingest(gpu, kind, out, off, lens, A16, b["w"], out=patterned(kind, len(got), A16, b["caps"]))
    assert not differing(kind, back, b["slab"])


# ------------------------------------------------------------------ 2. widths
WIDTHS = {"orswot": [(1, 1, 1), (2, 2, 2), (4, 4, 4), (8, 8, 8), (1, 8, 2)],
          "nested": [(1, 1, 1, 1), (2, 2, 2, 2), (4, 4, 4, 4), (8, 8, 8, 8), (1, 8, 2, 4)]}


@pytest.mark.parametrize("kind,w", [(k, w) for k in KINDS for w in WIDTHS[k]])
def test_widths_both_ways(gpu, kind, w):
    b = batch(kind)
    states = narrowed(kind, b["states"][:600], w)
    exp = pack(kind, states, A16, b["caps"])
    rng = random.Random(sum(w))
    got = ingest_patterned(gpu, kind, [enc(kind, s, w, rng) for s in states], A16, w, b["caps"], rng)
    assert not differing(kind, got, exp)
    assert blobs_of(*egest(gpu, kind, exp.to("cuda:0"), A16, w)) == [enc(kind, s, w) for s in states]


# ------------------------------------------------------------------ 3. edges
def _full(A, c=1):
    return [(a, c + a) for a in range(A)]


def _three(A):
    """Three deferred clocks that differ only in their second pair (one actor: in their counter)."""
    hi = A - 1
    return [[(0, 1), (hi, 3 - j)] if A >= 2 else [(0, 3 - j)] for j in range(3)]


def _desc_clocks(A, n):
    """n clocks, given in descending CLOCK ORDER."""
    return [[(0, n - j)] + ([(A - 1, 1)] if A >= 2 and j % 2 else []) for j in range(n)]


def _long(kind, A, k):
    """k keys with full clocks: the longest blob k keys of three members / inner keys give at this A."""
    if kind == "orswot":
        v = lambda j: (_full(A, 2), [(5 + m, _full(A, 1 + m)) for m in range(3)], [])  # noqa: E731
    else:
        v = lambda j: (_full(A, 2), [(5 + m, _full(A, 1 + m), [(_full(A, 3), 100 * j + m)]) for m in range(3)], [])  # noqa: E731
    return (_full(A, 9), [(10 + 3 * j, _full(A, 2), v(j)) for j in range(k)], [])


def edge_batch(kind, A):
    """-> (states, rngs, caps, names): every edge object between ordinary ones; `full` meets every capacity."""
    w = W8[kind]
    hi = A - 1
    k = 1
    while len(NC.raw(kind, w, _long(kind, A, k))[0]) <= LDS_WINDOW:
        k += 1
    kcap = max(k + 1, 3)
    big = [(hi, U64MAX)]
    e = {"empty": ([], [], [])}
    sh = random.Random(A)
    if kind == "orswot":
        caps = dict(kcap=kcap, mcap=65, vdcap=3, vscap=65, dcap=65, scap=3)
        o = lambda clock=(), members=(), defs=(): (list(clock), list(members), list(defs))  # noqa: E731
        e["empty_nested_set"] = ([(0, 1)], [(7, [(0, 1)], o())], [])
        e["empty_member_clock"] = ([(0, 2)], [(4, [(0, 1)], o([(0, 2)], [(6, []), (8, [(0, 2)])]))], [])
        e["max_counter_last_actor"] = (big, [(U64MAX, big, o(big, [(U64MAX, big)], [(big, [U64MAX])]))], [(big, [U64MAX])])
        e["65_members_descending"] = ([(0, 70)], [(1, [(0, 70)], o([(0, 70)], [(200 - m, [(0, 1 + m)])
                                                                               for m in range(65)]))], [])
        e["65_map_deferred_descending"] = ([(0, 1)], [], [(c, [1 + j % 3]) for j, c in enumerate(_desc_clocks(A, 65))])
        e["three_nested_deferred"] = ([(0, 1)], [(1, [(0, 1)], o([(0, 1)], [], [(c, [j]) for j, c in
                                                                               enumerate(_three(A))]))], [])
        s65 = list(range(100, 165))
        sh.shuffle(s65)
        e["deferred_member_set_of_65"] = ([(0, 1)], [(1, [(0, 1)], o([(0, 1)], [], [([(0, 9)], s65)]))], [])
        full_v = lambda j: o(_full(A, 2), [(300 - m, [(m % A, 1 + m)]) for m in range(65)],  # noqa: E731
                             [(c, [150 - x for x in range(65)]) for c in _desc_clocks(A, 3)])
        e["full"] = (_full(A, 9), [(10 + j, [(hi, 1 + j)], full_v(j)) for j in range(kcap)],
                     [(c, [10, 11, 12]) for c in _desc_clocks(A, 65)])
    else:
        caps = ((kcap, 64, 3), (3, 3, 3, 3))
        i = lambda clock=(), entries=(), defs=(): (list(clock), list(entries), list(defs))  # noqa: E731
        e["empty_inner_map"] = ([(0, 1)], [(7, [(0, 1)], i())], [])
        e["register_without_values"] = ([(0, 2)], [(4, [(0, 2)], i([(0, 2)], [(6, [(0, 2)], [])]))], [])
        e["max_counter_last_actor"] = (big, [(U64MAX, big, i(big, [(U64MAX, big, [(big, U64MAX)])], [(big, [U64MAX])]))],
                                       [(big, [U64MAX])])
        e["64_outer_deferred_descending"] = ([(0, 1)], [], [(c, [1 + j % 3]) for j, c in enumerate(_desc_clocks(A, 64))])
        e["three_inner_deferred"] = ([(0, 1)], [(1, [(0, 1)], i([(0, 1)], [], [(c, [j]) for j, c in
                                                                              enumerate(_three(A))]))], [])
        full_v = lambda j: i(_full(A, 2), [(5 + m, [(hi, 1 + m)], [([(m % A, 1 + v)], 10 * m + v) for v in range(3)])  # noqa: E731
                                          for m in range(3)], [(c, [5, 6, 7]) for c in _desc_clocks(A, 3)])
        e["full"] = (_full(A, 9), [(10 + j, [(hi, 1 + j)], full_v(j)) for j in range(kcap)],
                     [(c, [10, 11, 12]) for c in _desc_clocks(A, 64)])
        # an inner map in the last outer slot, k = kcap - 1, after empty ones
        e["inner_map_in_last_slot"] = ([(0, 3)], [(j, [(0, 1)], i()) for j in range(kcap - 1)] +
                                       [(99, [(0, 3)], full_v(0))], [])
    e["one_key_past_the_window"] = _long(kind, A, k)
    # the same keys and one more set of deferred clocks: a nested value lies across byte 4096 of the blob
    lg = _long(kind, A, k)
    lg = (lg[0], [(lg[1][0][0], [], lg[1][0][2])] + lg[1][1:], [(c, [10]) for c in _desc_clocks(A, 3)])
    e["value_straddles_the_window_end"] = lg
    # the descending / shuffled specs are kept as written by encoding them raw; states come from decoding
    blobs = {name: NC.raw(kind, w, s)[0] for name, s in e.items()}
    states = {name: dec(kind, b, w) for name, b in blobs.items()}
    assert caps_of(kind, [states["full"]]) == caps
    assert len(blobs["one_key_past_the_window"]) > LDS_WINDOW >= len(NC.raw(kind, w, _long(kind, A, k - 1))[0])
    lens = NC.raw(kind, w, lg)[1]
    first = "orswot clock" if kind == "orswot" else "inner map clock"
    starts = [p for p, label in lens if label == first]
    ends = [p - 8 for p, label in lens if label == "entry clock"][1:] + [p for p, label in lens if label == "deferred n"]
    assert any(p < LDS_WINDOW < q for p, q in zip(starts, ends)), list(zip(starts, ends))
    for name in blobs:
        if "descending" in name or "three" in name or "65" in name or name == "full":
            assert blobs[name] != enc(kind, states[name], w), name  # presented out of order
    pool = map_truncgen.states_of(kind, 40 + A, 40, A) if A >= 3 or kind == "orswot" else []
    fits = lambda m: all(x <= y for x, y in zip(_flat(kind, caps_of(kind, [m])), _flat(kind, caps)))  # noqa: E731
    ordinary = [m for m in pool if fits(m)] or [states["empty"]]
    out_b, out_s, names = [], [], []
    for j, name in enumerate(e):
        m = ordinary[j % len(ordinary)]
        out_b += [enc(kind, m, w, random.Random(j)), blobs[name]]
        out_s += [m, states[name]]
        names += ["ordinary", name]
    return out_b, out_s, caps, names


def _flat(kind, caps):
    return list(caps.values()) if kind == "orswot" else list(caps[0]) + list(caps[1])


@pytest.mark.parametrize("kind,A", [(k, A) for k in KINDS for A in (1, 16, 128)])
def test_edges(gpu, kind, A):
    blobs, states, caps, names = edge_batch(kind, A)
    w = W8[kind]
    exp = pack(kind, states, A, caps)
    got = ingest_patterned(gpu, kind, blobs, A, w, caps, random.Random(A))
    bad = differing(kind, got, exp)
    assert not bad, [names[i] for i in bad]
    assert untouched(kind, got)
    assert blobs_of(*egest(gpu, kind, got, A, w)) == [enc(kind, m, w) for m in states]


# ------------------------------------------------------------------ 4. malformed blobs
A_ERR = 128  # the golden u8 states use the reference's test actors (up to 93)
ERR_CAPS = {"orswot": dict(kcap=3, mcap=3, vdcap=3, vscap=3, dcap=3, scap=3), "nested": ((3, 3, 3), (3, 3, 3, 3))}


def neighbours(kind):
    """Well-formed u8 states inside ERR_CAPS: the malformed blobs' base state and the u8 golden ones."""
    from test_nested_bincode_ref import golden_cases, state_of as golden_state

    name = "bincode_map_orswot.json" if kind == "orswot" else "bincode_map_map.json"
    out = [state_of(kind, NC.GOOD[kind], NC.WIDTHS[kind])]
    out += [golden_state(c) for c in golden_cases((name,)) if c["widths"][0] == 1 and c["canonical"]]
    assert len(out) >= 4
    return out


def bad_blobs(kind):
    """name -> (blob, code)"""
    import crdts_hip

    out = {k: (b, crdts_hip.CRDT_ENONCANON) for k, (b, _) in NC.malformed(kind, A_ERR).items()}
    out["empty_blob"] = (b"", crdts_hip.CRDT_ENONCANON)
    for k, b in NC.over_capacity(kind, ERR_CAPS[kind]).items():
        out[k + " + 1"] = (b, crdts_hip.CRDT_ECAPACITY)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_errors_every_fourth(gpu, kind):
    import crdts_hip

    w, caps = NC.WIDTHS[kind], ERR_CAPS[kind]
    bad, good = bad_blobs(kind), neighbours(kind)
    assert {n[12:] for n in bad if n.startswith("length_2_63 ")} == NC.LENGTH_LABELS[kind]
    empty = state_of(kind, ([], [], []), w)
    blobs, states, where = [], [], []
    for j, name in enumerate(sorted(bad)):
        for x in range(3):
            m = good[(3 * j + x) % len(good)]
            blobs.append(enc(kind, m, w, random.Random(j)))
            states.append(m)
        where.append(len(blobs))
        blobs.append(bad[name][0])
        states.append(empty)
    with pytest.raises(crdts_hip.CrdtError) as e:
        ingest_patterned(gpu, kind, blobs, A_ERR, w, caps, random.Random(3))
    assert e.value.code in (crdts_hip.CRDT_ENONCANON, crdts_hip.CRDT_ECAPACITY)
    got = ingest_patterned(gpu, kind, blobs, A_ERR, w, caps, random.Random(3), check_status=False)
    with pytest.raises(crdts_hip.CrdtError):
        gpu.status()
    assert not differing(kind, got, pack(kind, states, A_ERR, caps), skip=where)  # every well-formed neighbour
    assert untouched(kind, got, skip=where)


@pytest.mark.parametrize("kind", KINDS)
def test_each_error_alone_has_its_own_code(gpu, kind):
    import crdts_hip

    w, caps = NC.WIDTHS[kind], ERR_CAPS[kind]
    bad, good = bad_blobs(kind), neighbours(kind)
    empty = state_of(kind, ([], [], []), w)
    exp = pack(kind, [good[0], empty, good[1]], A_ERR, caps)
    for name in sorted(bad):
        three = [enc(kind, good[0], w, random.Random(1)), bad[name][0], enc(kind, good[1], w, random.Random(2))]
        got = ingest_patterned(gpu, kind, three, A_ERR, w, caps, random.Random(4), check_status=False)
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.status()
        assert e.value.code == bad[name][1], name
        assert not differing(kind, got, exp, skip=[1]), name


def _i64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


@pytest.mark.parametrize("kind", KINDS)
def test_blob_extent_outside_the_buffer_is_reported(gpu, kind):
    """A blob_len that overruns blob_bytes, a blob_off past it and a 2^63 length
    are CRDT_ENONCANON; the bytes are not read (the good blob ends the buffer)."""
    import crdts_hip

    w, caps = NC.WIDTHS[kind], ERR_CAPS[kind]
    m = neighbours(kind)[0]
    good = enc(kind, m, w)
    exp = pack(kind, [m, m, m], A_ERR, caps)
    for off, ln in ((0, len(good) + 1), (2 * len(good) + 5, 8), (0, 1 << 63), (1 << 63, len(good)), (1, U64MAX)):
        t, bo, bl = upload([good, good, good])
        bo[1], bl[1] = _i64(off), _i64(ln)
        assert int(bo[2]) + int(bl[2]) == t.numel()
        out = patterned(kind, 3, A_ERR, caps)
        with pytest.raises(crdts_hip.CrdtError) as e:
            ingest(gpu, kind, t, bo, bl, A_ERR, w, out=out)
        assert e.value.code == crdts_hip.CRDT_ENONCANON, (off, ln)
        assert not differing(kind, out, exp, skip=[1])


# ------------------------------------------------------------------ 5. egest errors, host-side refusals
def _fn(kind, what):
    from crdts_hip._lib import lib

    return getattr(lib, f"crdt_map_{'orswot' if kind == 'orswot' else 'map'}_{what}")


@pytest.mark.parametrize("kind", KINDS)
def test_egest_errors(gpu, kind):
    """A member / value that does not fit one byte, a count above its capacity
    (outer and nested): size 0, nothing written inside the object's span,
    CRDT_ENONCANON; a blob placed past out_bytes: CRDT_ECAPACITY, not written."""
    import torch

    import crdts_hip

    w, caps = NC.WIDTHS[kind], ERR_CAPS[kind]
    good = neighbours(kind)
    states = [good[i % len(good)] for i in range(8)]
    base = state_of(kind, NC.GOOD[kind], w)
    states[1] = states[3] = states[5] = base
    S = pack(kind, states, A_ERR, caps)
    if kind == "orswot":
        S.a["vmem"][1, 0, 0] = 300      # a member past u8
        S.a["n_keys"][3] = caps["kcap"] + 1
        S.a["vn_mem"][5, 1] = caps["mcap"] + 1
    else:
        S.inner.a["mv_val"][1 * 3 + 0, 1, 0] = 300  # a value past u8
        S.a["n_def"][3] = caps[0][1] + 1
        S.inner.a["n_keys"][5 * 3 + 1] = caps[1][0] + 1
    wrong = (1, 3, 5)
    dev = S.to("cuda:0")
    s = dev.cstruct()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sizes = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
    assert _fn(kind, "bincode_sizes")(gpu.ctx, C.byref(s), 8, A_ERR, *w, p(sizes), None) == 0
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    exp = [b"" if i in wrong else enc(kind, m, w) for i, m in enumerate(states)]
    assert sizes.cpu().tolist() == [len(b) for b in exp]
    # every object gets a 7-byte-misaligned span of its size + 64 bytes of 0xEE; the last is placed past the end
    off, pos = [], 7
    for b in exp:
        off.append(pos)
        pos += len(b) + 64
    pos -= 64 + 1  # the last blob's last byte lies outside
    out = torch.full((pos + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    doff = torch.tensor(off, dtype=torch.int64, device="cuda:0")
    assert _fn(kind, "to_bincode")(gpu.ctx, C.byref(s), 8, A_ERR, *w, p(out), p(doff), pos, None) == 0
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code in (crdts_hip.CRDT_ENONCANON, crdts_hip.CRDT_ECAPACITY)
    want = bytearray(b"\xEE" * (pos + 64))
    for o, b in list(zip(off, exp))[:-1]:
        want[o:o + len(b)] = b
    assert out.cpu().numpy().tobytes() == bytes(want)  # the blobs, and not a byte outside them
    # the placement alone: its own code
    ok = pack(kind, states[:1], A_ERR, caps).to("cuda:0")
    s1 = ok.cstruct()
    n1 = len(enc(kind, states[0], w))
    buf = torch.zeros(n1 + 40, dtype=torch.uint8, device="cuda:0")
    doff = torch.tensor([41], dtype=torch.int64, device="cuda:0")
    assert _fn(kind, "to_bincode")(gpu.ctx, C.byref(s1), 1, A_ERR, *w, p(buf), p(doff), n1 + 40, None) == 0
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ECAPACITY and not buf.any()


@pytest.mark.parametrize("kind", KINDS)
def test_argument_validation(gpu, kind):
    import torch

    import crdts_hip

    EINVAL = crdts_hip.CRDT_EINVAL
    w, caps = NC.WIDTHS[kind], ERR_CAPS[kind]
    m = neighbours(kind)[0]
    t, bo, bl = upload([enc(kind, m, w)])
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    out = alloc(kind, 1, A_ERR, caps, device="cuda:0")
    r = out.cstruct()
    sizes = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    buf = torch.zeros(512, dtype=torch.uint8, device="cuda:0")
    at0 = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def ing(ctx=gpu.ctx, blobs=p(t), n=1, w=w, A=A_ERR, slab=r):
        return _fn(kind, "from_bincode")(ctx, blobs, int(t.numel()), p(bo), p(bl), n, *w, A, C.byref(slab), None)

    def siz(w=w, A=A_ERR, slab=r, dst=p(sizes)):
        return _fn(kind, "bincode_sizes")(gpu.ctx, C.byref(slab), 1, A, *w, dst, None)

    def wri(w=w, slab=r, dst=p(buf), nbytes=512, n=1):
        return _fn(kind, "to_bincode")(gpu.ctx, C.byref(slab), n, A_ERR, *w, dst, p(at0), nbytes, None)

    assert ing() == 0 and siz() == 0 and wri() == 0
    gpu.status()
    assert ing(ctx=None) == EINVAL and ing(blobs=None) == EINVAL
    assert ing(blobs=None, n=0) == 0 and wri(dst=None, n=0, nbytes=0) == 0  # n_obj == 0: nothing is launched
    for j in range(len(w)):
        for v in (0, 3, 16):
            bw = w[:j] + (v,) + w[j + 1:]
            assert ing(w=bw) == EINVAL and siz(w=bw) == EINVAL and wri(w=bw) == EINVAL, bw
    assert ing(A=0) == EINVAL and ing(A=129) == EINVAL and siz(A=0) == EINVAL and siz(A=129) == EINVAL
    assert siz(dst=None) == EINVAL and wri(dst=None) == EINVAL and wri(nbytes=23) == EINVAL

    def with_caps(**kw):
        import crdts_hip as ch

        if kind == "orswot":
            return ch.MapOrswotSlab(out.a, {**caps, **kw}).cstruct()
        o = dict(zip(("kcap", "dcap", "scap"), caps[0]))
        i = dict(zip(("ikcap", "imcap", "idcap", "iscap"), caps[1]))
        o.update({k: v for k, v in kw.items() if k in o})
        i.update({k: v for k, v in kw.items() if k in i})
        return ch.MapMapSlab(out.a, o["kcap"], o["dcap"], o["scap"], ch.MapSlab(out.inner.a, *i.values())).cstruct()

    # ingest: the merges' per-side limits; egest: twice them
    limits = (dict(kcap=4096, mcap=256, vdcap=256, vscap=256, dcap=256, scap=4096) if kind == "orswot" else
              dict(kcap=4096, dcap=64, scap=4096, ikcap=4096, imcap=128, idcap=64, iscap=4096))
    for name, lim in limits.items():
        assert ing(slab=with_caps(**{name: 0})) == EINVAL and siz(slab=with_caps(**{name: 0})) == EINVAL, name
        assert ing(slab=with_caps(**{name: lim + 1})) == EINVAL, name
        assert siz(slab=with_caps(**{name: 2 * lim + 1})) == EINVAL and wri(slab=with_caps(**{name: 2 * lim + 1})) == EINVAL
    gpu.status()


@pytest.mark.parametrize("kind", KINDS)
def test_side_stream(gpu, kind):
    import torch

    b = batch(kind)
    n = 300
    st = torch.cuda.Stream()
    t, bo, bl = upload(b["blobs"][:n], random.Random(5))
    out = patterned(kind, n, A16, b["caps"])
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got = ingest(gpu, kind, t, bo, bl, A16, b["w"], out=out, stream=st)
        blobs = egest(gpu, kind, got, A16, b["w"], stream=st)
    st.synchronize()
    assert not differing(kind, got, pack(kind, b["states"][:n], A16, b["caps"]))
    assert blobs_of(*blobs) == b["canon"][:n]


# ------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("kind", KINDS)
def test_blobs_merge_blobs_on_the_device(gpu, kind):
    """1 000 pairs: ingest both sides, the merge kernel, egest; the bytes are the
    restatement's encoding of crdts_ref's merge of the decoded inputs."""
    n = 1000
    b = batch(kind)
    w = b["w"]
    L, R = b["states"][:n], map_truncgen.states_of(kind, 21, n, A16)
    rng = random.Random(22)
    lb, rb = [enc(kind, m, w, rng) for m in L], [enc(kind, m, w, rng) for m in R]
    capsR = caps_of(kind, R)
    if kind == "orswot":
        S = gpu.map_orswot_from_bincode(*upload(lb, rng), A16, *w, out_caps=b["caps"])
        O = gpu.map_orswot_from_bincode(*upload(rb, rng), A16, *w, out_caps=capsR)
        M = gpu.map_orswot_merge(S, O, A16)
    else:
        S = gpu.map_map_from_bincode(*upload(lb, rng), A16, *w, out_caps=(*b["caps"][0], b["caps"][1]))
        O = gpu.map_map_from_bincode(*upload(rb, rng), A16, *w, out_caps=(*capsR[0], capsR[1]))
        M = gpu.map_map_merge(S, O, A16)
    got = blobs_of(*egest(gpu, kind, M, A16, w))
    bad = []
    for i, (x, y, g) in enumerate(zip(lb, rb, got)):
        e = dec(kind, x, w)  # Map<Orswot>: built with order=crdts_ref.clock_order, as map_orswot_opgen.new_map does
        e.merge(dec(kind, y, w))
        if g != enc(kind, e, w):
            bad.append(i)
    assert not bad, f"{len(bad)} merges differ; first {bad[0]}"
    assert sum(bool(m.deferred) for m in R) > 50
