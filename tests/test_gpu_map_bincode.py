"""GPU parity of the bincode codec of MVReg<V, A> and Map<K, MVReg<V, A>, A>
(crdt_mvreg_{from,to}_bincode, crdt_map_mvreg_{from,to}_bincode; SURVEY.md
§8(f) rank 1) against the format restatement (tests/map_bincode_ref.py) and
the slab renderings of tests/map_slab.py / tests/mvreg_opgen.py: byte-exact
slabs from blobs whose deferred HashMap is in any order and which lie at any
byte alignment, byte-exact blobs from slabs, every integer width, the edges of
the slab capacities and of the LDS stage window, malformed input, and blobs ->
merge -> blobs on the device against the restatement's merge."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import map_bincode_ref as MB
import map_slab
import mvreg_opgen
from map_slab import crdts_ref
from test_map_bincode_ref import gen_map_states

pytestmark = pytest.mark.gpu

A16 = 16
CAPS = (5, 4, 5, 5)      # kcap, mcap, dcap, scap of the generated batches (their maxima: 4, 3, 4, 4)
PATTERN = 0x5A5A5A5A
LDS_WINDOW = 4096        # the ingest kernel's per-wave stage window (csrc/map_bincode.hip, kStage)
U64MAX = (1 << 64) - 1


# ------------------------------------------------------------------ helpers
def _upload(blobs, rng=None):
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
    o = torch.tensor(off, dtype=torch.int64, device="cuda:0")
    n = torch.tensor(ln, dtype=torch.int64, device="cuda:0")
    return t, o, n


def _blobs_of(out, off, lens):
    host = out.cpu().numpy()
    o, n = off.cpu().numpy(), lens.cpu().numpy()
    return [host[a:a + b].tobytes() for a, b in zip(o, n)]


def _slab_of(maps, A, caps):
    import crdts_hip

    S = crdts_hip.MapSlab.alloc(len(maps), A, *caps)
    for i, m in enumerate(maps):
        map_slab.mvreg_map_to_row(m, S, i, A, zero=False)
    return S


def _patterned(n, A, caps):
    import crdts_hip

    out = crdts_hip.MapSlab.alloc(n, A, *caps, device="cuda:0")
    for v in out.a.values():
        v.fill_(PATTERN)
    return out


def _differing(got, exp, skip=()):
    """Objects whose used slots differ (got: a device slab; exp: a host slab, zero past its counts)."""
    g = got.canonical()
    bad = set()
    for f in exp.a:
        d = (g.a[f] != exp.a[f]).reshape(len(exp.a["n_keys"]), -1).any(axis=1)
        bad |= set(np.nonzero(d)[0].tolist())
    return sorted(bad - set(skip))


def _untouched(got, skip=()):
    """Only the used slots are written: every other slot of a patterned output keeps the pattern."""
    h = got.host()
    keep = np.ones(len(h.a["n_keys"]), bool)
    keep[list(skip)] = False
    for f, m in got.used_masks().items():
        v = h.a[f][keep]
        if not (v[~m[keep]] == PATTERN).all():
            return False
    return True


def _ingest_maps(gpu, blobs, A, widths, caps, rng=None, check_status=True):
    t, bo, bl = _upload(blobs, rng)
    out = _patterned(len(blobs), A, caps)
    return gpu.map_mvreg_from_bincode(t, bo, bl, A, *widths, out=out, check_status=check_status)


def _i64(x):
    """A u64 as the int64 a torch tensor holds."""
    return x - (1 << 64) if x >= 1 << 63 else x


class _Reverse:
    """An `rng` for encode_map_mvreg: the deferred clocks in descending CLOCK ORDER."""

    def shuffle(self, x):
        x.reverse()


def _vc(pairs):
    return crdts_ref.VClock(list(pairs))


def _reg(vals):
    r = crdts_ref.MVReg()
    r.vals = [(_vc(c), v) for c, v in vals]
    return r


def _map(clock, entries, deferred=()):
    m = crdts_ref.Map(crdts_ref.MVReg)
    m.clock = _vc(clock)
    for key, ec, vals in entries:
        m.entries[key] = [_vc(ec), _reg(vals)]
    for c, ks in deferred:
        m.deferred[_vc(c)] = set(ks)
    return m


_BATCH = {}


def _batch():
    """The 5 000 generated maps (shared, unchanged): states, blobs in shuffled deferred order, the expected slab."""
    if not _BATCH:
        states = gen_map_states(11, 5000, A16)
        rng = random.Random(12)
        _BATCH.update(states=states, blobs=[MB.encode_map_mvreg(s, 1, 8, 8, rng=rng) for s in states],
                      slab=_slab_of(states, A16, CAPS))
    return _BATCH


# ------------------------------------------------------------------ Map: ingest, egest, round trip
def test_map_ingest_generated(gpu):
    b = _batch()
    assert sum(len(s.deferred) >= 2 for s in b["states"]) >= 100  # the deferred sort is exercised
    assert any(not s.entries and not s.deferred for s in b["states"])
    got = _ingest_maps(gpu, b["blobs"], A16, (1, 8, 8), CAPS, random.Random(13))
    bad = _differing(got, b["slab"])
    assert not bad, f"{len(bad)} maps differ; first {bad[0]}: {b['states'][bad[0]].canonical()}"
    assert _untouched(got)


def test_map_egest_and_round_trip(gpu):
    b = _batch()
    S = b["slab"].to("cuda:0")
    out, off, lens = gpu.map_mvreg_to_bincode(S, A16, 1, 8, 8)
    got = _blobs_of(out, off, lens)
    exp = [MB.encode_map_mvreg(s, 1, 8, 8) for s in b["states"]]  # CLOCK ORDER
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, f"{len(bad)} blobs differ; first {bad[0]}"
    back = gpu.map_mvreg_from_bincode(out, off, lens, A16, 1, 8, 8, out=_patterned(len(exp), A16, CAPS))
    assert not _differing(back, b["slab"])


def _narrow(states, wv):
    """The same maps with every value inside val_bytes."""
    mask = (1 << (8 * wv)) - 1
    for s in states:
        for e in s.entries.values():
            e[1].vals = [(c, v & mask) for c, v in e[1].vals]
    return states


@pytest.mark.parametrize("wa,wk,wv", [(1, 1, 1), (2, 2, 2), (4, 4, 4), (8, 8, 8), (1, 8, 2)])
def test_map_widths_both_ways(gpu, wa, wk, wv):
    top = (1 << (8 * wk)) - 1
    keys = (3, 17, top - 55, top)  # inside the key width, its largest value included
    states = _narrow(gen_map_states(100 + wa + wk + wv, 1500, A16, keys=keys), wv)
    caps = (4, 4, 5, 4)
    exp = _slab_of(states, A16, caps)
    rng = random.Random(wa * 64 + wk * 8 + wv)
    got = _ingest_maps(gpu, [MB.encode_map_mvreg(s, wa, wk, wv, rng=rng) for s in states], A16, (wa, wk, wv), caps, rng)
    assert not _differing(got, exp)
    blobs = _blobs_of(*gpu.map_mvreg_to_bincode(exp.to("cuda:0"), A16, wa, wk, wv))
    assert blobs == [MB.encode_map_mvreg(s, wa, wk, wv) for s in states]


# ------------------------------------------------------------------ Map: edges
def _full_clock(A, c=1):
    return [(a, c + a) for a in range(A)]


def _long_map(A, k, mcap):
    """k keys with full clocks: the longest blob k keys give at this A."""
    return _map(_full_clock(A, 9), [(10 + 3 * j, _full_clock(A, 2), [(_full_clock(A, 1 + v), 100 * j + v)
                                                                     for v in range(mcap)]) for j in range(k)])


def edge_batch(A):
    """-> (maps, rngs, caps, names): every edge object between ordinary ones; caps are met exactly by `full`."""
    mcap, dcap, scap = 3, 3, 3
    k = 1
    while len(MB.encode_map_mvreg(_long_map(A, k, mcap), 8, 8, 8)) <= LDS_WINDOW:
        k += 1
    kcap = max(k + 1, 4)  # the keys the window needs, plus one
    hi = A - 1
    if A >= 2:
        three = [([(0, 1), (hi, 3)], [1]), ([(0, 1), (hi, 2)], [2]), ([(0, 1), (hi, 1)], [3])]
    else:
        three = [([(0, 3)], [1]), ([(0, 2)], [2]), ([(0, 1)], [3])]
    full_def = [([(0, 5 + d)] + ([(hi, 1)] if A >= 2 else []), [7 + d + 11 * j for j in range(scap)])
                for d in range(dcap)]
    edges = {
        "empty": _map([], []),
        "zero_values": _map([(0, 1)], [(7, [(0, 1)], [])]),
        "max_counter_last_actor": _map([(hi, U64MAX)], [(U64MAX, [(hi, U64MAX)], [([(hi, U64MAX)], U64MAX)])],
                                       [([(hi, U64MAX)], [U64MAX])]),
        "empty_clocks": _map([(0, 2)], [(4, [], [([], 6)])]),
        "full": None,  # below: `long` with dcap deferred clocks of scap keys
        "long": _long_map(A, kcap, mcap),
        "three_deferred_descending": _map([(0, 1)], [(1, [(0, 1)], [([(0, 1)], 5)])], three),
    }
    full = _long_map(A, kcap, mcap)
    for c, ks in full_def:
        full.deferred[_vc(c)] = set(ks)
    edges["full"] = full
    assert len(full.entries) == kcap and all(len(e[1].vals) == mcap for e in full.entries.values())
    assert len(full.deferred) == dcap and all(len(s) == scap for s in full.deferred.values())
    assert len(MB.encode_map_mvreg(edges["long"], 8, 8, 8)) > LDS_WINDOW
    caps = (kcap, mcap, dcap, scap)
    ordinary = [m for m in gen_map_states(40 + A, 60, A, n_ops=8)
                if len(m.entries) <= kcap and len(m.deferred) <= dcap and
                all(len(e[1].vals) <= mcap for e in m.entries.values()) and
                all(len(s) <= scap for s in m.deferred.values())]
    assert len(ordinary) > len(edges) + 1
    maps, rngs, names = [ordinary[0]], [None], ["ordinary"]
    for j, (name, m) in enumerate(edges.items()):
        maps += [m, ordinary[j + 1]]
        rngs += [_Reverse(), random.Random(j)]
        names += [name, "ordinary"]
    return maps, rngs, caps, names


@pytest.mark.parametrize("A", [1, 16, 128])
def test_map_edges(gpu, A):
    maps, rngs, caps, names = edge_batch(A)
    blobs = [MB.encode_map_mvreg(m, 8, 8, 8, rng=r) for m, r in zip(maps, rngs)]
    i3 = names.index("three_deferred_descending")
    assert blobs[i3] != MB.encode_map_mvreg(maps[i3], 8, 8, 8)  # presented in descending order
    exp = _slab_of(maps, A, caps)
    got = _ingest_maps(gpu, blobs, A, (8, 8, 8), caps, random.Random(A))
    bad = _differing(got, exp)
    assert not bad, [names[i] for i in bad]
    assert _untouched(got)
    out = _blobs_of(*gpu.map_mvreg_to_bincode(got, A, 8, 8, 8))
    assert out == [MB.encode_map_mvreg(m, 8, 8, 8) for m in maps]


# ------------------------------------------------------------------ Map: errors
def _raw_clock(pairs, wa):
    out = struct.pack("<Q", len(pairs))
    for a, c in pairs:
        out += a.to_bytes(wa, "little") + struct.pack("<Q", c)
    return out


def _raw_map(clock, entries, deferred, w=(1, 1, 1)):
    """The format with nothing sorted or checked: entries [(key, clock, [(clock, val)])], deferred [(clock, [keys])]."""
    wa, wk, wv = w
    out = _raw_clock(clock, wa) + struct.pack("<Q", len(entries))
    for key, ec, vals in entries:
        out += key.to_bytes(wk, "little") + _raw_clock(ec, wa) + struct.pack("<Q", len(vals))
        for c, v in vals:
            out += _raw_clock(c, wa) + v.to_bytes(wv, "little")
    out += struct.pack("<Q", len(deferred))
    for c, ks in deferred:
        out += _raw_clock(c, wa) + struct.pack("<Q", len(ks)) + b"".join(k.to_bytes(wk, "little") for k in ks)
    return out


ERR_CAPS = (3, 2, 3, 3)
E5 = (5, [(0, 1)], [([(0, 1)], 42)])
E9 = (9, [(3, 1)], [])
GOOD = ([(0, 2), (3, 1)], [E5, E9], [([(0, 4), (1, 1)], [5, 9]), ([(1, 3)], [5])])


def malformed():
    """name -> (blob, code): every CRDT_ENONCANON kind, one object per capacity at cap + 1."""
    NC, CAP = -2, -4
    good = _raw_map(*GOOD)
    assert MB.map_equal(MB.decode_map_mvreg(good, 1, 1, 1), _map(*GOOD))
    clock, ents, defs = GOOD
    kcap, mcap, dcap, scap = ERR_CAPS
    out = {
        "zero_counter": (_raw_map([(0, 0), (3, 1)], ents, defs), NC),
        "zero_counter_in_value_clock": (_raw_map(clock, [(5, [(0, 1)], [([(0, 0)], 42)]), E9], defs), NC),
        "actor_out_of_range": (_raw_map([(0, 2), (16, 1)], ents, defs), NC),
        "actors_descending": (_raw_map([(3, 1), (0, 2)], ents, defs), NC),
        "actors_duplicate": (_raw_map([(3, 1), (3, 2)], ents, defs), NC),
        "keys_swapped": (_raw_map(clock, [E9, E5], defs), NC),
        "keys_duplicate": (_raw_map(clock, [E5, E5], defs), NC),
        "deferred_set_descending": (_raw_map(clock, ents, [([(0, 4), (1, 1)], [9, 5])]), NC),
        "deferred_set_duplicate": (_raw_map(clock, ents, [([(0, 4), (1, 1)], [5, 5])]), NC),
        "deferred_clock_duplicate": (_raw_map(clock, ents, [defs[0], defs[1], defs[0]]), NC),
        "one_byte_short": (good[:-1], NC),
        "one_byte_extra": (good + b"\0", NC),
        "first_length_word_2_63": (struct.pack("<Q", 1 << 63) + good[8:], NC),
        "entries_length_word_2_63": (good[:26] + struct.pack("<Q", 1 << 63) + good[34:], NC),
        "deferred_length_word_too_large": (_raw_map(clock, ents, [])[:-8] + struct.pack("<Q", 3), NC),
        "empty_blob": (b"", NC),
        "keys_cap_plus_1": (_raw_map(clock, [(k, [(0, 1)], []) for k in range(kcap + 1)], defs), CAP),
        "vals_cap_plus_1": (_raw_map(clock, [(5, [(0, 1)], [([(0, 1 + v)], v) for v in range(mcap + 1)])], defs), CAP),
        "deferred_cap_plus_1": (_raw_map(clock, ents, [([(1, 3 + d)], [5]) for d in range(dcap + 1)]), CAP),
        "set_cap_plus_1": (_raw_map(clock, ents, [([(1, 3)], list(range(scap + 1)))]), CAP),
    }
    for name, (blob, code) in out.items():  # the restatement rejects what the format forbids
        if code == NC and name != "actor_out_of_range":
            with pytest.raises(MB.FormatError):
                MB.decode_map_mvreg(blob, 1, 1, 1)
        else:
            MB.decode_map_mvreg(blob, 1, 1, 1)  # well-formed: past the slab, not the format
    return out


def _ordinary_small(n):
    st = [m for m in _narrow(gen_map_states(77, 4 * n, A16, keys=(3, 17, 200, 255), n_ops=6), 1)
          if len(m.entries) <= ERR_CAPS[0] and len(m.deferred) <= ERR_CAPS[2] and
          all(len(e[1].vals) <= ERR_CAPS[1] for e in m.entries.values()) and
          all(len(s) <= ERR_CAPS[3] for s in m.deferred.values())]
    assert len(st) >= n
    return st[:n]


def test_map_errors_every_fourth(gpu):
    import crdts_hip

    bad = malformed()
    names = sorted(bad)
    good = _ordinary_small(3 * len(names))
    blobs, maps, where = [], [], {}
    for j, name in enumerate(names):
        for m in good[3 * j:3 * j + 3]:
            blobs.append(MB.encode_map_mvreg(m, 1, 1, 1, rng=random.Random(j)))
            maps.append(m)
        where[len(blobs)] = name
        blobs.append(bad[name][0])
        maps.append(_map([], []))
    with pytest.raises(crdts_hip.CrdtError) as e:
        _ingest_maps(gpu, blobs, A16, (1, 1, 1), ERR_CAPS, random.Random(3))
    assert e.value.code in (crdts_hip.CRDT_ENONCANON, crdts_hip.CRDT_ECAPACITY)
    got = _ingest_maps(gpu, blobs, A16, (1, 1, 1), ERR_CAPS, random.Random(3), check_status=False)
    with pytest.raises(crdts_hip.CrdtError):
        gpu.status()
    assert not _differing(got, _slab_of(maps, A16, ERR_CAPS), skip=where)  # every well-formed neighbour
    assert _untouched(got, skip=where)
    # each malformed blob between two neighbours: the status is its own code
    for name in names:
        three = [blobs[0], bad[name][0], blobs[1]]
        with pytest.raises(crdts_hip.CrdtError) as e:
            _ingest_maps(gpu, three, A16, (1, 1, 1), ERR_CAPS, random.Random(4))
        assert e.value.code == bad[name][1], name
        got = _ingest_maps(gpu, three, A16, (1, 1, 1), ERR_CAPS, random.Random(4), check_status=False)
        with pytest.raises(crdts_hip.CrdtError):
            gpu.status()
        assert not _differing(got, _slab_of([maps[0], _map([], []), maps[1]], A16, ERR_CAPS), skip=[1]), name


def test_map_blob_extent_outside_the_buffer_is_reported(gpu):
    """A blob_len that overruns blob_bytes, a blob_off past it and a 2^63 length
    are CRDT_ENONCANON; the bytes are not read (the good blob ends the buffer)."""
    import torch

    import crdts_hip

    m = _map(*GOOD)
    good = MB.encode_map_mvreg(m, 1, 1, 1)
    for off, ln in ((0, len(good) + 1), (2 * len(good) + 5, 8), (0, 1 << 63), (1 << 63, len(good)), (1, U64MAX)):
        t, bo, bl = _upload([good, good, good])
        bo[1], bl[1] = _i64(off), _i64(ln)
        assert int(bo[2]) + int(bl[2]) == t.numel()
        out = _patterned(3, A16, ERR_CAPS)
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.map_mvreg_from_bincode(t, bo, bl, A16, 1, 1, 1, out=out)
        assert e.value.code == crdts_hip.CRDT_ENONCANON, (off, ln)
        assert not _differing(out, _slab_of([m, m, m], A16, ERR_CAPS), skip=[1])
        torch.cuda.synchronize()


def test_map_egest_errors(gpu):
    """A value that does not fit val_bytes = 1, and a count above its capacity:
    size 0, nothing written inside the object's span, CRDT_ENONCANON."""
    import torch

    import crdts_hip
    from crdts_hip._lib import lib

    maps = _ordinary_small(8)
    S = _slab_of(maps, A16, ERR_CAPS)
    wide = next(i for i, m in enumerate(maps) if any(e[1].vals for e in m.entries.values()))
    k = next(k for k in range(ERR_CAPS[0]) if S.a["mv_n"][wide, k])
    S.a["mv_val"][wide, k, 0] = 300
    over = (wide + 3) % 8
    S.a["n_keys"][over] = ERR_CAPS[0] + 1
    D = S.to("cuda:0")
    s = D.cstruct()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sizes = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
    assert lib.crdt_map_mvreg_bincode_sizes(gpu.ctx, C.byref(s), 8, A16, 1, 1, 1, p(sizes), None) == 0
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    exp = [b"" if i in (wide, over) else MB.encode_map_mvreg(m, 1, 1, 1) for i, m in enumerate(maps)]
    assert sizes.cpu().tolist() == [len(b) for b in exp]
    # every object gets a 7-byte-misaligned span of its size + 64 bytes of 0xEE
    off, pos = [], 7
    for b in exp:
        off.append(pos)
        pos += len(b) + 64
    out = torch.full((pos,), 0xEE, dtype=torch.uint8, device="cuda:0")
    doff = torch.tensor(off, dtype=torch.int64, device="cuda:0")
    assert lib.crdt_map_mvreg_to_bincode(gpu.ctx, C.byref(s), 8, A16, 1, 1, 1, p(out), p(doff), pos, None) == 0
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    host = out.cpu().numpy().tobytes()
    want = bytearray(b"\xEE" * pos)
    for o, b in zip(off, exp):
        want[o:o + len(b)] = b
    assert host == bytes(want)  # the blobs, and not a byte outside them


def test_map_argument_validation(gpu):
    import torch

    import crdts_hip
    from crdts_hip._lib import lib

    EINVAL = crdts_hip.CRDT_EINVAL
    m = _map(*GOOD)
    t, bo, bl = _upload([MB.encode_map_mvreg(m, 1, 1, 1)])
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    out = crdts_hip.MapSlab.alloc(1, A16, *ERR_CAPS, device="cuda:0")
    r = out.cstruct()
    sizes = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def ingest(ctx=gpu.ctx, blobs=p(t), n=1, w=(1, 1, 1), A=A16, slab=r):
        return lib.crdt_map_mvreg_from_bincode(ctx, blobs, int(t.numel()), p(bo), p(bl), n, *w, A, C.byref(slab), None)

    assert ingest() == 0
    gpu.status()
    assert ingest(ctx=None) == EINVAL and ingest(blobs=None) == EINVAL
    assert ingest(blobs=None, n=0) == 0  # n_obj == 0: nothing is launched, null arrays included
    for w in ((3, 1, 1), (1, 0, 1), (1, 1, 16)):
        assert ingest(w=w) == EINVAL
    assert ingest(A=0) == EINVAL and ingest(A=129) == EINVAL
    for caps in ((0, 2, 3, 3), (4097, 2, 3, 3), (3, 129, 3, 3), (3, 2, 65, 3), (3, 2, 3, 4097)):
        bad = crdts_hip.MapSlab(out.a, *caps).cstruct()
        assert ingest(slab=bad) == EINVAL, caps
    assert lib.crdt_map_mvreg_bincode_sizes(gpu.ctx, C.byref(r), 1, A16, 1, 5, 1, p(sizes), None) == EINVAL
    assert lib.crdt_map_mvreg_bincode_sizes(gpu.ctx, C.byref(r), 1, A16, 1, 1, 1, None, None) == EINVAL
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    assert lib.crdt_map_mvreg_to_bincode(gpu.ctx, C.byref(r), 1, A16, 1, 1, 1, p(buf), p(sizes), 23, None) == EINVAL
    assert lib.crdt_map_mvreg_to_bincode(gpu.ctx, C.byref(r), 1, A16, 1, 1, 1, None, p(sizes), 256, None) == EINVAL
    # a blob placed past out_bytes is latched for that object, not written
    sizes[0] = 250
    assert lib.crdt_map_mvreg_to_bincode(gpu.ctx, C.byref(r), 1, A16, 1, 1, 1, p(buf), p(sizes), 256, None) == 0
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.status()
    assert e.value.code == crdts_hip.CRDT_ECAPACITY and not buf.any()
    # the stand-alone register's entry points
    n1 = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    c1 = torch.zeros((1, 4, A16), dtype=torch.int64, device="cuda:0")
    v1 = torch.zeros((1, 4), dtype=torch.int64, device="cuda:0")
    f = lib.crdt_mvreg_from_bincode
    assert f(gpu.ctx, p(t), 8, p(bo), p(bl), 1, 1, 1, A16, p(n1), p(c1), p(v1), 0, None) == EINVAL
    assert f(gpu.ctx, p(t), 8, p(bo), p(bl), 1, 1, 1, A16, p(n1), p(c1), p(v1), 1025, None) == EINVAL
    assert f(gpu.ctx, p(t), 8, p(bo), p(bl), 1, 1, 3, A16, p(n1), p(c1), p(v1), 4, None) == EINVAL
    assert f(gpu.ctx, p(t), 8, p(bo), p(bl), 1, 1, 1, 0, p(n1), p(c1), p(v1), 4, None) == EINVAL
    assert f(gpu.ctx, p(t), 8, p(bo), p(bl), 1, 1, 1, A16, None, p(c1), p(v1), 4, None) == EINVAL
    assert f(None, p(t), 8, p(bo), p(bl), 1, 1, 1, A16, p(n1), p(c1), p(v1), 4, None) == EINVAL
    assert f(gpu.ctx, None, 0, None, None, 0, 1, 1, A16, None, None, None, 4, None) == 0
    assert lib.crdt_mvreg_bincode_sizes(gpu.ctx, p(n1), p(c1), p(v1), 2049, 1, A16, 1, 1, p(sizes), None) == EINVAL
    assert lib.crdt_mvreg_to_bincode(gpu.ctx, p(n1), p(c1), p(v1), 4, 1, A16, 1, 1, p(buf), p(sizes), 7, None) == EINVAL
    gpu.status()


# ------------------------------------------------------------------ the stand-alone MVReg
def _dev(slab):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.int64))
                 .to("cuda:0") for x in slab)


def _host(slab):
    return tuple(x.cpu().numpy().view(np.uint32 if x.dtype.itemsize == 4 else np.uint64) for x in slab)


def _patterned_regs(n, cap, A):
    import torch

    return (torch.full((n,), PATTERN, dtype=torch.int32, device="cuda:0"),
            torch.full((n, cap, A), PATTERN, dtype=torch.int64, device="cuda:0"),
            torch.full((n, cap), PATTERN, dtype=torch.int64, device="cuda:0"))


def _same(got, exp):
    return all(np.array_equal(g, e) for g, e in zip(_host(got), exp))


@pytest.mark.parametrize("cap,n", [(4, 4000), (64, 600)])
def test_mvreg_both_ways(gpu, cap, n):
    rng = random.Random(cap)
    regs = [mvreg_opgen.random_reg(rng, A16, cap, 1 << 40, val0=1000 * i) for i in range(n)]
    regs[0].vals = [(_vc([(A16 - 1, U64MAX)]), U64MAX)] * cap  # full, the largest counter, the last actor
    regs[1].vals = []
    exp = mvreg_opgen.slab(regs, cap, A16)
    blobs = [MB.encode_mvreg(r, 1, 8) for r in regs]
    if cap == 64:
        assert max(map(len, blobs)) > LDS_WINDOW > min(map(len, blobs))  # both the window and the HBM walk
    t, bo, bl = _upload(blobs, rng)
    got = gpu.mvreg_from_bincode(t, bo, bl, A16, 1, 8, out=_patterned_regs(n, cap, A16))
    assert _same(got, exp)  # whole arrays: every unused slot zero-filled
    out, off, lens = gpu.mvreg_to_bincode(_dev(exp), A16, 1, 8)
    assert _blobs_of(out, off, lens) == blobs
    back = gpu.mvreg_from_bincode(out, off, lens, A16, 1, 8, out=_patterned_regs(n, cap, A16))
    assert _same(back, exp)


def test_mvreg_cap_128_and_narrow_widths(gpu):
    """One register of 128 values (crdt_mvreg_merge's HBM tier) among small ones, at (2, 4) byte widths."""
    rng = random.Random(128)
    regs = [mvreg_opgen.random_reg(rng, A16, 5, 1 << 30, val0=7 * i) for i in range(9)]
    big = crdts_ref.MVReg()
    big.vals = [(_vc([(a, 1 + v + a) for a in range(A16) if (v + a) % 3]), (1 << 32) - 1 - v) for v in range(128)]
    regs[4] = big
    exp = mvreg_opgen.slab(regs, 128, A16)
    blobs = [MB.encode_mvreg(r, 2, 4) for r in regs]
    t, bo, bl = _upload(blobs, rng)
    got = gpu.mvreg_from_bincode(t, bo, bl, A16, 2, 4, out=_patterned_regs(9, 128, A16))
    assert _same(got, exp)
    assert _blobs_of(*gpu.mvreg_to_bincode(got, A16, 2, 4)) == blobs
    merged = gpu.mvreg_merge(got, got, A16)  # the slab is the merge's input as it stands
    exp_m = []
    for r in regs:
        e = r.clone()
        e.merge(r)
        exp_m.append(e)
    assert all(np.array_equal(g, e) for g, e in zip(_host(merged), mvreg_opgen.slab(exp_m, 256, A16)))


def test_mvreg_errors(gpu):
    import crdts_hip

    rng = random.Random(9)
    regs = [mvreg_opgen.random_reg(rng, A16, 4, 1 << 20, val0=10 * i) for i in range(12)]
    regs[2].vals = [(_vc([(3, 5)]), 1), (_vc([(4, 5)]), 2)]
    good = [MB.encode_mvreg(r, 1, 8) for r in regs]
    two = good[2]
    bad = {
        1: (two[:-1], -2), 3: (two + b"\0", -2), 5: (two[:17] + bytes(8) + two[25:], -2),
        7: (struct.pack("<Q", 1 << 63) + two[8:], -2), 9: (two[:16] + b"\x10" + two[17:], -2),
        11: (MB.encode_mvreg(_reg([([(0, 1 + v)], v) for v in range(5)]), 1, 8), -4),
    }
    exp = list(mvreg_opgen.slab([crdts_ref.MVReg() if i in bad else r for i, r in enumerate(regs)], 4, A16))
    for i, (blob, code) in bad.items():
        blobs = list(good)
        blobs[i] = blob
        t, bo, bl = _upload(blobs, rng)
        with pytest.raises(crdts_hip.CrdtError) as e:
            gpu.mvreg_from_bincode(t, bo, bl, A16, 1, 8, out_cap=4)
        assert e.value.code == code, i
    blobs = [bad[i][0] if i in bad else b for i, b in enumerate(good)]
    t, bo, bl = _upload(blobs, rng)
    got = gpu.mvreg_from_bincode(t, bo, bl, A16, 1, 8, out=_patterned_regs(12, 4, A16), check_status=False)
    with pytest.raises(crdts_hip.CrdtError):
        gpu.status()
    h = _host(got)
    assert h[0].tolist() == exp[0].tolist()  # a faulty object's count is 0
    keep = [i for i in range(12) if i not in bad]
    assert np.array_equal(h[1][keep], exp[1][keep]) and np.array_equal(h[2][keep], exp[2][keep])
    # egest: a value that does not fit one byte, a count above the capacity
    S = list(mvreg_opgen.slab([_reg([([(0, 1)], 255)]), _reg([([(0, 1)], 256)]), _reg([([(1, 1)], 3)])], 2, A16))
    S[0][2] = 3
    with pytest.raises(crdts_hip.CrdtError) as e:
        gpu.mvreg_to_bincode(_dev(S), A16, 1, 1)
    assert e.value.code == crdts_hip.CRDT_ENONCANON
    out, off, lens = gpu.mvreg_to_bincode(_dev(S), A16, 1, 1, check_status=False)
    with pytest.raises(crdts_hip.CrdtError):
        gpu.status()
    assert lens.cpu().tolist() == [8 + 8 + 9 + 1, 0, 0]
    assert _blobs_of(out, off, lens)[0] == MB.encode_mvreg(_reg([([(0, 1)], 255)]), 1, 1)


# ------------------------------------------------------------------ end to end
def test_blobs_merge_blobs_on_the_device(gpu):
    """2 000 pairs: ingest both sides, crdt_map_mvreg_merge, egest; the decoded
    result equals the restatement's merge of the decoded inputs (Map.__eq__)."""
    n = 2000
    L, R = _batch()["states"][:n], gen_map_states(21, n, A16)
    rng = random.Random(22)
    lb = [MB.encode_map_mvreg(m, 1, 8, 8, rng=rng) for m in L]
    rb = [MB.encode_map_mvreg(m, 1, 8, 8, rng=rng) for m in R]
    S = gpu.map_mvreg_from_bincode(*_upload(lb, rng), A16, 1, 8, 8, out_caps=CAPS)
    O = gpu.map_mvreg_from_bincode(*_upload(rb, rng), A16, 1, 8, 8, out_caps=CAPS)
    M = gpu.map_mvreg_merge(S, O, A16)
    got = _blobs_of(*gpu.map_mvreg_to_bincode(M, A16, 1, 8, 8))
    bad = []
    for i, (a, b, g) in enumerate(zip(lb, rb, got)):
        e = MB.decode_map_mvreg(a, 1, 8, 8)
        e.merge(MB.decode_map_mvreg(b, 1, 8, 8))
        if not (MB.decode_map_mvreg(g, 1, 8, 8) == e):
            bad.append(i)
    assert not bad, f"{len(bad)} merges differ; first {bad[0]}"
    assert sum(bool(m.deferred) for m in R) > 50
