"""The host bookkeeping of the three Map slab classes — used_masks(),
used_bytes() and canonical() — pinned to literals on small seeded host slabs
(n = 3, A = 2, every capacity 2 or 3, every array nonzero noise, some slot of
every nested axis unused, key slots of the nested map dead)."""
import hashlib

import numpy as np

import crdts_hip

N, A = 3, 2


def _noise(slab, rng, counts):
    """Fill every array with nonzero noise, then the count fields: the given
    ones as they are, the others drawn in [0, the capacity of their axis]."""
    for f, v in slab.a.items():
        hi = 1 << 32 if v.dtype == np.uint32 else 1 << 63
        v[...] = rng.integers(1, hi, v.shape, dtype=np.uint64).astype(v.dtype)
    for f, c in counts.items():
        slab.a[f][...] = rng.integers(0, c + 1, slab.a[f].shape) if isinstance(c, int) else np.asarray(c)
    return slab


def _digest(slab):
    h = hashlib.sha256()
    for f in sorted(slab.a):
        v = slab.a[f]
        h.update(f.encode() + str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def _popcounts(slab):
    return {f: int(m.sum()) for f, m in slab.used_masks().items()}


def _map_slab():
    S = crdts_hip.MapSlab.alloc(N, A, 3, 2, 2, 3)  # kcap, mcap, dcap, scap
    return _noise(S, np.random.default_rng(0x51AB01), {
        "n_keys": [2, 0, 3], "mv_n": [[1, 2, 2], [2, 1, 0], [0, 2, 1]], "n_def": [1, 2, 0],
        "dset_n": [[2, 3], [0, 3], [1, 1]]})


def _map_orswot_slab():
    S = crdts_hip.MapOrswotSlab.alloc(N, A, kcap=3, mcap=2, vdcap=2, vscap=3, dcap=2, scap=2)
    return _noise(S, np.random.default_rng(0x51AB02), {
        "n_keys": [2, 0, 3], "vn_mem": [[1, 2, 2], [2, 1, 0], [0, 2, 1]], "vn_def": [[2, 0, 1], [1, 1, 1], [1, 2, 0]],
        "vdset_n": 3, "n_def": [1, 2, 0], "dset_n": [[2, 1], [0, 2], [1, 1]]})


def _map_map_slab():
    S = crdts_hip.MapMapSlab.alloc(N, A, 2, 2, 3, (3, 2, 2, 3))  # kcap, dcap, scap, inner (kcap, mcap, dcap, scap)
    rng = np.random.default_rng(0x51AB03)
    _noise(S, rng, {"n_keys": [1, 2, 0], "n_def": [2, 0, 1], "dset_n": [[1, 3], [2, 2], [0, 1]]})
    _noise(S.inner, rng, {"n_keys": 3, "mv_n": 2, "n_def": 2, "dset_n": 3})
    return S


def test_map_slab():
    S = _map_slab()
    # by hand: clock 3 x 2 x 8 = 48; n_keys, n_def 3 x 4 = 12 each; 2 + 0 + 3 = 5 used keys: keys 5 x 8 = 40,
    # eclock 5 x 2 x 8 = 80, mv_n 5 x 4 = 20; values of used keys (1 + 2) + 0 + (0 + 2 + 1) = 6: mv_val 6 x 8 = 48,
    # mv_clock 6 x 2 x 8 = 96; 1 + 2 + 0 = 3 deferred: dclock 3 x 2 x 8 = 48, dset_n 3 x 4 = 12; their set
    # elements 2 + (0 + 3) = 5: dset 5 x 8 = 40. 48 + 12 + 12 + 40 + 80 + 20 + 48 + 96 + 48 + 12 + 40 = 456
    assert S.used_bytes() == 456
    assert _popcounts(S) == MAP_POP
    C = S.canonical()
    assert (C.kcap, C.mcap, C.dcap, C.scap) == (3, 2, 2, 3)
    assert _digest(C) == MAP_SHA
    assert _digest(C.canonical()) == MAP_SHA and C.used_bytes() == 456


def test_map_orswot_slab():
    S = _map_orswot_slab()
    assert S.used_bytes() == MAP_ORSWOT_BYTES
    pop = _popcounts(S)
    assert pop == MAP_ORSWOT_POP
    assert all(0 < pop[f] < S.a[f].size for f in ("keys", "vmem", "vmclock", "vdclock", "vdset_n", "vdset", "dset"))
    C = S.canonical()
    assert C.caps == S.caps
    assert _digest(C) == MAP_ORSWOT_SHA
    assert _digest(C.canonical()) == MAP_ORSWOT_SHA and C.used_bytes() == MAP_ORSWOT_BYTES


def test_map_map_slab():
    S = _map_map_slab()
    assert int((np.arange(2)[None, :] >= S.a["n_keys"][:, None]).sum()) == 3  # dead key slots: nested maps unused
    assert S.used_bytes() == MAP_MAP_BYTES
    assert _popcounts(S.inner) == MAP_MAP_INNER_POP  # (of the inner slab on its own: dead key slots included)
    C = S.canonical()
    assert (C.kcap, C.dcap, C.scap, C.inner_caps) == (2, 2, 3, (3, 2, 2, 3))
    assert (_digest(C), _digest(C.inner)) == MAP_MAP_SHA
    assert (_digest(C.canonical()), _digest(C.canonical().inner)) == MAP_MAP_SHA and C.used_bytes() == MAP_MAP_BYTES
    dead = np.arange(2)[None, :] >= S.a["n_keys"][:, None]
    assert all(not v[dead.reshape(-1)].any() for v in C.inner.a.values())


# all taken from the implementation before the slab classes shared a base
MAP_POP = {"clock": 6, "n_keys": 3, "n_def": 3, "keys": 5, "eclock": 10, "mv_n": 5, "mv_clock": 12, "mv_val": 6,
           "dclock": 6, "dset_n": 3, "dset": 5}
MAP_SHA = "b5126feb2e7664f0aaeb8612a9c8a0f1c3b53aadb32aca1d1a0431c19a8de3bb"
MAP_ORSWOT_BYTES = 704
MAP_ORSWOT_POP = {"clock": 6, "n_keys": 3, "n_def": 3, "keys": 5, "eclock": 10, "vclock": 10, "vn_mem": 5, "vn_def": 5,
                  "vmem": 6, "vmclock": 12, "vdclock": 10, "vdset_n": 5, "vdset": 7, "dclock": 6, "dset_n": 3,
                  "dset": 4}
MAP_ORSWOT_SHA = "ad150edd52225d91a5441922e3dc38263ba7c2a9c83ada7b3fcf74eff2a87229"
MAP_MAP_BYTES = 708
MAP_MAP_INNER_POP = {"clock": 12, "n_keys": 6, "n_def": 6, "keys": 11, "eclock": 22, "mv_n": 11, "mv_clock": 20,
                     "mv_val": 10, "dclock": 6, "dset_n": 3, "dset": 3}
MAP_MAP_SHA = ("8ca5d273761d4c61ce8c5e934d38d249b68093351a488902a04eebffdbcbb3c4",
               "385981a2e98eaec747f3cfcb7c2733d8561db1a6fc1123f55b642ccfd79b6fff")
