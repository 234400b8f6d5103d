"""The structured MVReg pair generator (tests/mvreg_pairgen.py) earns its
place without a GPU: at every shape the GPU parity tests use, each outcome
class of the merge (src/mvreg.rs:121-153) holds a floor share of the slots,
the C++ oracle, the Python restatement and a brute-force count agree on the
batch, and every deliberately wrong merge differs from the oracle wherever it
can. The same for the partial_cmp rows (src/vclock.rs:59-71)."""
import functools

import numpy as np
import pytest

import mvreg_opgen as mo
import mvreg_pairgen as pg

ALL = pg.SHAPES + pg.EXTRA_SHAPES
CMP_A = (1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 300, 1000)


@functools.lru_cache(maxsize=None)
def batch(shape):
    """-> (S, O, info, oracle's merge at out_cap = scap + ocap): made once, read-only."""
    import oracle_ffi

    A, scap, ocap, n, _ = shape
    info = {}
    S, O = pg.gen(0x9000 + 7 * A + 3 * scap + ocap, n, A, scap, ocap, info)
    E = oracle_ffi.mvreg_merge(*S, *O, A, scap + ocap)
    for x in (*S, *O, *E):
        x.flags.writeable = False
    return S, O, info, E


@functools.lru_cache(maxsize=None)
def _relations(shape, key):
    S, O, _, _ = batch(shape)
    return pg.relations(S, O, key)


def test_tiers_of_the_table():
    """Every launch tier is in the table: 4, 3, 2 and 1 waves per block, both
    sides of the 64-slot and of the 60 KB boundary."""
    for A, scap, ocap, _, t in ALL:
        assert pg.tier(A, scap, ocap) == t, (A, scap, ocap)
    assert {s[4] for s in pg.SHAPES} == {"W4", "W3", "W2", "W1", "big"}
    assert [pg.per_wave_bytes(A, 4, 4) for A in (300, 400, 600)] == [(64 * A + 40 + 15) & ~15 for A in (300, 400, 600)]
    assert pg.per_wave_bytes(767, 5, 5) == 61424 <= pg.LDS_BYTES < pg.per_wave_bytes(768, 5, 5) == 61504


@pytest.mark.parametrize("shape", ALL, ids=pg.shape_id)
def test_class_floor(shape):
    """Each outcome class holds >= 1 % of its side's used slots and >= 20
    slots; >= 20 duplicates inside self; >= 5 % of the nonzero counters are
    >= 2^63; every hot slot is touched.

    Two shapes cannot meet a floor by arithmetic, not by the generator:
    * self_cap 1 has no duplicates inside self;
    * (4, 1024, 8) at 8 objects has at most 48 used slots on the other side,
      fewer than four classes of 20: there the classes are counted over
      merge(S, O) and merge(O, S) together, both of which the GPU test runs."""
    A, scap, ocap, n, _ = shape
    S, O, info, _ = batch(shape)
    c, _ = pg.classify(S, O)
    used_s, used_o = int(S[0].sum()), int(O[0].sum())
    if (A, scap, ocap) == (4, 1024, 8):
        assert 6 * ocap < 4 * 20
        c2, _ = pg.classify(O, S)
        c = {k: c[k] + c2[k] for k in c}
        used_s = used_o = used_s + used_o
    for k in pg.CLASSES:
        used = used_s if k.startswith("self") else used_o
        assert c[k] >= 20 and c[k] >= 0.01 * used, (k, c, used_s, used_o)
    assert sum(c[k] for k in pg.CLASSES) == used_s + used_o
    assert c["dup_in_self"] >= (20 if scap > 1 else 0), c
    nz = np.concatenate([S[1][S[1] > 0], O[1][O[1] > 0]])
    assert (nz >= np.uint64(2**63)).mean() >= 0.05
    assert all(info["touched"].get(h, 0) >= 1 for h in pg.hot(A)), (pg.hot(A), info["touched"])
    # the forced objects, and values that are unique with the high bit set
    assert (S[0][:4].tolist(), O[0][:4].tolist()) == ([scap, 0, scap, 0], [ocap, ocap, 0, 0])
    vals = np.concatenate([S[2][S[2] > 0], O[2][O[2] > 0]])
    assert len(vals) == int(S[0].sum()) + int(O[0].sum()) == len(np.unique(vals))
    assert (vals >= np.uint64(2**63)).all()


@pytest.mark.parametrize("shape", ALL, ids=pg.shape_id)
def test_references_agree(shape):
    """The C++ oracle, the Python restatement (crdts_ref.MVReg.merge) and the
    numpy restatement give identical slabs, order included; the output counts
    are the brute-force classification's."""
    A, scap, ocap, n, _ = shape
    S, O, _, E = batch(shape)
    regs = mo.regs_of(*S)
    for r, o in zip(regs, mo.regs_of(*O)):
        r.merge(o)
    for name, e, p, m in zip(("n", "clk", "val"), E, mo.slab(regs, scap + ocap, A), pg.merge_np(S, O, scap + ocap)):
        assert (e == p).all(), f"{name}: oracle vs crdts_ref"
        assert (e == m).all(), f"{name}: oracle vs numpy"
    assert (pg.classify(S, O)[1] == E[0]).all()
    assert len(set(E[0].tolist())) >= min(4, scap + ocap)


@pytest.mark.parametrize("mutant", sorted(pg.MUTANTS))
@pytest.mark.parametrize("shape", ALL, ids=pg.shape_id)
def test_wrong_merges_differ(shape, mutant):
    """A merge that is wrong in one way gives another slab than the oracle on
    this very batch, wherever it can. It cannot: ignoring slots >= 64 at
    A <= 64; the order of the sides at A = 1, where clocks are totally ordered
    and only one side survives."""
    A, scap, ocap, n, _ = shape
    knobs, can = pg.MUTANTS[mutant]
    S, O, _, E = batch(shape)
    got = pg.merge_np(S, O, scap + ocap, rel=_relations(shape, knobs.get("key")), **knobs)
    differs = sum(int((g != e).reshape(n, -1).any(axis=1).sum()) for g, e in zip(got, E))
    if (A, scap, ocap) == (4, 1024, 8):  # 8 objects: counted over both orientations, as the class floor is
        import oracle_ffi

        got, exp = pg.merge_np(O, S, scap + ocap, **knobs), oracle_ffi.mvreg_merge(*O, *S, A, scap + ocap)
        differs += sum(int((g != e).reshape(n, -1).any(axis=1).sum()) for g, e in zip(got, exp))
    if can(A):
        assert differs >= 1, (mutant, differs)
    else:
        assert differs == 0, (mutant, differs)


# ------------------------------------------------------------- partial_cmp
@functools.lru_cache(maxsize=None)
def cmp_batch(A):
    import oracle_ffi

    a, b = pg.cmp_rows(0xC0 + A, A)
    e = oracle_ffi.partial_cmp_rows(a, b, A)
    for x in (a, b, e):
        x.flags.writeable = False
    return a, b, e


@pytest.mark.parametrize("A", CMP_A)
def test_cmp_rows_references_agree(A):
    """Per slot the four pairs give Equal, Greater, Less and None in turn (at
    A = 1 the fourth is Greater); the oracle and numpy agree."""
    a, b, e = cmp_batch(A)
    assert len(a) == 4 * A + 3 and len(a) % 2 == 1
    assert (e == pg.cmp_np(a, b)).all()
    assert e[:4 * A].reshape(A, 4).tolist() == [[0, 1, -1, 2 if A > 1 else 1]] * A
    assert set(e.tolist()) == ({0, 1, -1, 2} if A > 1 else {0, 1, -1})
    both = np.concatenate([a, b])
    assert (both >= np.uint64(2**63)).any() and (both == np.uint64(2**64 - 1)).any()
    assert (a != b).any(axis=0).all()  # every slot decides some pair


@pytest.mark.parametrize("mutant", sorted(pg.CMP_MUTANTS))
@pytest.mark.parametrize("A", CMP_A)
def test_wrong_compares_differ(A, mutant):
    knobs, can = pg.CMP_MUTANTS[mutant]
    a, b, e = cmp_batch(A)
    differs = int((pg.cmp_np(a, b, **knobs) != e).sum())
    if can(A):
        assert differs >= 2, (mutant, differs)
    else:
        assert differs == 0
