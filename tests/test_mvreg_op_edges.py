"""The edge batches of the MVReg op path (tests/mvreg_op_edges.py) earn their
place without a GPU: the launch tiers are recomputed from the launcher's rule
and sit on both sides of every boundary, every outcome class and every named
extra Put has its floor, the structure batches cause the header reloads,
unstaged Puts and compactions they are there for (counted by a walk of the
physical slots, not read off their names), the three restatements agree, and
every deliberately wrong apply / truncate / read clock changes at least
FLOOR objects of every batch it can apply to — while the op-simulated inputs
of the older tests cannot see a 32-bit or a signed counter compare at all."""

import numpy as np
import pytest

import mvreg_op_edges as me
import mvreg_opgen as mo
from mvreg_opgen import crdts_ref

FLOOR = 20  # objects a mutant must change, ops of a class, objects of an extra: as in the Orswot and Map suites
PAIR = [n for n in me.NAMES if me.SPECS[n][0] is me.pair_batch]
CHAIN = [n for n in me.NAMES if me.SPECS[n][0] is me.chain_batch]
COMPACT = [n for n in me.NAMES if me.SPECS[n][0] is me.compact_batch]


# ------------------------------------------------------------------ tiers
def _waves(A, out_cap):
    """The launcher's rule written out once more, from the LDS layout: the
    waves per block that fit 60 KB, 0 for the general kernel."""
    pw = -(-(8 * out_cap * A + 8 * A + 8 * out_cap + out_cap) // 16) * 16
    return 0 if out_cap > 64 or pw > 61440 else min(4, 61440 // pw)


def test_tier_table():
    for A in list(range(1, 300)) + [767, 768, 2048]:
        for cap in (1, 3, 8, 16, 17, 18, 24, 25, 36, 37, 63, 64, 65, 100):
            w = _waves(A, cap)
            assert me.tier(A, cap) == (f"W{w}" if w else "general"), (A, cap)
    # out_cap 64: the boundaries along A; A = 100: the boundaries along out_cap
    assert me.tier_edges_by_A(64) == [(28, "W4", 29, "W3"), (38, "W3", 39, "W2"), (57, "W2", 58, "W1"),
                                      (117, "W1", 118, "general")]
    assert me.tier_edges_by_cap(100) == [(17, "W4", 18, "W3"), (24, "W3", 25, "W2"), (36, "W2", 37, "W1"),
                                         (64, "W1", 65, "general")]
    assert (me.tier(16, 64), me.tier(16, 65)) == ("W4", "general")
    assert me.per_wave_bytes(117, 64) == 61424 <= me.LDS_BYTES == 61440 < me.per_wave_bytes(118, 64) == 61936
    # every batch on a boundary is there with its neighbour, and the table holds every tier
    for lo, tl, hi, th in me.tier_edges_by_A(64):
        assert (me.batch(f"A{lo}-cap64")["tier"], me.batch(f"A{hi}-cap64")["tier"]) == (tl, th)
    for lo, tl, hi, th in me.tier_edges_by_cap(100):
        assert (me.batch(f"A100-cap{lo}")["tier"], me.batch(f"A100-cap{hi}")["tier"]) == (tl, th)
    assert {me.batch(n)["tier"] for n in PAIR} == {"W4", "W3", "W2", "W1", "general"}
    assert {me.batch(n)["A"] for n in PAIR} >= {1, 5, 16, 33, 63, 64, 65, 2048}
    assert [me.truncate_form(ns, 8) for ns in (0, 63, 64, 65, 1024)] == ["lane_element"] * 3 + ["lane_slot"] * 2


def test_truncate_forms():
    """Both forms of the truncate kernel, with registers of exactly 63, 64, 65 and 66 used slots."""
    b = me.batch("A8-cap100")
    ns = b["S"][0]
    forms = [me.truncate_form(int(k), b["A"]) for k in ns]
    assert forms.count("lane_element") >= FLOOR and forms.count("lane_slot") >= FLOOR
    assert all((ns == k).sum() >= 5 for k in (63, 64, 65, 66)), [(k, int((ns == k).sum())) for k in (63, 64, 65, 66)]
    for n in me.NAMES:
        if n != "A8-cap100":
            assert me.batch(n)["scap"] <= 64 or n == "compact-A5-cap70"


# ------------------------------------------------------------------ floors
@pytest.mark.parametrize("name", me.NAMES)
def test_class_floor(name):
    """Every outcome class of a Put holds >= FLOOR ops; every extra is in >=
    FLOOR objects of a pair batch; >= 5 % of the counters are >= 2^63 and some
    are 2^64 - 1; the unused input slots hold the poison word, the unused
    answer slots zero; no answer is without a neighbour of another size."""
    b = me.batch(name)
    assert all(b["classes"][c] >= FLOOR for c in mo.CLASSES), b["classes"]
    if name in PAIR:
        assert all(v >= FLOOR for v in b["extras"].values()), b["extras"]
    (sn, sclk, sval), (pn, pclk, _), (en, eclk, eval_) = b["S"], b["P"], b["E"]
    used = np.arange(b["scap"])[None, :] < sn[:, None]
    assert (sclk[~used] == me.POISON).all() and (sval[~used] == me.POISON).all()
    eused = np.arange(b["out_cap"])[None, :] < en[:, None]
    assert not eclk[~eused].any() and not eval_[~eused].any()
    nz = np.concatenate([sclk[used][sclk[used] > 0], pclk[pclk > 0]])
    assert (nz >= np.uint64(2**63)).mean() >= 0.05 and (nz == np.uint64(me.M64)).any()
    assert (nz >> np.uint64(32) == 0).any() and len(set(en.tolist())) >= 3
    assert b["census"]["peak"] <= b["out_cap"] and b["n"] >= 120
    if b["out_cap"] * b["A"] <= 4000 and name in PAIR:
        assert b["n"] == 300


def test_structure_census():
    """What the structure batches cause, counted by the walk of the physical slots."""
    for name in CHAIN:
        b, c = me.batch(name), me.batch(name)["census"]
        lens = b["P"][0].tolist()
        assert b["tier"] == "W4" and b["out_cap"] == 8 and {63, 64, 65, 130} == set(lens)
        # 65 Puts: one reload of the 64 op headers; 130: two; 63 and 64: none
        assert c["reloads"] == lens.count(65) + 2 * lens.count(130) >= 3 * FLOOR
        assert c["staged"] >= 1000 and c["unstaged"] >= 1000 and c["longest"] == 130
        both = 0
        for i in range(b["n"]):  # staged and unstaged Puts inside one 64-op chunk
            pairs = [int(np.count_nonzero(p)) for p, _ in me.puts_of(b, i)]
            both += any(0 < me.staging(pairs[k:k + 64])[1] and 0 < me.staging(pairs[k:k + 64])[2]
                        for k in range(0, len(pairs), 64))
        assert both >= FLOOR
    for name in COMPACT:
        b, c = me.batch(name), me.batch(name)["census"]
        assert c["compact_objs"] >= 4 * FLOOR and c["compact_mid"] >= 150 and c["peak"] == b["out_cap"], c
        if b["tier"] == "general":
            assert c["compact_end"] >= FLOOR
    fast = {n: me.batch(n)["tier"] for n in COMPACT}
    assert fast == {"compact-A5-cap64": "W4", "compact-A64-cap64": "W1", "compact-A100-cap64": "W1",
                    "compact-A5-cap70": "general", "compact-A200-cap40": "general"}
    assert me.batch("compact-A5-cap70")["census"]["over_64_used"] >= 100  # (general by out_cap; A200-cap40 by LDS)
    # the general kernel's 64-slot step loop runs twice; its end-of-list compaction
    g = me.batch("A8-cap100")
    assert g["tier"] == "general" and g["census"]["over_64_used"] >= FLOOR and g["census"]["compact_end"] >= FLOOR
    assert me.batch("A2048-cap3")["census"]["compact_mid"] >= FLOOR
    # the fast kernel's in-place compaction needs a full block: none outside the structure batches
    assert all(me.batch(n)["census"]["compact_mid"] == 0 for n in PAIR if me.batch(n)["tier"] != "general")


def test_tiled_batch_sizes():
    """The tiling rule of the GPU test: three objects per wave of the largest grid, values still apart."""
    b = me.batch(me.TILED)
    assert b["tier"] == "W4"
    n = 3 * me.fast_grid_waves(256) + 5
    S, P, E = me.tile(b, n)
    assert len(S[0]) == n and (S[1][b["n"]] == S[1][0]).all() and (E[0][b["n"]:2 * b["n"]] == b["E"][0]).all()
    k = int(np.nonzero(E[0] > 0)[0][0])
    assert E[2][k + b["n"], 0] == E[2][k, 0] + np.uint64(1 << 41)
    ends, val, cend, act, ctr = me.op_arrays(b["P"])
    import crdts_hip

    lists = [[([(int(a), int(c[a])) for a in np.nonzero(c)[0]], v) for c, v in me.puts_of(b, i)] for i in range(b["n"])]
    for got, exp in zip((ends, val, cend, act, ctr), crdts_hip.MVRegOps.arrays_from_lists(lists)):
        assert got.dtype == exp.dtype and (got == exp).all()


# ------------------------------------------------------ the restatements agree
def _reg(R, V):
    r = crdts_ref.MVReg()
    for row, v in zip(R, V):
        r.vals.append((crdts_ref.VClock([(int(a), int(row[a])) for a in np.nonzero(row)[0]]), int(v)))
    return r


def _pairs(c):
    return [(int(a), int(c[a])) for a in np.nonzero(c)[0]]


@pytest.mark.parametrize("name", me.NAMES)
def test_references_agree(name):
    """apply_ref with no knob == crdts_ref.MVReg.apply_put == mvreg_opgen.apply_ref, on every object: the
    answers of the batch are crdts_ref's; the same for truncate and the read clock."""
    b = me.batch(name)
    A, n = b["A"], b["n"]
    regs = [_reg(*me.reg_of(b, i)) for i in range(n)]
    ops = [[(_pairs(c), v) for c, v in me.puts_of(b, i)] for i in range(n)]
    after = mo.apply_ref(regs, ops)
    for e, p in zip(b["E"], mo.slab(after, b["out_cap"], A)):
        assert (e == p).all()
    one = regs[7].clone()
    for pairs, v in ops[7]:
        one.apply_put(crdts_ref.VClock(pairs), v)
    assert one.canonical() == after[7].canonical()
    T, ET = me.truncate_batch(name)
    out = []
    for i, r in enumerate(regs):
        r = r.clone()
        r.truncate(crdts_ref.VClock(_pairs(T[i])))
        out.append(r)
    for e, p in zip(ET, mo.slab(out, b["scap"], A)):
        assert (e == p).all()
    ER = me.read_batch(name)
    assert ER.shape == (n, A)
    for i in range(0, n, 3):
        assert _pairs(ER[i]) == mo.pairs_of(mo.fold(regs[i]))


def test_references_agree_with_cpp_oracle(oracle):
    """The C++ oracle's nested register (register i is the value of key 7 of a
    one-key OracleMap("mvreg"), every Put carried by an Op::Up with a fresh dot
    of an actor of the Ups' own) against apply_ref, from the empty register:
    the stored rows of the batch first, as Puts, then its Put list."""
    b = me.batch("A5-cap16")
    A, key, cap = b["A"], 7, b["scap"] + b["P"][1].shape[1]
    for i in range(0, b["n"], 2):
        R, V = me.reg_of(b, i)
        puts = list(zip(R, V)) + me.puts_of(b, i)
        h = oracle.OracleMap("mvreg")
        for d, (c, v) in enumerate(puts):
            h.apply_up_mvreg((A, d + 1), key, _pairs(c), v)
        M = h.slab(A + 1, dict(kcap=1, mcap=cap, dcap=1, scap=1))
        eR, eV = me.apply_ref(np.zeros((0, A), np.uint64), [], puts)
        if int(M.a["n_keys"][0]):
            k = int(M.a["mv_n"][0, 0])
            assert (M.a["mv_clock"][0, 0, :k, :A] == eR).all() and M.a["mv_val"][0, 0, :k].tolist() == eV, i
        else:
            assert not eV, i


# ---------------------------------------------------------------- the mutants
def _exempt_apply(mutant, b):
    """Why a wrong apply cannot change a batch (None: it must change FLOOR objects)."""
    if b["A"] == 1 and mutant == "skip_on_concurrent":
        return "one actor: clocks are totally ordered, no survivor is concurrent with the Put"
    if b["A"] == 1 and mutant == "unnamed_actor_blind":
        return "one actor: a non-empty Put names every actor"
    if mutant == "append_before_drop" and b["census"]["full_puts"] == 0:
        return "no register of the batch ever holds out_cap values"
    return None


TABLE = {}


@pytest.mark.parametrize("name", me.NAMES)
def test_wrong_applies_differ(name):
    b = me.batch(name)
    for mutant, knobs in me.APPLY_MUTANTS.items():
        d = me.apply_differs(b, **knobs)
        TABLE[("apply", name, mutant)] = d
        if _exempt_apply(mutant, b):
            assert d == 0, (mutant, d)
        else:
            assert d >= FLOOR, (mutant, d)


@pytest.mark.parametrize("name", me.NAMES)
def test_wrong_truncates_and_reads_differ(name):
    """No exemption: every batch has counters on both sides of 2^32 and 2^63 in one column."""
    b = me.batch(name)
    for kind, mutants, differs in (("truncate", me.TRUNCATE_MUTANTS, me.truncate_differs),
                                   ("read", me.READ_MUTANTS, me.read_differs)):
        for mutant, knobs in mutants.items():
            d = differs(b, **knobs)
            TABLE[(kind, name, mutant)] = d
            assert d >= FLOOR, (kind, mutant, d)


def test_wrong_kernels_table():
    """`-s -k wrong` prints what every mutant changes, batch by batch (objects)."""
    for kind, mutants in (("apply", me.APPLY_MUTANTS), ("truncate", me.TRUNCATE_MUTANTS), ("read", me.READ_MUTANTS)):
        names = [n for n in me.NAMES if (kind, n, next(iter(mutants))) in TABLE]
        if not names:
            continue
        print(f"\n{kind}: objects changed (of n)\n" + " " * 24 + "n tier    "
              + " ".join(m[-12:].rjust(12) for m in mutants))
        for n in names:
            b = me.batch(n)
            print(f"{n:20s} {b['n']:4d} {b['tier']:7s} " + " ".join(f"{TABLE[(kind, n, m)]:12d}" for m in mutants))
    print("\ncensus\n" + "\n".join(f"{n:20s} {me.batch(n)['tier']:7s} {me.batch(n)['classes']} {me.batch(n)['census']}"
                                  for n in me.NAMES))


# ---------------------------------------------- what the older inputs cannot see
def _dense(pairs, A):
    c = np.zeros(A, np.uint64)
    for a, x in pairs:
        c[a] = x
    return c


def test_old_style_inputs_cannot_see_the_compare_mutants():
    """On the op-simulated batches of tests/test_gpu_mvreg_ops.py as they are
    (mvreg_opgen.gen_batch at its (A, cap, hi); the truncate / read clock
    registers of _truncate_reference), a compare of the low words and a signed
    compare give the right answer on every object: every counter is below
    2^31, where the three compares are the same function. Exact, not a bound."""
    from test_gpu_mvreg_ops import SHAPES, _truncate_reference

    for A, cap, hi in [(8, 4, 3), (16, 8, 2), (64, 3, 4), (5, 16, 2), (1, 4, 3)]:
        b = mo.gen_batch(0xA000 + 100 * A + cap, 400, A, cap, hi, 0, 8)  # (the first 400 objects of the 20,000)
        S, E = mo.slab(b["regs0"], cap, A), mo.slab(b["regs"], cap + 8, A)
        assert int(S[1].max()) < 2**31 and max((c for ops in b["ops"] for p, _ in ops for _, c in p), default=0) < 2**31
        for i in range(400):
            puts = [(_dense(p, A), v) for p, v in b["ops"][i]]
            exp = me.answer_of(E, i)
            for compare in (None, "low32", "signed"):
                assert me._same(me.apply_ref(S[1][i, :S[0][i]], S[2][i, :S[0][i]], puts, compare=compare), exp), (A, i)
    for A, cap, n in SHAPES:
        S, T, E = _truncate_reference(A, cap, n)
        assert int(S[1].max()) < 2**31 and int(T.max()) < 2**31
        for i in range(min(n, 400)):
            R, V = S[1][i, :S[0][i]], S[2][i, :S[0][i]]
            for compare in (None, "low32", "signed"):
                assert me._same(me.truncate_ref(R, V, T[i], compare=compare), me.answer_of(E, i)), (A, i)
                assert (me.read_clock_ref(S[1][i], int(S[0][i]), compare=compare)
                        == me.read_clock_ref(S[1][i], int(S[0][i]))).all()
