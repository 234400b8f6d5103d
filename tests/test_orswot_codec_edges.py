"""CPU proof of the Orswot codec suite (tests/orswot_codec_edges.py), no GPU:
the restated walk (ingest_ref / egest_ref) equals both references — the
Python pair bincode_ref + records and the C++ oracle — on every object of
every batch; accepts() equals the C++ oracle's verdict on the whole malformed
matrix; every knob of MUTANTS changes at least FLOOR objects of the batch
meant for it (or is a stated exemption, asserted to change nothing); the
inputs of tests/test_gpu_bincode.py cannot see most of the compare knobs; the
census of every tier batch; and the placement bound holds on every object and
is tight, to its 16-byte rounding, on one object per term.

    python -m pytest tests/test_orswot_codec_edges.py -s -k wrong

prints the knob counts of DESIGN.md §3."""
import random

import pytest

import bincode_ref as BC
import orswot_codec_edges as ce
import records
from test_bincode_oracle import bincode_record_bound, extreme_state

FLOOR = ce.FLOOR
VALUE_IDS = ["%d_%d_%s" % (wa, wm, "wide" if w else "dense") for wa, wm, w in ce.VALUE_SHAPES]


def _cases():
    return [("value",) + s for s in ce.VALUE_SHAPES] + [("tier", n) for n in ce.TIER_SHAPES]


@pytest.mark.parametrize("key", _cases(), ids=lambda k: "-".join(map(str, k)))
def test_restatements_equal_both_references(oracle, key):
    c = ce.case(*key)
    wa, wm, A, sp = c["wa"], c["wm"], c["A"], c["sparse"]
    assert len(c["blobs"]) <= 2048
    for i, (blob, rec, canon) in enumerate(zip(c["blobs"], c["recs"], c["canon"])):
        assert ce.accepts(blob, wa, wm, A, sp) == 0, (key, i)
        assert ce.ingest_ref(blob, wa, wm, A, sp) == rec, (key, i)
        assert ce.ingest_ref(canon[:c["lens"][i]], wa, wm, A, sp) == rec, (key, i)
        assert oracle.bincode_verdict(blob, wa, wm, A, int(sp), cap=len(rec) + 64) == (0, rec), (key, i)
        assert ce.egest_ref(rec, wa, wm, A) == canon, (key, i)
        assert c["buf"][c["offs"][i]:c["offs"][i] + c["lens"][i]] == blob
    if key[0] == "value":  # every blob alignment, every edge counter and key the width holds
        assert {o & 15 for o in c["offs"]} == set(range(16))
        ctrs = {x for s in c["states"] for x in s["clock"].values()} | \
            {x for s in c["states"] for d in s["entries"].values() for _, x in d} | \
            {x for s in c["states"] for cl, _ in s["deferred"] for _, x in cl}
        keys = {m for s in c["states"] for m in s["entries"]} | {m for s in c["states"] for _, ms in s["deferred"] for m in ms}
        assert set(ce.pg.EDGE) <= ctrs
        assert {k for k in ce.pg.KEYS if k < 1 << (8 * wm)} | {(1 << (8 * wm)) - 1} <= keys


@pytest.mark.parametrize("variant", list(ce.VARIANTS))
def test_accepts_equals_the_oracle_on_the_matrix(oracle, variant):
    wa, wm = ce.MATRIX_W
    codes = {}
    for name, A, good, bad, past in ce.matrix(variant):
        assert ce.accepts(good, wa, wm, A) == 0 and oracle.bincode_verdict(good, wa, wm, A)[0] == 0
        want = ce.accepts(bad, wa, wm, A)
        got, rec = oracle.bincode_verdict(bad, wa, wm, A, cap=1 << 20)
        assert got == want, (variant, name, got, want)
        r = ce.ingest_ref(bad, wa, wm, A)
        assert (r == rec) if want == 0 else (r == want), (variant, name)
        codes[name] = want
    # all but the valid default blob and the blob that is bad only by where it lies are refused
    assert [n for n, c in codes.items() if c == 0] == ["len_24_zero_is_default", "past_the_buffer"]
    assert codes["length_high_word:entries"] == codes["length_high_word:deferred"] == ce.ECAPACITY
    assert ce.accepts(bytes(24), wa, wm, 16) == 0 and ce.ingest_ref(bytes(24), wa, wm, 16) == ce.rec_of(ce.state({}, {}), 16)


def test_capacity_edges_of_the_contract():
    """16 384 members and 1 024 deferred clocks are accepted, one more is CRDT_ECAPACITY."""
    rng = random.Random(3)
    for n, code in ((ce.XB_MEM, 0), (ce.XB_MEM + 1, ce.ECAPACITY)):
        assert ce.accepts(BC.encode(ce._members_state(rng, n, 8), 1, 8), 1, 8, 16) == code
    for n, code in ((ce.XB_DEF, 0), (ce.XB_DEF + 1, ce.ECAPACITY)):
        assert ce.accepts(BC.encode(ce._members_state(rng, 2, 2, n_def=n), 2, 2), 2, 2, 16) == code


def _changed_ingest(c, knob):
    K = ce.MUTANTS[knob]
    return sum(ce.ingest_ref(b, c["wa"], c["wm"], c["A"], c["sparse"], **K) != r for b, r in zip(c["blobs"], c["recs"]))


def _changed_egest(c, knob, wa=None, wm=None):
    K = ce.MUTANTS[knob]
    wa, wm = wa or c["wa"], wm or c["wm"]
    return sum(ce.egest_ref(r, wa, wm, c["A"], **K) != ce.egest_ref(r, wa, wm, c["A"]) for r in c["recs"])


def _changed_verdicts(kind, knob):
    wa, wm, A, items = ce.reject_batch(kind)
    return sum(ce.ingest_ref(b, wa, wm, A, **ce.MUTANTS[knob]) != (code or ce.ingest_ref(b, wa, wm, A))
               for b, code in items)


# knob -> the value batches meant for it ((wa, wm, wide)), or a tier / reject batch
D18, D88, W44, W88 = (1, 8, False), (8, 8, False), (4, 4, True), (8, 8, True)
MEANT = {
    "member_order_signed": [D18, D88, W88], "member_order_low32": [D18, D88, W88],
    "member_equal_on_low32": ["members"],
    "clock_order_counter_signed": list(ce.VALUE_SHAPES), "clock_order_counter_low32": list(ce.VALUE_SHAPES),
    "clock_order_counter_high32": list(ce.VALUE_SHAPES),
    "clock_order_actor_signed": [W44, W88, (8, 1, True)],
    "clock_order_longer_first": list(ce.VALUE_SHAPES),
    "set_order_signed": [D18, D88, W88], "set_equal_on_low32": [D18, D88, W88],
}
# a knob that cannot matter on a batch: asserted to change nothing there
EXEMPT = {
    # keys of 1, 2 and 4 bytes are below 2^63 (signed = unsigned) and have no high word
    "member_order_signed": [(1, 1, False), (2, 2, False), (4, 4, False), (8, 1, False), W44, (8, 1, True)],
    "set_order_signed": [(1, 1, False), (2, 2, False), (4, 4, False), (8, 1, False), W44, (8, 1, True)],
    "member_order_low32": [(1, 1, False), (2, 2, False), (4, 4, False), (8, 1, False), W44, (8, 1, True)],
    "set_equal_on_low32": [(1, 1, False), (2, 2, False), (4, 4, False), (8, 1, False), W44, (8, 1, True)],
    # 64 members or fewer are ranked in registers: duplicates show in the rank sum, no equality is taken
    "member_equal_on_low32": list(ce.VALUE_SHAPES),
    # dense batches of 16 actors: every actor is below 2^31
    "clock_order_actor_signed": [s for s in ce.VALUE_SHAPES if not s[2]],
}


def test_every_wrong_knob_changes_its_batch():
    table = {}
    for knob in ce.COMPARE_MUTANTS:
        for b in MEANT[knob]:
            c = ce.case("tier", b) if isinstance(b, str) else ce.case("value", *b)
            n = table[knob, b] = _changed_ingest(c, knob)
            assert n >= FLOOR, (knob, b, n)
        for b in EXEMPT.get(knob, ()):
            assert _changed_ingest(ce.case("value", *b), knob) == 0, (knob, b)
    for kind, knob in ce.REJECT_KINDS.items():
        n = table[knob, kind] = _changed_verdicts(kind, knob)
        assert n >= FLOOR, (knob, n)
        for other in ce.REJECT_KINDS.values():  # each reject batch is refused by one check only
            if other != knob:
                assert _changed_verdicts(kind, other) == 0, (kind, other)
    dense = [s for s in ce.VALUE_SHAPES if not s[2]]
    for b in dense:  # dense clocks of 16 slots with absent actors
        n = table["egest_emits_zero_slots", b] = _changed_egest(ce.case("value", *b), "egest_emits_zero_slots")
        assert n >= FLOOR, (b, n)
    for b in ce.VALUE_SHAPES[6:]:  # a sparse clock has no zero slots
        assert _changed_egest(ce.case("value", *b), "egest_emits_zero_slots") == 0
    # the 8-byte keys of the (1, 8) batch written as 1-byte members: refused, unless the check is skipped
    n = table["egest_width_check_skipped", "D18 at wm=1"] = _changed_egest(ce.case("value", *D18),
                                                                          "egest_width_check_skipped", 1, 1)
    assert n >= FLOOR
    assert all(_changed_egest(ce.case("value", *b), "egest_width_check_skipped") == 0 for b in ce.VALUE_SHAPES)
    for b in ((1, 1, False), (1, 8, False), (8, 1, False)):  # fields at every byte alignment of a dword
        n = table["egest_or_spills_neighbour", b] = _changed_egest(ce.case("value", *b), "egest_or_spills_neighbour")
        assert n >= FLOOR, (b, n)
    for (knob, b), n in table.items():
        print("%-28s %-22s %4d" % (knob, b, n))
    assert {k for k, _ in table} == set(ce.MUTANTS)


def test_old_style_inputs_cannot_see_most_compare_mutants():
    """The inputs of tests/test_gpu_bincode.py: the 20 000 generate_orswot(
    first_obj=5) states at (1, 8) and extreme_state. Their member keys are
    full 64-bit draws, so a wrong member order shows on every object; their
    counters stay below 2^40 and their actors below 2^10, so the counter,
    actor, prefix and equality knobs change nothing or next to nothing. The
    counts are asserted as upper bounds."""
    import crdts_hip

    (b, o), _ = crdts_hip.generate_orswot(20_000, first_obj=5, threads=16)
    recs = records.unpack_batch(b, o)
    rng = random.Random(7)
    sts = [records.decode(r) for r in recs]
    blobs = [BC.encode(dict(clock=s["clock"], entries=s["entries"], deferred=s["deferred"]), 1, 8, rng=rng) for s in sts]
    seen = {k: sum(ce.ingest_ref(x, 1, 8, 16, **ce.MUTANTS[k]) != r for x, r in zip(blobs, recs))
            for k in ce.COMPARE_MUTANTS}
    print(seen)
    assert seen["member_order_signed"] == seen["member_order_low32"] == 20_000
    for k, most in (("member_equal_on_low32", 0), ("clock_order_counter_signed", 0), ("clock_order_counter_low32", 0),
                    ("clock_order_actor_signed", 0), ("clock_order_longer_first", 0), ("set_equal_on_low32", 0),
                    ("set_order_signed", 14), ("clock_order_counter_high32", 378)):
        assert seen[k] <= most, (k, seen[k])
    # extreme_state: counters below 20, keys below 2^40, 400 states per width and clock form
    ext = dict.fromkeys(ce.COMPARE_MUTANTS, 0)
    for wa, wm in [(1, 1), (1, 8), (2, 2), (8, 1), (8, 8), (4, 2)]:
        for sparse in (False, True):
            rng = random.Random(wa * 10 + wm + sparse)
            A = 256 if sparse else 16
            for _ in range(400):
                s = extreme_state(rng, A, wa, wm)
                x, r = BC.encode(s, wa, wm), ce.rec_of(s, A, sparse)
                for k in ce.COMPARE_MUTANTS:
                    ext[k] += ce.ingest_ref(x, wa, wm, A, sparse, **ce.MUTANTS[k]) != r
    print(ext)
    for k in ("member_order_signed", "member_equal_on_low32", "clock_order_counter_signed", "clock_order_counter_low32",
              "clock_order_actor_signed", "set_order_signed", "set_equal_on_low32"):
        assert ext[k] == 0, (k, ext[k])


@pytest.mark.parametrize("name", ce.TIER_SHAPES)
def test_census(name):
    c = ce.assert_census(name)
    print(name, dict(c))


def test_chunks_cover_every_object_once():
    for n in (1, 5, 40, 41, 255, 256, 257, 348, 2048):
        ch = ce.chunks(n)
        assert [b for b, _ in ch] == [0] + [e for _, e in ch][:-1] and ch[-1][1] == n
        assert max(e - b for b, e in ch) <= 64
    assert max(e - b for b, e in ce.chunks(2048)) == 40  # a small batch never fills the 64 lanes of a chunk


def test_record_bound_holds_and_is_tight():
    """bc_record_bound on every object of the new batches, and its slope: the
    bound is 48 + 8 A + c L, c = max(12 / (wa + 8), 12 / (wm + 8), 8 / wm). Its
    constant part (48 + 24 c for the three length words every blob has,
    against the record's 32-byte header) keeps any record at least 32 bytes
    below it, so tightness is shown per term on the part that grows: a family
    of objects on which the record grows by exactly c bytes per blob byte, so
    that the slack between bound and record stays within one 16-byte rounding
    however large the object. 12 / (wm + 8) is below 8 / wm at every width and
    never binds."""
    for key in _cases():
        c = ce.case(*key)
        for n, r in zip(c["lens"], c["recs"]):
            assert len(r) <= bincode_record_bound(n, c["wa"], c["wm"], c["A"], c["sparse"]), key
    assert all(12 * wm < 8 * (wm + 8) for wm in (1, 2, 4, 8))

    def slack(st, wa, wm, A, sparse):
        return bincode_record_bound(ce.blob_len(st, wa, wm), wa, wm, A, sparse) - len(ce.rec_of(st, A, sparse))

    # 8 / wm (binds at wm = 1, 2, 4 and with wa >= 4): a deferred set of n members, wm blob bytes -> 8 record bytes each
    # 12 / (wa + 8) (binds at wm = 8, wa = 1, 2): a sparse top clock / a member's dots, wa + 8 blob bytes -> 12 each
    fam = {
        "8/wm": lambda n: slack(ce.state({}, {}, [([(0, 1)], list(range(n)))]), 8, 1, 16, False),
        "8/wm at (8, 8)": lambda n: slack(ce.state({}, {}, [([(0, 1)], list(range(n)))]), 8, 8, 16, False),
        "12/(wa+8) top clock": lambda n: slack(ce.state({a: 1 for a in range(n)}, {}), 1, 8, 256, True),
        "12/(wa+8) dots": lambda n: slack(ce.state({}, {7: [(a, 1) for a in range(n)]}), 2, 8, 256, False),
    }
    got = {k: (f(30), f(120), f(250)) for k, f in fam.items()}
    print(got)
    for k, v in got.items():
        assert min(v) >= 0 and max(v) - min(v) <= 16, (k, v)
