"""CPU: tests/map_get_ref.py, the plain-Python restatement of the value of
Map::get for Map<u64, Orswot> and the nested map that tests/test_gpu_map_get.py
holds the kernels against, is itself held against tests/records.py and the
restatement's own states; every knob (one plausible wrong kernel each) is
caught by some case; and no batch passes on misses alone."""
import struct

import pytest

import crdts_ref
import map_get_ref as G
import records

CASES = [(kind, A) for A in G.PARITY_A for kind in ("orswot", "nested")] + [("edges", A) for A in G.EDGE_A]


def _id(c):
    return f"{c[0]}-A{c[1]}"


def _reference_record(o, A):
    rec = bytearray(records.from_py(o, A))
    if any(not c.dots for c in o.entries.values()):
        rec[28:32] = struct.pack("<I", struct.unpack_from("<I", rec, 28)[0] | G.EMPTY_MEMBER_CLOCK)
    return bytes(rec)


def _reference(b):
    out = []
    for i, q, k in G.flat_queries(b):
        m = b["maps"][i]
        v = m.entries[q[1]][1] if k is not None else None
        if b["kind"] == "nested":
            out.append((int(k is not None), v if v is not None else crdts_ref.Map(crdts_ref.MVReg)))
        else:
            out.append((int(k is not None), _reference_record(v if v is not None else crdts_ref.Orswot(), b["A"])))
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("fill", [False, True], ids=["zeroed", "garbage"])
def test_restatement_equals_the_reference_value(case, fill):
    b = G.batch(*case)
    got = G.expected(b, G.pack(b, fill))
    exp = _reference(b)
    assert len(got) == len(exp) == sum(len(qs) for qs in b["per_obj"])
    for j, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f"query {j}: {G.flat_queries(b)[j]}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_no_batch_passes_on_misses(case):
    b = G.batch(*case)
    flat = G.flat_queries(b)
    keyq = [k for _, q, k in flat if q[0] == "key"]
    assert 2 * sum(k is not None for k in keyq) >= len(keyq)
    assert any(k is None for k in keyq) and any(q[0] == "all" for _, q, _ in flat)
    lens = {len(qs) for qs in b["per_obj"]}
    assert {0, 70} <= lens or case[0] == "edges"
    n_keys = {len(m.entries) for m in b["maps"]}
    kcap = b["caps"][0][0] if b["kind"] == "nested" else b["caps"]["kcap"]
    assert {0, 1, kcap} <= n_keys or case[0] == "edges" and {0, 1, 8} <= n_keys


def _out_caps(b):
    return tuple(c + 1 + x for x, c in enumerate(b["caps"][1]))


@pytest.mark.parametrize("knob", G.KNOBS)
def test_every_knob_is_caught(knob):
    caught = []
    for case in CASES:
        b = G.batch(*case)
        if (b["kind"] == "nested") != (knob == "inner_out_stride"):
            continue
        S = G.pack(b)
        oc = _out_caps(b) if b["kind"] == "nested" else None
        if G.expected(b, S, knob, oc) != G.expected(b, S):
            caught.append(case)
    assert caught, knob
    if knob in ("actor_major", "dend_at_step", "inner_out_stride"):
        assert {A for _, A in caught} >= {64, 128}  # where a row ends on a 64-cell step, and a two-step row


def test_edges_reach_what_they_are_for():
    for A in G.EDGE_A:
        b = G.batch("edges", A)
        S = G.pack(b)
        recs = [r for p, r in G.expected(b, S) if p]
        hdr = [struct.unpack_from("<8I", r, 0) for r in recs]
        assert any(h[2] == 0 for h in hdr)                                 # no members
        assert any(h[2] == 16 and h[3] == 16 * A for h in hdr)             # mcap members of A dots each
        assert {(h[2] + h[3]) % 2 for h in hdr} == {0, 1}                  # the pad after mem_dend, and none
        raw = [len(r) for p, r in G.expected(b, S, "no_pad16") if p]
        assert {n % 16 for n in raw} >= {0, 8}                             # record ends before the padding
        assert any(h[4] == 3 and h[6] == 9 for h in hdr)                   # vdcap clocks with vscap-full sets
        assert sum(h[7] == G.EMPTY_MEMBER_CLOCK for h in hdr) == 1         # the member with an all-zero row
        words = {w for r in recs for w in struct.unpack_from(f"<{(len(r) - 32) // 8}Q", r, 32)}
        assert {0, 1, G.U64} <= words and {0, 1, G.U64} <= set(b["maps"][0].entries)
