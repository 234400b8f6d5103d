"""The reference's Map op-exchange properties (test/map.rs:518-745) through the
op-exchange harness (tests/map_exchange.py) on the CPU: the Python restatement
for the three kinds (Map<u64, MVReg>, Map<u64, Orswot>, Map<u64, Map<u64,
MVReg>>), and the C++ oracle's Map handles for the two flat kinds, which must
agree with it state for state. tests/test_gpu_map_exchange.py runs the same
expressions on the kernels and compares with the restatement states made
here; the harness's own pieces (op conversion, slab packing, the pattern
check, the non-vacuity floors) are pinned here, where no GPU is needed."""
import numpy as np
import pytest

import map_exchange as mx
import map_kat_runner as mkr
import map_slab

KIND_MODES = [(k, m) for k in mx.KINDS for m in mx.modes_of(k)]
FLAT_MODES = [(k, m) for k, m in KIND_MODES if k != "nested"]


@pytest.mark.parametrize("kind,mode", KIND_MODES)
def test_properties_hold_on_the_restatement(kind, mode):
    """prop_op_exchange_same_as_merge, _converges, _associative,
    prop_op_idempotent, prop_op_associative, prop_merge_associative,
    _commutative, _idempotent, prop_truncate_with_empty_vclock_is_nop and ops
    == merge of three replicas: every generated case, 0 discarded, 0 failing."""
    ops, memo, caps, peak = mx.reference(kind, mode)
    n = mx.MODES[mode][0]
    assert all(len(o) == n for o in ops)
    for prop, (pairs, more) in mx.PROPERTIES.items():
        for e in mx.expressions(prop):
            assert len(memo[e]) == n
        for x, y in pairs:
            bad = [i for i, (a, b) in enumerate(zip(memo[x], memo[y])) if a != b]
            assert not bad, f"{prop}: {mx.show(x)} != {mx.show(y)} in {len(bad)} cases, first {bad[:5]}"
    # the truncated merge, merged on: T is the identity there too
    t, u = memo[mx.M(mx.T(mx.MM), mx.S3)], memo[mx.M(mx.MM, mx.S3)]
    assert all(mx.ordered(a) == mx.ordered(b) for a, b in zip(t, u))
    # the capacities hold every state the applies made, and the tripled ones the merges'
    assert all(p <= c for p, c in zip(peak, caps))
    for e, states in memo.items():
        rc = mx.result_caps(caps, e)
        assert all(s <= c for m in states for s, c in zip(mx.sizes(kind, m), rc)), mx.show(e)


@pytest.mark.parametrize("kind,mode", FLAT_MODES)
def test_oracle_engine_agrees(kind, mode, oracle):
    """The same expressions on the C++ oracle's handles (its Map has no
    truncate: that property runs on the restatement alone): every state
    equal to the restatement's, MVReg values in the same order."""
    ops, memo, caps, _ = mx.reference(kind, mode)
    A = mx.MODES[mode][1]
    wide = dict(kcap=0, mcap=0, vdcap=0, vscap=0, dcap=0, scap=0)
    wide.update({k: 3 * c for k, c in zip(mx.CAP_NAMES[kind], caps)})
    eng = mx.OracleEngine(kind, A, wide)
    got = {}
    for prop in mx.PROPERTIES:
        if prop == "truncate_with_empty_vclock_is_nop":
            continue
        for e in mx.expressions(prop):
            mx.evaluate(eng, ops, e, got)
    assert len(got) >= 14
    for e, hs in got.items():
        bad = [i for i, (a, b) in enumerate(zip(eng.view(hs), memo[e])) if mx.ordered(a) != mx.ordered(b)]
        assert not bad, f"{mx.show(e)}: {len(bad)} states differ, first {bad[:5]}"


@pytest.mark.parametrize("kind,mode", KIND_MODES)
def test_op_conversion_round_trips(kind, mode):
    """The op vectors in the generator's own form, applied as the old tests
    apply them, then renamed to the interned ids == the kernel op lists
    applied through map_opgen.apply_op / map_orswot_opgen.apply_op /
    map_kat_runner.apply_raw (the built maps S1..S3 of the reference run)."""
    n, A, spread, keys = mx.MODES[mode]
    ops, memo, _, _ = mx.reference(kind, mode)
    cases = mx.draw(kind, mx.MODES["a16"][0] if keys == 4 else n, keys)[:n]
    py = mkr.PyMapBackend()
    ids = mx.actor_ids(A, spread)
    assert len(set(ids)) == 3 and max(ids) < A
    for i, (acts, vecs) in enumerate(cases):
        fwd = mx.interning(acts, ids)
        assert sorted(fwd, key=fwd.get) == sorted(acts)  # order-preserving
        for j, vec in enumerate(vecs):
            m = py.new(kind)
            if kind == "nested":
                for op in vec:
                    mkr.apply_raw(m, op)
            else:
                mx.apply_ops(py, m, vec, kind)
            assert map_slab.actors_of(m) <= {acts[j]}
            assert mx.ordered(map_slab.relabel(m, fwd)) == mx.ordered(memo[mx.B(j)][i]), (i, j)
            assert len(ops[j][i]) == len(vec) <= 12


@pytest.mark.parametrize("kind,mode", KIND_MODES)
def test_non_vacuity(kind, mode):
    """The state shapes only the op path makes are there, and the op path and
    the merge path differ in MVReg value order — floors at half of the shares
    the restatement shows at the committed seeds (flat kinds 1234, nested 99;
    map_exchange.MEASURED), of the 3 n built maps / the n merges m1 ^ m2:

                          built maps                              m1 ^ m2
                deferred  inner def.  empty value  empty map  deferred  multi-value
    mvreg  a16    25.8 %      -          13.6 %      15.8 %    45.7 %     22.5 %
    mvreg  a100   25.8 %      -          12.5 %      16.0 %    46.5 %     24.5 %
    orswot a16    25.8 %      -          40.6 %      15.8 %    45.7 %     22.4 %
    orswot a100   25.8 %      -          37.2 %      16.0 %    46.5 %     22.0 %
    nested a16    26.0 %    29.7 %       51.7 %      16.9 %    47.4 %      0.5 %
    nested a100   23.5 %    32.0 %       54.5 %      16.0 %    46.5 %      0.5 %
    nested k2     25.0 %    22.3 %       40.9 %      16.2 %    46.0 %      2.0 %

    (empty value: an entry whose register has zero values / whose set is
    empty / whose inner map has no entries; k2: outer and inner keys drawn
    from 2, 300 cases — a multi-value inner register stays rare: 2.0 %.)
    Order-sensitive cases — P(S2, o1) == M(S1, S2) although the rows differ,
    in MVReg value order: mvreg 225 / 1000 and 49 / 200, nested 5 / 1000,
    1 / 200 and 6 / 300 (k2); P(S1, o2) and M(S1, S2) hold their values in the
    same order in every case, and with Orswot values == is row equality."""
    got = mx.assert_non_vacuous(kind, mode)
    assert set(mx.FLOORS[kind, mode]) <= set(got)
    assert got["order_sensitive_x1"] == 0
    if kind == "orswot":
        assert got["order_sensitive_x2"] == 0
    else:
        assert got["order_sensitive_x2"] > 0


@pytest.mark.parametrize("kind", mx.KINDS)
def test_pack_unpack_and_pattern_check(kind):
    """The expected-slab writer and the row decoder are inverse at the merge's
    capacities, and pattern_words sees the fill pattern in used slots only."""
    _, memo, caps, _ = mx.reference(kind, "a16")
    A = mx.MODES["a16"][1]
    states = memo[mx.MM][:200]
    H = mx.pack(kind, states, A, mx.result_caps(caps, mx.MM))
    assert mx.caps_of(kind, H) == tuple(2 * c for c in caps)
    assert all(mx.ordered(a) == mx.ordered(b) for a, b in zip(mx.unpack(kind, H), states))
    # a buffer that held the pattern before the state was written: unused slots keep it
    P = mx.pack(kind, states, A, mx.result_caps(caps, mx.MM))
    flat = P.inner if kind == "nested" else P  # (the nested kind: the inner maps' unused slots)
    for f, used in flat.used_masks().items():
        if flat.a[f].dtype == np.uint64:
            flat.a[f][~used] = mx.PATTERN
    assert any((flat.a[f] == mx.PATTERN).any() for f in mx.VALUE_FIELDS["orswot" if kind == "orswot" else "mvreg"])
    mx.assert_rows(kind, P, H)
    assert mx.pattern_words(kind, P) == 0
    i = next(i for i, m in enumerate(states) if m.entries)
    P.a["keys"][i, 0] = mx.PATTERN
    assert mx.pattern_words(kind, P) == 1
    P.a["keys"][i, 0] = mx.PATTERN * 0x100000001
    assert mx.pattern_words(kind, P) == 1
