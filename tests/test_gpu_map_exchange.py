"""The reference's Map op-exchange properties (test/map.rs:518-745) on the
kernels: the output of one Map kernel is the input of the next, as device
slabs from the build to the end of the property (tests/map_exchange.py
GpuEngine) — crdt_map_mvreg_apply / _merge / _truncate, crdt_map_orswot_* and
crdt_map_map_* for Map<u64, MVReg>, Map<u64, Orswot> and Map<u64, Map<u64,
MVReg>>.

With S_i = B(o_i) one apply launch from the empty slab, P(S, o) an apply and
M(S, O) a merge, all cases batched per launch:

  build parity                         S1, S2, S3
  prop_op_exchange_same_as_merge :520  P(S1, o2) == M(S1, S2) == P(S2, o1)
  prop_op_exchange_converges :546      P(S1, o2) == P(S2, o1)
  prop_op_exchange_associative :574,
  prop_op_associative :620             P(P(S1, o2), o3) == P(P(S2, o3), o1)
  prop_op_idempotent :607              P(S1, o1) == S1
  prop_merge_commutative :688          M(S1, S2) == M(S2, S1)
  prop_merge_associative :654          M(M(S1, S2), S3) == M(S1, M(S2, S3))
  prop_merge_idempotent :716           M(S1, S1) == S1
  prop_truncate_with_empty_vclock_is_nop :732
                                       T(M(S1, S2)) == M(S1, S2), and M(T(..), S3)
  ops == merge, three replicas         P(P(S1, o2), o3) == M(M(S1, S2), S3)

Two checks on every slab a property makes, intermediate ones included:
  - parity: row-exact, in canonical form, against the restatement's state of
    the same expression packed at the slab's own capacities;
  - the property: the two sides decoded to restatement maps and compared with
    the reference's == (MVReg's PartialEq is set-like, src/mvreg.rs:74-100:
    the op path and the merge path order the values differently — how many
    cases do is compared with the restatement's count).
The status is read after every launch (a latched CRDT_ECAPACITY /
CRDT_ENONCANON fails the test), every output buffer held the fill pattern,
which must not show in a used key, value or set slot, and the capacities come
from the restatement's peak sizes alone (apply outputs: the peak, rounded up;
merge outputs: the sums — 3 x for the associativity chain, whose second
merges have sides of unequal capacities).

Shapes: 1000 cases of three op vectors (0-12 ops; keys from 4) at 16 actors
with the case's actors interned to 0..2; the first 200 of them at 100 actors
with the actors at {3, 50, 99} (two clock slots per lane); for the nested kind
300 more with keys from 2. Non-vacuity floors: map_exchange.assert_non_vacuous
(from restatement states; shares in tests/test_map_exchange_ref.py).

Order-sensitive cases (== with other canonical rows): P(S1, o2) and M(S1, S2)
hold their values in the same order in every case (0 cases: both put S1's
values first); P(S2, o1) and M(S1, S2) differ in 225 / 1000 (mvreg, 16
actors), 49 / 200 (mvreg, 100 actors), 5 / 1000, 1 / 200 and 6 / 300 (nested)
cases and in none with Orswot values, on the restatement and on the kernels."""
import pytest

import map_exchange as mx

pytestmark = pytest.mark.gpu
KIND_MODES = [(k, m) for k in mx.KINDS for m in mx.modes_of(k)]


def _run(gpu, kind, mode, exprs, pairs=()):
    ops, memo, caps, _ = mx.reference(kind, mode)
    n, A, _, _ = mx.MODES[mode]
    mx.assert_non_vacuous(kind, mode)
    eng = mx.GpuEngine(kind, gpu, A, caps)
    dev = {}
    for e in exprs:
        mx.evaluate(eng, ops, e, dev)
    assert eng.launches == len(dev)  # one launch per expression, the status read after each
    # ---- read back, only now; both checks run on every slab before anything is reported
    views, failed = {}, []
    for e, slab in dev.items():
        H = slab.host()
        assert mx.caps_of(kind, H) == mx.result_caps(caps, e)
        try:
            mx.assert_rows(kind, H, mx.pack(kind, memo[e], A, mx.caps_of(kind, H)), what=f"parity {mx.show(e)}")
        except AssertionError as err:
            failed.append(str(err))
        if mx.pattern_words(kind, H):
            failed.append(f"{mx.show(e)}: the fill pattern in {mx.pattern_words(kind, H)} used slots")
        views[e] = mx.unpack(kind, H)
    for x, y in pairs:
        what = f"property {mx.show(x)} == {mx.show(y)}"
        bad = [i for i, (a, b) in enumerate(zip(views[x], views[y])) if a != b]
        if bad:
            failed.append(f"{what}: fails in {len(bad)} / {n} cases, first {bad[:5]}")
        # == although the rows differ (only MVReg value order can): as often as on the restatement
        order = sum(mx.ordered(a) != mx.ordered(b) for a, b in zip(views[x], views[y])) - len(bad)
        if order != sum(mx.ordered(a) != mx.ordered(b) for a, b in zip(memo[x], memo[y])) or (kind == "orswot" and order):
            failed.append(f"{what}: {order} cases equal with other rows, not as on the restatement")
    assert not failed, "\n".join(failed)
    return views


@pytest.mark.parametrize("kind,mode", KIND_MODES)
def test_build_parity(kind, mode, gpu):
    """S1, S2, S3: one apply launch each from the empty slab, row-exact."""
    views = _run(gpu, kind, mode, [mx.S1, mx.S2, mx.S3])
    assert len(views) == 3


@pytest.mark.parametrize("prop", list(mx.PROPERTIES))
@pytest.mark.parametrize("kind,mode", KIND_MODES)
def test_property(kind, mode, prop, gpu):
    pairs, _ = mx.PROPERTIES[prop]
    views = _run(gpu, kind, mode, mx.expressions(prop), pairs)
    if prop == "op_exchange_same_as_merge" and kind != "orswot":
        # what makes the second comparison necessary: P(S2, o1) and M(S1, S2) are == with other rows
        assert sum(mx.ordered(a) != mx.ordered(b) for a, b in zip(views[mx.X2], views[mx.MM])) > 0
