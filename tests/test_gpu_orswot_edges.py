"""GPU parity of the Orswot kernels at u64 edges and at every tier boundary:
the join (crdt_orswot_merge_ex, dense and CSR), crdt_orswot_truncate and
crdt_orswot_apply on the structured inputs of tests/orswot_pairgen.py, where
every comparison the kernels make sits on an edge (counters around 2^32, 2^63
and 2^64 - 1, member keys 0 and 2^64 - 1 and keys that share a word, ties of
dots against top clocks and of deferred clocks against merged clocks), with a
small tail for the codec and the read path on the same states.
tests/test_orswot_pairgen.py proves without a GPU that these inputs tell a
right kernel from the wrong ones of pg.MUTANTS.

Bar: byte-exact against the C++ oracle for every object. Output buffers are
pre-filled with a pattern where the API takes an `out`, both orientations are
run, every launch is run twice on one context, and every test asserts that its
batch holds the intended objects per launch tier (pg.tier, pg.truncate_form),
so a launcher change that re-routes a shape fails here instead of silently
un-testing a kernel."""
import os
import random
import sys

import numpy as np
import pytest

import orswot_pairgen as pg
import read_ref
import records
import truncate_cases as T
from orswot_edge_cases import (apply_case, assert_apply_workspaces, assert_merge_tiers, assert_truncate_forms,
                               merge_case, truncate_case)

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import bincode_ref as BC  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5


def _dev(recs, A, sparse):
    import crdts_hip

    return crdts_hip.OrswotBatch.from_host(*records.pack_batch(recs), A, flags=crdts_hip.SPARSE_CLOCK if sparse else 0)


def _same(got, exp, what):
    assert len(got) == len(exp)
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    if bad:
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} / {len(exp)} objects differ; first {i}:\n"
                             f"gpu    {records.decode(got[i])}\noracle {records.decode(exp[i])}")


def _merge_twice(gpu, L, R, exp, what):
    """L ⊔ R into a pre-filled output, twice on one context -> the second launch's output batch."""
    for k in range(2):
        out = gpu.orswot_alloc_out(L, R)
        out.base.fill_(FILL)
        out.off.fill_(0x5A5A5A5A5A5A5A5A)
        _same(gpu.orswot_merge(L, R, out=out).records(), exp, f"{what}, launch {k}")
    return out


# ------------------------------------------------------------------ merge
# the list caps of test_mixed_batch_general_path_list_caps, for the shapes whose objects leave the first kernel
CAPS = {name: (65536, 8, 0) for name in ("A16_limits", "A160", "A16_big", "csr")}


@pytest.mark.parametrize("name", list(pg.MERGE_SHAPES))
def test_merge_edges(name, gpu, oracle):
    """Every merge shape of pg.MERGE_SHAPES: join5<6, 32> at A = 1, 16, 32
    (plain and deferred-remove objects, actor 31, 640 objects: static and
    ticket chunks) and at its limits (A16_limits: unions of 64 / 65 members,
    records of 2 048 / 2 064 bytes, 31 / 32 / 33 deferred clocks a side with
    the killing clock last); join5<5, 64> at A = 33, 64; the DN mask join,
    orswot_dense_wide_kernel and the general kernel at A = 65, 128, 160
    (present-actor unions of 64 / 65 / 128 / 129, pairs at and one piece past
    6 KB and 16 KB); A = 1024, the last width of the dense-wide launcher, and
    1025, the first on join5<5, 64>, where every record is past every stage;
    orswot_big_kernel's LDS, HBM and one-wave paths (the last a pair of
    270 000 union positions, keys 0 and 2^64 - 1 among them); CSR records over 1 024 actors (unions of 64 / 65
    actors and members, pairs at and past the 7 KB stage, one big pair, actor
    ids 0 and 1023)."""
    A, sparse, _, _, Ls, Rs, lr, rl = merge_case(name)
    assert_merge_tiers(name)
    L, R = _dev(Ls, A, sparse), _dev(Rs, A, sparse)
    gpu.orswot_validate(L)  # canonical inputs
    gpu.orswot_validate(R)
    try:
        for cap in CAPS.get(name, (65536,)):
            gpu.set_list_cap(cap)
            _merge_twice(gpu, L, R, lr, f"{name} self ⊔ other, list cap {cap}")
            _merge_twice(gpu, R, L, rl, f"{name} other ⊔ self, list cap {cap}")
    finally:
        gpu.set_list_cap(65536)


def test_csr_four_replica_fold(gpu, oracle):
    """((r0 ⊔ r1) ⊔ r2) ⊔ r3 over CSR edge records, every intermediate batch
    (gapped: out.off = self.off + other.off) fed back as it is; each step
    byte-exact against the oracle's fold, into a pre-filled output, twice."""
    import crdts_hip

    A, sparse, _, _, Ls, Rs, lr, _ = merge_case("csr")
    rng = random.Random(0xF01D)
    more = [[pg.encode(pg.pair(rng, A, n_def=(0, 2))[k], A, True) for _ in Ls] for k in (0, 1)]
    acc_g, acc_o = _dev(Ls, A, True), records.pack_batch(Ls)
    for step, recs in enumerate([Rs] + more):
        rb, ro = records.pack_batch(recs)
        acc_o = oracle.orswot_merge_batch(*acc_o, rb, ro, A, threads=16, flags=crdts_hip.SPARSE_CLOCK)
        exp = records.unpack_batch(*acc_o)
        acc_g = _merge_twice(gpu, acc_g, _dev(recs, A, True), exp, f"fold step {step}")
    assert exp[:len(lr)] != lr


# ------------------------------------------------------------------ truncate
def _truncate_twice(gpu, oracle, recs, clocks, A, sparse, what, exp=None):
    import crdts_hip

    lb, lo = records.pack_batch(recs)
    cn = T.clocks_csr(clocks)
    if exp is None:
        exp = records.unpack_batch(*oracle.orswot_truncate_batch(lb, lo, cn, A, int(sparse), threads=16))
    B, C = _dev(recs, A, sparse), crdts_hip.ClockBatch.from_host(*cn)
    for k in range(2):
        out = gpu.orswot_alloc_out(B, B)
        out.base.fill_(FILL)
        out.off.fill_(0x5A5A5A5A5A5A5A5A)
        got = gpu.orswot_truncate(B, C, out=out)
        _same(got.records(), exp, f"{what}, launch {k}")
        assert (got.off.cpu().numpy().view(np.uint64) == lo).all()
    return exp


@pytest.mark.parametrize("name", list(pg.TRUNCATE_SHAPES))
def test_truncate_edges(name, gpu, oracle):
    """crdt_orswot_truncate on edge states and edge truncating clocks, every
    form test_gpu_truncate.py distinguishes: the streaming fast form at
    A = 8, 16, 32 with 1..8 deferred clocks, each count held (next to records past its limits,
    listed, found by their flags and with no list); the single-pass and the
    two-pass LDS form (> 64 members, a member of > 4 dots); the HBM form at
    A = 40 (> 4 KB, > 8 deferred clocks); CSR records; and clock runs of more
    than 64 entries decided past their first 64. Members left with an EMPTY
    clock occur in every shape, and each output is truncated again by a clock
    aimed at it."""
    A, sparse, states, clocks, recs, exp = truncate_case(name)
    assert_truncate_forms(name)
    try:
        for cap in (65536, 8, 0) if name.startswith("fast") else (65536,):
            gpu.set_list_cap(cap)
            first = _truncate_twice(gpu, oracle, recs, clocks, A, sparse, f"{name}, list cap {cap}", exp)
    finally:
        gpu.set_list_cap(65536)
    assert sum(1 for r in first if np.frombuffer(r[28:32], np.uint32)[0] & pg.EMPTY_MEMBER_CLOCK) >= 20
    rng = random.Random(name)
    again = [pg.truncating_clock(rng, pg.state_of(r), A) for r in first]
    second = _truncate_twice(gpu, oracle, first, again, A, sparse, f"{name}, truncated again")
    assert second != first


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("name", list(pg.APPLY_SHAPES))
def test_apply_edges(name, gpu, oracle):
    """crdt_orswot_apply on edge states, dense and CSR, in the small and the
    large workspace (65..128 members dense and CSR, > 16 deferred clocks
    dense; counted by assert_apply_workspaces): Adds at exactly
    the top counter (stale), one edge step above it and at 2^64 - 1; removes
    whose context is the member's clock or one step past it; future-context
    removes left deferred and released by the Add at exactly that counter;
    members 0 and 2^64 - 1 added next to keys 1 and 2^64 - 2."""
    import crdts_hip

    A, sparse, states, ops, recs, exp = apply_case(name)
    assert_apply_workspaces(name)
    assert sum(e != r for e, r in zip(exp, recs)) > 0.7 * len(recs)
    B, O = _dev(recs, A, sparse), crdts_hip.OrswotOps.from_lists(ops)
    for k in range(2):
        _same(gpu.orswot_apply(B, O).records(), exp, f"{name}, launch {k}")


# ------------------------------------------------------------------ codec and reads on the same states
def _blobs(out, off, lens):
    host, o, n = out.cpu().numpy(), off.cpu().numpy(), lens.cpu().numpy()
    return [host[a:a + b].tobytes() for a, b in zip(o, n)]


@pytest.mark.parametrize("name", ["A16", "csr"])
def test_codec_round_trip_on_edge_records(name, gpu):
    """actor_bytes = member_bytes = 8: orswot_to_bincode of the edge records
    equals bincode_ref.encode, and orswot_from_bincode of the same states'
    blobs in shuffled map / set order gives the records back, in the packed
    and in the bounds-placed layout; every launch twice (neither call takes
    an `out`)."""
    import torch

    A, sparse, _, _, Ls, Rs, _, _ = merge_case(name)
    recs = [r for r in Ls + Rs if np.frombuffer(r[24:28], np.uint32)[0] <= 64]  # (not the sets grown to pad a record)
    sts = [records.decode(r) for r in recs]
    sts = [dict(clock=s["clock"], entries=s["entries"], deferred=s["deferred"]) for s in sts]
    B = _dev(recs, A, sparse)
    blobs = [BC.encode(s, 8, 8) for s in sts]
    for k in range(2):
        assert _blobs(*gpu.orswot_to_bincode(B, 8, 8)) == blobs, f"{name} egest, launch {k}"
    rng = random.Random(8)
    buf, off, ln = bytearray(), [], []
    for s in sts:
        b = BC.encode(s, 8, 8, rng=rng)
        buf += bytes(rng.randrange(6))
        off.append(len(buf))
        ln.append(len(b))
        buf += b
    t = torch.frombuffer(buf, dtype=torch.uint8).to("cuda:0")
    bo, bl = (torch.tensor(x, dtype=torch.int64, device="cuda:0") for x in (off, ln))
    for packed in (True, False, True, False):  # (each layout twice)
        got = gpu.orswot_from_bincode(t, bo, bl, A, 8, 8, flags=B.flags, packed=packed).records()
        _same(got, recs, f"{name} ingest, packed={packed}")


@pytest.mark.parametrize("name", ["A16", "csr"])
def test_contains_edge_keys(name, gpu):
    """Engine.orswot_read: contains() for keys 0, 2^64 - 1, each present
    member and its neighbours in the high and in the low word, present and
    absent, on edge states, against tests/read_ref.py."""
    import crdts_hip

    A, sparse, _, _, Ls, Rs, _, _ = merge_case(name)
    rng = random.Random(5)
    objs = [T.to_ref(pg.state_of(r)) for r in Ls]
    per = []
    for o in objs:
        ks = {0, pg.M64}
        for m in rng.sample(sorted(o.entries), min(3, len(o.entries))):
            ks |= {m, m ^ (1 << 32), m ^ (1 << 63), m ^ 1, m ^ (1 << 31)}
        per.append([("key", k) for k in sorted(ks)])
    q = crdts_hip.ReadQueries.from_lists(per)
    exp = read_ref.expect(objs, per, A)
    assert sum(e["val"] for e in exp) > len(objs) and sum(1 - e["val"] for e in exp) > len(objs)
    assert sum(e["val"] for e, qq in zip(exp, [x for p in per for x in p]) if qq[1] in (0, pg.M64)) >= 20
    for k in range(2):
        got = read_ref.answers(gpu.orswot_read(_dev(Ls, A, sparse), q, want=("val", "slot", "rm")), q.n_q)
        read_ref.assert_answers(got, exp, f"{name} contains, launch {k}")
