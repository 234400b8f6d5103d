"""The reference-shaped host objects — Orswot, VClock, GCounter, PNCounter —
whose `merge` runs on the GPU, `merge_batch` over them, the process's default
Engine and the build record of the loaded library."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._lib import CRDT_ECAPACITY, CRDT_ENONCANON, LIB_PATH, SPARSE_CLOCK, CrdtError, check, lib
from ._util import _torch
from .batches import OrswotBatch
from .record import decode_record


class HostOrswot:
    """Host Orswot built through the reference's op path (src/orswot.rs:61-85)."""

    def __init__(self, handle=None):
        self.h = C.c_void_p(handle) if handle is not None else C.c_void_p(lib.crdt_host_orswot_new())

    def __del__(self):
        if getattr(self, "h", None) is not None and lib is not None:
            lib.crdt_host_orswot_free(self.h)
            self.h = None

    def clone(self):
        return HostOrswot(lib.crdt_host_orswot_clone(self.h))

    def apply_add(self, actor, counter, member):
        check(lib.crdt_host_orswot_apply_add(self.h, actor, counter, member), "apply_add")

    def apply_rm(self, member, clock_pairs):
        n = len(clock_pairs)
        a = (C.c_uint32 * max(1, n))(*[int(x) for x, _ in clock_pairs])
        c = (C.c_uint64 * max(1, n))(*[int(y) for _, y in clock_pairs])
        check(lib.crdt_host_orswot_apply_rm(self.h, member, a, c, n), "apply_rm")

    def encode(self, n_actors, flags=0):
        cap = 1 << 14
        while True:
            buf = (C.c_uint8 * cap)()
            n = lib.crdt_host_orswot_encode_ex(self.h, n_actors, flags, buf, cap)
            if n == CRDT_ECAPACITY:
                cap *= 4
                continue
            check(n if n < 0 else 0, "encode")
            return bytes(buf[:n])

    @staticmethod
    def decode(rec: bytes):
        arr = (C.c_uint8 * len(rec)).from_buffer_copy(rec)
        h = lib.crdt_host_orswot_decode(arr, len(rec))
        if not h:
            raise CrdtError(CRDT_ENONCANON, "decode")
        return HostOrswot(h)


def build_record():
    """The loaded library's sha256 and, if present, the build record written
    by __graft_entry__.build() (rust-crdt_amd/lib/build_info.json): whether
    the library in use is the one that build produced."""
    import hashlib
    import json

    with open(LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    rec = {"loaded": os.path.relpath(LIB_PATH, os.path.dirname(os.path.dirname(LIB_PATH))), "sha256": sha}
    info = os.path.join(os.path.dirname(LIB_PATH), "build_info.json")
    try:
        with open(info) as f:
            b = json.load(f)
        rec.update(built_sha256_matches=b.get("sha256") == sha, built_from=b.get("git_head"),
                   built_dirty=b.get("git_dirty"), built_at=b.get("built_at"), built_on=b.get("host"))
    except (OSError, ValueError):
        rec["build_info"] = None
    return rec


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        from .engine import Engine

        _default_engine = Engine(0)
    return _default_engine


class Orswot:
    """Reference-shaped Orswot (src/orswot.rs:26-30) whose `merge` runs on the GPU.

    `n_actors` is the dense top-clock width used when the state crosses the
    C ABI (actors must be interned to ids < n_actors); with sparse=True the
    top clock crosses as CSR and n_actors is only the actor-id universe.
    """

    def __init__(self, n_actors=16, host=None, sparse=False):
        self.n_actors = n_actors
        self.sparse = bool(sparse)
        self.host = host or HostOrswot()

    @property
    def flags(self):
        return SPARSE_CLOCK if self.sparse else 0

    def clone(self):
        return Orswot(self.n_actors, self.host.clone(), self.sparse)

    def apply_add(self, actor, counter, member):  # CmRDT::apply Op::Add
        self.host.apply_add(actor, counter, member)

    def apply_rm(self, member, clock_pairs):  # CmRDT::apply Op::Rm
        self.host.apply_rm(member, clock_pairs)

    def merge(self, other: "Orswot", engine=None):  # CvRDT::merge
        merge_batch([self], [other], engine)

    def state(self):
        return decode_record(self.host.encode(self.n_actors, self.flags))

    def clock(self):
        return sorted(self.state()["clock"].items())

    def entry(self, member):
        e = self.state()["entries"].get(member)
        return None if e is None else list(e)

    def value(self):
        return sorted(self.state()["entries"])

    def deferred_len(self):
        return len(self.state()["deferred"])

    def record(self):
        return self.host.encode(self.n_actors, self.flags)


def merge_batch(selfs, others, engine=None):
    """`merge_batch(&mut [T], &[T])`: selfs[i].merge(&others[i]) for every i, one kernel launch."""
    if len(selfs) != len(others):
        raise CrdtError(-1, "merge_batch length mismatch")
    if not selfs:
        return
    eng = engine or default_engine()
    kinds = {type(x) for x in selfs} | {type(x) for x in others}
    if kinds == {Orswot}:
        n_actors = max(x.n_actors for x in list(selfs) + list(others))
        fl = SPARSE_CLOCK if any(x.sparse for x in list(selfs) + list(others)) else 0
        L = OrswotBatch.from_records([x.host.encode(n_actors, fl) for x in selfs], n_actors, eng.device, fl)
        R = OrswotBatch.from_records([x.host.encode(n_actors, fl) for x in others], n_actors, eng.device, fl)
        out = eng.orswot_merge(L, R)
        for x, rec in zip(selfs, out.records()):
            x.host = HostOrswot.decode(rec)
        return
    if kinds <= {VClock, GCounter, PNCounter} and len(kinds) == 1:
        kind = {VClock: "vclock", GCounter: "gcounter", PNCounter: "pncounter"}[kinds.pop()]
        n_actors = max(x.n_actors for x in list(selfs) + list(others))
        torch = _torch()
        a = torch.from_numpy(np.stack([x.row(n_actors) for x in selfs]).view(np.int64)).to(f"cuda:{eng.device}")
        b = torch.from_numpy(np.stack([x.row(n_actors) for x in others]).view(np.int64)).to(f"cuda:{eng.device}")
        eng.dense_merge(a, b, n_actors, kind)
        rows = a.cpu().numpy().view(np.uint64)
        for x, r in zip(selfs, rows):
            x.set_row(r, n_actors)
        return
    raise CrdtError(-1, f"merge_batch: unsupported element types {kinds}")


class VClock:
    """Reference-shaped VClock (src/vclock.rs:54-57) over interned actor ids."""

    def __init__(self, dots=None, n_actors=16):
        self.n_actors = n_actors
        self.dots = {}
        for a, c in (dots or []):
            self.witness(a, c)

    def get(self, a):
        return self.dots.get(a, 0)

    def witness(self, a, c):  # src/vclock.rs:159-163
        if not (self.get(a) >= c):
            self.dots[a] = int(c)

    def merge(self, other, engine=None):
        merge_batch([self], [other], engine)

    def truncate(self, other):  # Causal::truncate, src/vclock.rs:103-120
        kept = {}
        for a, c in self.dots.items():
            m = min(c, other.get(a))
            if m > 0:
                kept[a] = m
        self.dots = kept

    def subtract(self, other):  # src/vclock.rs:236-242
        for a, c in other.dots.items():
            if c >= self.get(a):
                self.dots.pop(a, None)

    def intersection(self, other):  # src/vclock.rs:219-228
        v = VClock(n_actors=self.n_actors)
        v.dots = {a: c for a, c in self.dots.items() if other.get(a) == c}
        return v

    def row(self, n):
        r = np.zeros(n, dtype=np.uint64)
        for a, c in self.dots.items():
            r[a] = c
        return r

    def set_row(self, r, n):
        self.dots = {a: int(r[a]) for a in range(n) if r[a]}


class GCounter(VClock):
    """src/gcounter.rs:26-28 — one VClock; value() = sum (:76-78)."""

    def inc(self, actor):
        return (actor, self.get(actor) + 1)

    def apply(self, dot):
        self.witness(*dot)

    def value(self):
        return sum(self.dots.values()) & 0xFFFFFFFFFFFFFFFF


class PNCounter:
    """src/pncounter.rs:33-36 — P and N GCounters, merged together as one [P|N] row."""

    def __init__(self, n_actors=16):
        self.n_actors = n_actors
        self.p = GCounter(n_actors=n_actors)
        self.n = GCounter(n_actors=n_actors)

    def inc(self, actor):
        return (self.p.inc(actor), True)

    def dec(self, actor):
        return (self.n.inc(actor), False)

    def apply(self, op):
        dot, pos = op
        (self.p if pos else self.n).apply(dot)

    def merge(self, other, engine=None):
        merge_batch([self], [other], engine)

    def value(self):
        def i64(x):
            x &= 0xFFFFFFFFFFFFFFFF
            return x - (1 << 64) if x >= (1 << 63) else x

        return i64(i64(self.p.value()) - i64(self.n.value()))

    def row(self, n):
        return np.concatenate([self.p.row(n), self.n.row(n)])

    def set_row(self, r, n):
        self.p.set_row(r[:n], n)
        self.n.set_row(r[n:], n)

