"""Engine's VClock / GCounter / PNCounter calls over dense rows and sparse
(CSR) clock batches: merge, the order, and the clocks' op path
(include/crdts_hip.h crdt_vclock_*, crdt_gcounter_*, crdt_pncounter_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CrdtError, check, lib
from ._util import _torch, dptr
from .batches import ClockBatch
from .ops import ClockOps


class ClockEngine:
    """Engine's clock and counter methods (mixed into crdts_hip.Engine)."""

    # ------------------------------------------------ dense rows
    def dense_merge(self, self_rows, other_rows, n_actors, kind="gcounter", stream=None):
        """In place: self_rows = max(self_rows, other_rows) (src/vclock.rs:131-137).

        Rows are torch int64 device tensors holding u64 counters; shape
        [n_obj, n_actors] (vclock / gcounter) or [n_obj, 2*n_actors] (pncounter).
        """
        fn = {"vclock": lib.crdt_vclock_dense_merge, "gcounter": lib.crdt_gcounter_merge,
              "pncounter": lib.crdt_pncounter_merge}[kind]
        slots = n_actors * (2 if kind == "pncounter" else 1)
        if self_rows.numel() != other_rows.numel() or self_rows.numel() % slots:
            raise CrdtError(-1, "dense rows shape mismatch")
        n_obj = self_rows.numel() // slots
        check(fn(self.ctx, C.c_void_p(self_rows.data_ptr()), C.c_void_p(other_rows.data_ptr()), n_obj,
                 n_actors, self._stream(stream)), f"dense merge ({kind})")
        return self_rows

    def vclock_partial_cmp(self, a_rows, b_rows, n_actors, stream=None):
        """partial_cmp of dense rows (src/vclock.rs:59-71): int8 tensor of
        0 Equal, 1 Greater, -1 Less, 2 None."""
        torch = _torch()
        n = int(a_rows.numel()) // n_actors
        out = torch.empty(n, dtype=torch.int8, device=a_rows.device)
        check(lib.crdt_vclock_partial_cmp(self.ctx, dptr(a_rows), dptr(b_rows), n, n_actors, dptr(out),
                                          self._stream(stream)), "vclock_partial_cmp")
        return out

    def dense_apply(self, rows, ops: "ClockOps", n_actors, kind="vclock", stream=None, check_status=True):
        """In place: row i witnesses object i's dots (VClock::apply
        src/vclock.rs:126-128; GCounter::apply src/gcounter.rs:53-55;
        PNCounter::apply src/pncounter.rs:82-87 on [P|N] rows, ops with dir)."""
        fn = {"vclock": lib.crdt_vclock_dense_apply, "gcounter": lib.crdt_gcounter_apply,
              "pncounter": lib.crdt_pncounter_apply}[kind]
        slots = n_actors * (2 if kind == "pncounter" else 1)
        if rows.numel() != ops.n_obj * slots:
            raise CrdtError(-1, "dense rows shape mismatch")
        c = ops.cops()
        self._done(fn(self.ctx, dptr(rows), C.byref(c), ops.n_obj, n_actors, self._stream(stream)),
                   f"dense apply ({kind})", stream, check_status)
        return rows

    def _dense_binop(self, fn, what, self_rows, other_rows, n_actors, stream):
        if self_rows.numel() != other_rows.numel() or self_rows.numel() % n_actors:
            raise CrdtError(-1, "dense rows shape mismatch")
        check(fn(self.ctx, dptr(self_rows), dptr(other_rows), self_rows.numel() // n_actors, n_actors,
                 self._stream(stream)), what)
        return self_rows

    def dense_truncate(self, self_rows, other_rows, n_actors, stream=None):
        """In place: Causal::truncate (src/vclock.rs:103-120), the pointwise min."""
        return self._dense_binop(lib.crdt_vclock_dense_truncate, "dense truncate", self_rows, other_rows, n_actors,
                                 stream)

    def dense_subtract(self, self_rows, other_rows, n_actors, stream=None):
        """In place: VClock::subtract (src/vclock.rs:236-242)."""
        return self._dense_binop(lib.crdt_vclock_dense_subtract, "dense subtract", self_rows, other_rows, n_actors,
                                 stream)

    def dense_intersection(self, self_rows, other_rows, n_actors, stream=None):
        """In place: VClock::intersection (src/vclock.rs:219-228)."""
        return self._dense_binop(lib.crdt_vclock_dense_intersection, "dense intersection", self_rows, other_rows,
                                 n_actors, stream)

    def _dense_value(self, fn, what, rows, slots, n_actors, out, stream):
        torch = _torch()
        if rows.numel() % slots:
            raise CrdtError(-1, "dense rows shape mismatch")
        n_obj = rows.numel() // slots
        out = out if out is not None else torch.empty(n_obj, dtype=torch.int64, device=rows.device)
        check(fn(self.ctx, dptr(rows), dptr(out), n_obj, n_actors, self._stream(stream)), what)
        return out

    def gcounter_value(self, rows, n_actors, out=None, stream=None):
        """GCounter::value (src/gcounter.rs:76-78): int64 tensor holding the wrapping u64 row sums."""
        return self._dense_value(lib.crdt_gcounter_value, "gcounter value", rows, n_actors, n_actors, out, stream)

    def pncounter_value(self, rows, n_actors, out=None, stream=None):
        """PNCounter::value (src/pncounter.rs:117-119) of [P|N] rows: int64 per object."""
        return self._dense_value(lib.crdt_pncounter_value, "pncounter value", rows, 2 * n_actors, n_actors, out,
                                 stream)

    def dense_get(self, rows, queries: "ClockOps", n_actors, out=None, stream=None, check_status=True):
        """VClock::get (src/vclock.rs:206-210) per queried actor: int64 tensor
        [queries.n_ops] of u64 counters, 0 for an absent actor. VClock::inc
        (:182-185) is this + 1."""
        torch = _torch()
        if rows.numel() != queries.n_obj * n_actors:
            raise CrdtError(-1, "dense rows shape mismatch")
        out = out if out is not None else torch.empty(max(1, queries.n_ops), dtype=torch.int64, device=rows.device)
        c = queries.cops()
        self._done(lib.crdt_vclock_dense_get(self.ctx, dptr(rows), C.byref(c), dptr(out), queries.n_obj, n_actors,
                                             self._stream(stream)), "dense get", stream, check_status)
        return out[: queries.n_ops]

    # ------------------------------------------------ sparse (CSR) clocks
    def _csr_out(self, n_obj, cap):
        torch = _torch()
        dev = f"cuda:{self.device}"
        cap = max(1, cap)
        return ClockBatch(torch.empty(n_obj, dtype=torch.int64, device=dev),
                          torch.empty(n_obj, dtype=torch.int32, device=dev),
                          torch.empty(cap, dtype=torch.int32, device=dev),
                          torch.empty(cap, dtype=torch.int64, device=dev), n_entries=cap)

    def clock_csr_alloc_out(self, S: "ClockBatch", O: "ClockBatch"):
        return self._csr_out(S.n_obj, S.n_entries + O.n_entries)

    def _csr_filter(self, fn, what, S, O, out, stream, check_status):
        """The shared shape of the two-clock CSR calls: fn(ctx, S, O, out, stream)."""
        out = out or self._csr_out(S.n_obj, S.n_entries)
        s, o, w = S.cstruct(), O.cstruct(), out.cout()
        self._done(fn(self.ctx, C.byref(s), C.byref(o), C.byref(w), self._stream(stream)), what, stream, check_status)
        return out

    def clock_csr_merge(self, S: "ClockBatch", O: "ClockBatch", out: "ClockBatch | None" = None, kind="vclock",
                        stream=None, check_status=True):
        """out[i] = S[i].merge(&O[i]) over sparse clocks (VClock::merge
        src/vclock.rs:131-137; GCounter src/gcounter.rs:58-62): the sorted union,
        counters max'ed, placed at S.off + O.off (crdt_vclock_csr_merge)."""
        fn = {"vclock": lib.crdt_vclock_csr_merge, "gcounter": lib.crdt_gcounter_csr_merge}[kind]
        return self._csr_filter(fn, f"{kind}_csr_merge", S, O, out or self.clock_csr_alloc_out(S, O), stream,
                                check_status)

    def pncounter_csr_merge(self, SP, SN, OP, ON, outs=None, stream=None, check_status=True):
        """PNCounter::merge (src/pncounter.rs:90-95) over sparse P and N clocks
        (crdt_pncounter_csr_merge); returns (out_p, out_n)."""
        op, on = outs or (self.clock_csr_alloc_out(SP, OP), self.clock_csr_alloc_out(SN, ON))
        w = [x.cout() for x in (op, on)]
        c = [x.cstruct() for x in (SP, SN, OP, ON)]
        self._done(lib.crdt_pncounter_csr_merge(self.ctx, *[C.byref(x) for x in c], C.byref(w[0]), C.byref(w[1]),
                                                self._stream(stream)), "pncounter_csr_merge", stream, check_status)
        return op, on

    # ------------------------------------------------ the fold of R replicas
    def dense_fold(self, rows_list, n_slots, out=None, stream=None):
        """out = the pointwise max of 1..32 replicas' dense rows, one launch
        (crdt_clock_dense_fold): the chain rows_list[0].merge(rows_list[1])...
        of VClock / GCounter rows (n_slots = n_actors) or PNCounter [P|N] rows
        (n_slots = 2 * n_actors). `out` may be one of the replicas (in place);
        default: a new tensor."""
        torch = _torch()
        numel = int(rows_list[0].numel()) if rows_list else 0
        if any(int(r.numel()) != numel for r in rows_list) or (n_slots and numel % n_slots):
            raise CrdtError(-1, "dense rows shape mismatch")
        if out is None and rows_list:
            out = torch.empty_like(rows_list[0])
        if out is not None and int(out.numel()) != numel:
            raise CrdtError(-1, "dense rows shape mismatch")
        ptrs = (C.c_void_p * max(1, len(rows_list)))(*[r.data_ptr() or None for r in rows_list])
        check(lib.crdt_clock_dense_fold(self.ctx, ptrs, len(rows_list), dptr(out) if out is not None else None,
                                        numel // n_slots if n_slots else 0, n_slots, self._stream(stream)),
              "dense fold")
        return out

    def clock_csr_fold(self, reps, out: "ClockBatch | None" = None, stream=None, check_status=True):
        """out[i] = reps[0][i].merge(reps[1][i]).merge(reps[2][i])... over 1..32
        replicas' sparse clock batches, one launch (crdt_clock_csr_fold): the
        sorted union with the largest counter per actor, placed at the sum of
        the replicas' offsets; `out` defaults to a new batch of the summed
        n_entries. GCounter alike; PNCounter: pncounter_csr_fold."""
        from ._lib import ClockCsr

        n_obj = reps[0].n_obj if reps else 0
        out = out or self._csr_out(n_obj, sum(r.n_entries for r in reps))
        views = (ClockCsr * max(1, len(reps)))(*[r.cstruct() for r in reps])
        w = out.cout()
        self._done(lib.crdt_clock_csr_fold(self.ctx, views, len(reps), C.byref(w), self._stream(stream)),
                   "clock_csr_fold", stream, check_status)
        return out

    def pncounter_csr_fold(self, P_list, N_list, outs=None, stream=None, check_status=True):
        """PNCounter::merge (src/pncounter.rs:90-95) folded over R replicas'
        sparse P and N clocks: two folds; returns (out_p, out_n)."""
        op, on = outs or (None, None)
        return (self.clock_csr_fold(P_list, out=op, stream=stream, check_status=check_status),
                self.clock_csr_fold(N_list, out=on, stream=stream, check_status=check_status))

    def clock_csr_truncate(self, S: "ClockBatch", O: "ClockBatch", out=None, stream=None, check_status=True):
        """out[i] = S[i] after Causal::truncate(&O[i]) (src/vclock.rs:103-120), placed at S.off."""
        return self._csr_filter(lib.crdt_vclock_csr_truncate, "csr truncate", S, O, out, stream, check_status)

    def clock_csr_subtract(self, S: "ClockBatch", O: "ClockBatch", out=None, stream=None, check_status=True):
        """out[i] = S[i] after subtract(&O[i]) (src/vclock.rs:236-242), placed at S.off."""
        return self._csr_filter(lib.crdt_vclock_csr_subtract, "csr subtract", S, O, out, stream, check_status)

    def clock_csr_intersection(self, S: "ClockBatch", O: "ClockBatch", out=None, stream=None, check_status=True):
        """out[i] = S[i].intersection(&O[i]) (src/vclock.rs:219-228), placed at S.off."""
        return self._csr_filter(lib.crdt_vclock_csr_intersection, "csr intersection", S, O, out, stream,
                                check_status)

    def clock_csr_apply(self, S: "ClockBatch", ops: "ClockOps", out=None, kind="vclock", stream=None,
                        check_status=True):
        """out[i] = S[i] after witnessing object i's dots (VClock::apply
        src/vclock.rs:126-128; GCounter::apply src/gcounter.rs:53-55), placed
        at S.off[i] + (ops before i)."""
        if ops.n_obj != S.n_obj:
            raise CrdtError(-1, "clock_csr_apply: one op list per object")
        out = out or self._csr_out(S.n_obj, S.n_entries + ops.n_ops)
        s, c, w = S.cstruct(), ops.cops(), out.cout()
        fn = {"vclock": lib.crdt_vclock_csr_apply, "gcounter": lib.crdt_gcounter_csr_apply}[kind]
        self._done(fn(self.ctx, C.byref(s), C.byref(c), C.byref(w), self._stream(stream)), f"{kind}_csr_apply",
                   stream, check_status)
        return out

    def clock_csr_value(self, S: "ClockBatch", out=None, stream=None, check_status=True):
        """GCounter::value (src/gcounter.rs:76-78) of sparse counters: int64 tensor of wrapping u64 sums."""
        torch = _torch()
        out = out if out is not None else torch.empty(max(1, S.n_obj), dtype=torch.int64, device=S.off.device)
        s = S.cstruct()
        self._done(lib.crdt_gcounter_csr_value(self.ctx, C.byref(s), dptr(out), self._stream(stream)), "csr value",
                   stream, check_status)
        return out[: S.n_obj]

    def clock_csr_get(self, S: "ClockBatch", queries: "ClockOps", out=None, stream=None, check_status=True):
        """VClock::get (src/vclock.rs:206-210) per queried actor over sparse clocks."""
        torch = _torch()
        if queries.n_obj != S.n_obj:
            raise CrdtError(-1, "clock_csr_get: one query list per object")
        out = out if out is not None else torch.empty(max(1, queries.n_ops), dtype=torch.int64, device=S.off.device)
        s, c = S.cstruct(), queries.cops()
        self._done(lib.crdt_vclock_csr_get(self.ctx, C.byref(s), C.byref(c), dptr(out), self._stream(stream)),
                   "csr get", stream, check_status)
        return out[: queries.n_ops]

    def pncounter_csr_apply(self, SP: "ClockBatch", SN: "ClockBatch", ops: "ClockOps", stream=None,
                            check_status=True):
        """PNCounter::apply (src/pncounter.rs:82-87) over sparse P and N clocks:
        the ops are split by dir on the host and applied as two batches;
        returns (out_p, out_n)."""
        if ops.host is None or ops.host[3] is None:
            raise CrdtError(-1, "pncounter_csr_apply: ops packed from host arrays with dir")
        ends, act, ctr, dr = ops.host
        obj = np.repeat(np.arange(ends.size), np.diff(ends.astype(np.int64), prepend=0))
        outs = []
        for d, S in ((0, SP), (1, SN)):
            m = dr == d
            sub_ends = np.cumsum(np.bincount(obj[m], minlength=ends.size)).astype(np.uint64)
            sub = ClockOps.from_arrays(sub_ends, act[m], ctr[m], device=self.device)
            outs.append(self.clock_csr_apply(S, sub, kind="gcounter", stream=stream, check_status=check_status))
        return tuple(outs)

    def pncounter_csr_value(self, SP: "ClockBatch", SN: "ClockBatch", stream=None, check_status=True):
        """PNCounter::value (src/pncounter.rs:117-119) over sparse P and N clocks: int64 per object."""
        return (self.clock_csr_value(SP, stream=stream, check_status=check_status) -
                self.clock_csr_value(SN, stream=stream, check_status=check_status))
