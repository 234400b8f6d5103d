"""Engine's Orswot calls over packed record batches: merge, fold, validate,
compact, and the op path's apply and truncate (include/crdts_hip.h
crdt_orswot_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SPARSE_CLOCK, Batch, CrdtError, check, lib
from ._util import _torch, dptr
from .batches import ClockBatch, OrswotBatch
from .ops import OrswotOps


class OrswotEngine:
    """Engine's Orswot methods (mixed into crdts_hip.Engine)."""

    def orswot_alloc_out(self, L: OrswotBatch, R: OrswotBatch):
        torch = _torch()
        nb = L.bytes + R.bytes
        base = torch.empty(nb, dtype=torch.uint8, device=f"cuda:{self.device}")
        off = torch.empty(L.n_obj, dtype=torch.int64, device=f"cuda:{self.device}")
        return OrswotBatch(base, off, L.n_actors, nb, L.flags)

    def orswot_merge(self, L: OrswotBatch, R: OrswotBatch, out: OrswotBatch | None = None, stream=None,
                     check_status=True):
        """out[i] = L[i].merge(&R[i])  (src/orswot.rs:87-157). Async unless check_status."""
        if L.n_actors != R.n_actors or L.n_obj != R.n_obj or L.flags != R.flags:
            raise CrdtError(-1, "batch shapes differ")
        if out is None:
            out = self.orswot_alloc_out(L, R)
        lb, rb = L.cbatch(), R.cbatch()
        out.flags = L.flags
        self._done(lib.crdt_orswot_merge_ex(self.ctx, C.byref(lb), C.byref(rb), dptr(out.base), dptr(out.off),
                                            out.bytes, L.n_actors, L.flags, self._stream(stream)),
                   "crdt_orswot_merge", stream, check_status)
        return out

    def orswot_fold(self, batches, out: OrswotBatch | None = None, stream=None, check_status=True):
        """((b0 ⊔ b1) ⊔ b2) ⊔ ... of batches of the same objects (crdt_orswot_fold:
        the rank-order fold of replica anti-entropy, R - 1 batched merges).
        Returns an OrswotBatch (`out`, reused, when given: at least the
        batches' bytes together and n_obj offsets)."""
        torch = _torch()
        B0 = batches[0]
        total = sum(B.bytes for B in batches)
        if out is None:
            out = OrswotBatch(torch.empty(max(16, total), dtype=torch.uint8, device=B0.base.device),
                              torch.empty(B0.n_obj, dtype=torch.int64, device=B0.base.device), B0.n_actors,
                              max(16, total), B0.flags)
        arr = (Batch * len(batches))(*[B.cbatch() for B in batches])
        self._done(lib.crdt_orswot_fold(self.ctx, arr, len(batches), B0.n_actors, B0.flags, dptr(out.base),
                                        dptr(out.off), out.bytes, self._stream(stream)),
                   "orswot_fold", stream, check_status)
        return out

    def orswot_validate(self, B: OrswotBatch, stream=None):
        b = B.cbatch()
        self._done(lib.crdt_orswot_validate_ex(self.ctx, C.byref(b), B.n_actors, B.flags, self._stream(stream)),
                   "validate", stream, True)

    def orswot_compact(self, B: OrswotBatch, stream=None):
        torch = _torch()
        dev = f"cuda:{self.device}"
        scratch = torch.empty(int(lib.crdt_orswot_compact_scratch_bytes(B.n_obj)), dtype=torch.uint8, device=dev)
        dst = torch.empty(B.bytes, dtype=torch.uint8, device=dev)
        doff = torch.empty(B.n_obj, dtype=torch.int64, device=dev)
        b = B.cbatch()
        check(lib.crdt_orswot_compact(self.ctx, C.byref(b), dptr(dst), dptr(doff), B.bytes, dptr(scratch),
                                      self._stream(stream)), "compact")
        torch.cuda.synchronize(self.device)
        used = 0
        if B.n_obj:
            last = int(doff[-1].item())
            used = last + int(dst[last:last + 4].cpu().numpy().view(np.uint32)[0])
        return OrswotBatch(dst, doff, B.n_actors, max(16, (used + 15) // 16 * 16), B.flags)

    def orswot_apply(self, B: "OrswotBatch", ops: "OrswotOps", stream=None, check_status=True):
        """out[i] = B[i] after CmRDT::apply of object i's ops in order
        (src/orswot.rs:61-85). Returns an OrswotBatch."""
        torch = _torch()
        dev = f"cuda:{self.device}"
        per_op = 48 if B.flags & SPARSE_CLOCK else 32  # include/crdts_hip.h: output reservation per op
        cap = B.bytes + per_op * ops.n_ops + 16 * ops.n_clk + 32 * B.n_obj
        base = torch.empty(max(16, cap), dtype=torch.uint8, device=dev)
        off = torch.empty(B.n_obj, dtype=torch.int64, device=dev)
        b = B.cbatch()
        o = ops.cops()
        self._done(lib.crdt_orswot_apply(self.ctx, C.byref(b), C.byref(o), B.n_actors, B.flags, dptr(base), dptr(off),
                                         int(base.numel()), self._stream(stream)),
                   "orswot_apply", stream, check_status)
        return OrswotBatch(base, off, B.n_actors, int(base.numel()), B.flags)

    def orswot_truncate(self, B: OrswotBatch, clocks: "ClockBatch", out: "OrswotBatch | None" = None, stream=None,
                        check_status=True):
        """out[i] = B[i] after Causal::truncate(&clocks[i]) (src/orswot.rs:159-172),
        written at B.off[i] (crdt_orswot_truncate). Returns an OrswotBatch
        (`out`, reused, when given: at least B.bytes bytes and B.n_obj offsets;
        it must not share memory with B's records — the call is not in place,
        CRDT_EINVAL)."""
        torch = _torch()
        dev = f"cuda:{self.device}"
        if out is not None:
            base, off = out.base, out.off
            if base.numel() < B.bytes or off.numel() < B.n_obj:
                raise ValueError("orswot_truncate: `out` is smaller than the input batch")
        else:
            base = torch.empty(max(16, B.bytes), dtype=torch.uint8, device=dev)
            off = torch.empty(B.n_obj, dtype=torch.int64, device=dev)
        b, c = B.cbatch(), clocks.cstruct()
        self._done(lib.crdt_orswot_truncate(self.ctx, C.byref(b), C.byref(c), B.n_actors, B.flags, dptr(base),
                                            dptr(off), base.numel(), self._stream(stream)),
                   "orswot_truncate", stream, check_status)
        return OrswotBatch(base, off, B.n_actors, base.numel(), B.flags)
