"""Engine's MVReg<u64, A> calls over register slabs (n, clocks[n][cap][A],
vals[n][cap]): merge, the rank-order fold, and the op path's apply, truncate
and read clock (include/crdts_hip.h crdt_mvreg_*)."""
from __future__ import annotations

import ctypes as C

from ._lib import MVRegViewC, lib
from ._util import _torch, dptr
from .ops import MVRegOps


class MVRegEngine:
    """Engine's MVReg methods (mixed into crdts_hip.Engine)."""

    def _mvreg_out(self, n_obj, cap, n_actors, dev, out):
        torch = _torch()
        if out is not None:
            return out
        return (torch.empty(n_obj, dtype=torch.int32, device=dev),
                torch.empty((n_obj, cap, n_actors), dtype=torch.int64, device=dev),
                torch.empty((n_obj, cap), dtype=torch.int64, device=dev))

    def mvreg_merge(self, self_slab, other_slab, n_actors, out_cap=None, out=None, stream=None, check_status=True):
        """MVReg<u64, A>::merge (src/mvreg.rs:121-153) over slabs (n, clocks[n][cap][A], vals[n][cap])
        of int32 / int64 device tensors; returns the output slab (`out`, or a new
        one of out_cap slots, default: the two capacities' sum). Not in place."""
        sn, sc, sv = self_slab
        on, oc, ov = other_slab
        n_obj, scap, ocap = int(sn.numel()), int(sv.shape[1]), int(ov.shape[1])
        cap = int(out[2].shape[1]) if out is not None else (out_cap or scap + ocap)
        outn, outc, outv = self._mvreg_out(n_obj, cap, n_actors, sn.device, out)
        self._done(lib.crdt_mvreg_merge(self.ctx, dptr(sn), dptr(sc), dptr(sv), scap, dptr(on), dptr(oc), dptr(ov), ocap,
                                        dptr(outn), dptr(outc), dptr(outv), cap, n_obj, n_actors, self._stream(stream)),
                   "mvreg_merge", stream, check_status)
        return outn, outc, outv

    def mvreg_fold(self, reps, n_actors, out_cap=None, out=None, stream=None, check_status=True):
        """reps[0].merge(reps[1]).merge(reps[2])... in rank order, one launch
        (crdt_mvreg_fold): `reps` is a list of 1..32 slabs (n, clocks[n][cap][A],
        vals[n][cap]) as mvreg_merge takes them, capacities of their own (each
        <= 1024, 2048 in all); returns the output slab (`out`, or a new one of
        out_cap slots, default: the capacities' sum, 2048 at the most). Not in place."""
        p = lambda t: t.data_ptr() or None  # noqa: E731
        views = (MVRegViewC * max(1, len(reps)))(*[MVRegViewC(p(n), p(c), p(v), int(v.shape[1])) for n, c, v in reps])
        n_obj = int(reps[0][0].numel()) if reps else 0
        total = sum(int(v.shape[1]) for _, _, v in reps)
        cap = int(out[2].shape[1]) if out is not None else (out_cap or min(total, 2048))
        outn, outc, outv = self._mvreg_out(n_obj, cap, n_actors, reps[0][0].device if reps else None, out)
        self._done(lib.crdt_mvreg_fold(self.ctx, views, len(reps), dptr(outn), dptr(outc), dptr(outv), cap, n_obj,
                                       n_actors, self._stream(stream)), "mvreg_fold", stream, check_status)
        return outn, outc, outv

    def mvreg_apply(self, self_slab, ops: "MVRegOps", n_actors, out_cap=None, out=None, stream=None,
                    check_status=True):
        """out[i] = self[i] after MVReg::apply (src/mvreg.rs:158-186) of object i's
        Puts in order, over slabs as in mvreg_merge; returns the output slab
        (`out`, or a new one of out_cap slots, default: self's plus one per op
        of the longest op list, within the call's limit: ops.max_ops, recorded
        when the batch was packed from host arrays; for an MVRegOps built from
        device tensors without it, obj_end is copied to the host to find it,
        which synchronises — pass out or out_cap to avoid that). Not in place."""
        sn, sc, sv = self_slab
        n_obj, scap = int(sn.numel()), int(sv.shape[1])
        if out is not None:
            out_cap = int(out[2].shape[1])
        elif out_cap is None:
            out_cap = min(2048, scap + ops.longest())
        outn, outc, outv = self._mvreg_out(n_obj, out_cap, n_actors, sn.device, out)
        o = ops.cops()
        self._done(lib.crdt_mvreg_apply(self.ctx, dptr(sn), dptr(sc), dptr(sv), scap, C.byref(o), dptr(outn), dptr(outc),
                                        dptr(outv), out_cap, n_obj, n_actors, self._stream(stream)),
                   "mvreg_apply", stream, check_status)
        return outn, outc, outv

    def mvreg_truncate(self, self_slab, clock_rows, n_actors, out_cap=None, out=None, stream=None,
                       check_status=True):
        """Causal::truncate (src/mvreg.rs:100-113) of register i by the dense
        clock row clock_rows[i] (int64 device tensor [n][n_actors], 0 = absent);
        returns the output slab (out_cap defaults to self's). Not in place."""
        sn, sc, sv = self_slab
        n_obj, scap = int(sn.numel()), int(sv.shape[1])
        out_cap = int(out[2].shape[1]) if out is not None else (out_cap or scap)
        outn, outc, outv = self._mvreg_out(n_obj, out_cap, n_actors, sn.device, out)
        self._done(lib.crdt_mvreg_truncate(self.ctx, dptr(sn), dptr(sc), dptr(sv), scap, dptr(clock_rows), dptr(outn),
                                           dptr(outc), dptr(outv), out_cap, n_obj, n_actors, self._stream(stream)),
                   "mvreg_truncate", stream, check_status)
        return outn, outc, outv

    def mvreg_read_clock(self, slab, n_actors, out=None, stream=None, check_status=True):
        """read().add_clock (src/mvreg.rs:201-222) of every register: the
        pointwise max of its used clock rows, an int64 device tensor [n][n_actors]."""
        torch = _torch()
        sn, sc = slab[0], slab[1]
        n_obj, cap = int(sn.numel()), int(sc.shape[1])
        if out is None:
            out = torch.empty((n_obj, n_actors), dtype=torch.int64, device=sn.device)
        self._done(lib.crdt_mvreg_read_clock(self.ctx, dptr(sn), dptr(sc), cap, dptr(out), n_obj, n_actors,
                                             self._stream(stream)), "mvreg_read_clock", stream, check_status)
        return out
