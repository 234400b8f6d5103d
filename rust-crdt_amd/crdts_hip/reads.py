"""Engine's batched read path: Orswot::contains / value, Map::get / len and
the contexts derived from them (include/crdts_hip.h crdt_orswot_read*,
crdt_map_read*)."""
from __future__ import annotations

import ctypes as C

from ._lib import CRDT_EINVAL, READ_SIZES_FIELDS, CrdtError, ReadOutC, ReadSizesC, check, lib
from ._util import _torch, on_stream
from .batches import OrswotBatch
from .ops import ReadQueries

READ_WANTS = ("val", "slot", "dot", "add", "rm", "list")


class ReadEngine:
    """Engine's read methods (mixed into crdts_hip.Engine)."""

    def _read(self, sizes_call, write_call, queries: "ReadQueries", want, stream, check_status):
        """The two-call protocol: sizes (zero-initialised), the inclusive prefix
        sums of the wanted groups' lengths on the device, write. Returns a
        dict of device tensors: val, slot, dot_ctr, and per wanted group g in
        add / rm: g_len, g_end, g_act, g_ctr; list: list_len, list_end, list_key."""
        torch = _torch()
        bad = set(want) - set(READ_WANTS)
        if bad:
            raise CrdtError(CRDT_EINVAL, f"read: unknown want {sorted(bad)}")
        dev = queries.t[0].device
        n_q = queries.n_q
        name = {"val": "val", "slot": "slot", "dot": "dot_ctr", "add": "add_len", "rm": "rm_len", "list": "list_len"}
        res = {name[w]: torch.zeros(n_q, dtype=torch.int64 if w in ("val", "dot") else torch.int32, device=dev)
               for w in READ_WANTS if w in want}
        q = queries.cqueries()
        z = ReadSizesC(*[C.c_void_p(res[f].data_ptr()) if f in res and n_q else None for f in READ_SIZES_FIELDS])
        st = self._stream(stream)
        check(sizes_call(C.byref(q), C.byref(z), st), "read_sizes")
        groups = [g for g in ("add", "rm", "list") if g in want]
        if groups:
            with on_stream(stream):
                for g in groups:
                    res[g + "_end"] = torch.cumsum(res[g + "_len"].to(torch.int64), 0)
                totals = {g: int(res[g + "_end"][-1].item()) if n_q else 0 for g in groups}
            o = ReadOutC()
            for g in groups:
                n = totals[g]
                setattr(o, "n_" + g, n)
                setattr(o, g + "_end", res[g + "_end"].data_ptr() if n_q else None)
                if g == "list":
                    res["list_key"] = torch.empty(n, dtype=torch.int64, device=dev)
                    o.list_key = res["list_key"].data_ptr() if n else None
                else:
                    res[g + "_act"] = torch.empty(n, dtype=torch.int32, device=dev)
                    res[g + "_ctr"] = torch.empty(n, dtype=torch.int64, device=dev)
                    setattr(o, g + "_act", res[g + "_act"].data_ptr() if n else None)
                    setattr(o, g + "_ctr", res[g + "_ctr"].data_ptr() if n else None)
            check(write_call(C.byref(q), C.byref(o), st), "read")
        if check_status:
            self.status(stream)
        return res

    def orswot_read(self, B: "OrswotBatch", queries: "ReadQueries", want=("val", "rm"), stream=None,
                    check_status=True):
        """Orswot::contains / value (src/orswot.rs:214-233) and the contexts
        derived from them (src/ctx.rs:45-60) for every query, on the device.
        want: any of val, slot, dot, add, rm, list — what is not wanted is
        not read. The rm / add groups are in the op-clock form of OrswotOps
        (clk_end / clk_act / clk_ctr), dot_ctr is the Add's counter."""
        b = B.cbatch()
        return self._read(
            lambda q, z, st: lib.crdt_orswot_read_sizes(self.ctx, C.byref(b), q, B.n_actors, B.flags, z, st),
            lambda q, o, st: lib.crdt_orswot_read(self.ctx, C.byref(b), q, B.n_actors, B.flags, o, st),
            queries, want, stream, check_status)

    def map_read(self, S, queries: "ReadQueries", n_actors, want=("val", "slot", "rm"), stream=None,
                 check_status=True):
        """Map::get / len (src/map.rs:282-302) and their contexts over the outer
        arrays of any of the three Map slabs (S.read_view()); `slot` is the
        key's index among the entries, the handle of the nested value."""
        v = S.read_view()
        n = int(S.a["n_keys"].shape[0])
        return self._read(
            lambda q, z, st: lib.crdt_map_read_sizes(self.ctx, C.byref(v), q, n, n_actors, z, st),
            lambda q, o, st: lib.crdt_map_read(self.ctx, C.byref(v), q, n, n_actors, o, st),
            queries, want, stream, check_status)
