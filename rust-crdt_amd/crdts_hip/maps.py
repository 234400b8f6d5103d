"""Engine's calls over the three Map slabs — Map<u64, MVReg>, Map<u64, Orswot>
and the nested Map<u64, Map<u64, MVReg>>: merge, apply, truncate and the value
of get (include/crdts_hip.h crdt_map_mvreg_*, crdt_map_orswot_*,
crdt_map_map_*)."""
from __future__ import annotations

import ctypes as C

from ._lib import check, lib
from ._util import _torch, dptr, on_stream, ptr
from .batches import OrswotBatch
from .ops import MapMapOps, MapOps, MapOrswotOps, ReadQueries
from .slabs import MapMapSlab, MapOrswotSlab, MapSlab


class MapEngine:
    """Engine's Map methods (mixed into crdts_hip.Engine)."""

    def _map_call(self, name, S, arg, out, n_actors, stream, check_status, scratch=None):
        """The shared shape of the Map merge / apply / truncate calls:
        crdt_<name>(ctx, S, arg, out, n, n_actors[, scratch, scratch_bytes],
        stream), `arg` the other slab or the op batch by reference, or the
        clock rows. `scratch` names the engine's scratch tensor of a nested-map
        call, sized by crdt_<name>_scratch_bytes for the output slab."""
        n = S.n
        s, r = S.cstruct(), out.cstruct()
        extra = ()
        if scratch is not None:
            nb = int(getattr(lib, f"crdt_{name}_scratch_bytes")(C.byref(r), n, n_actors))
            sc = self._scratch(scratch, nb, S.a["clock"].device)
            extra = (dptr(sc), int(sc.numel()))
        self._done(getattr(lib, f"crdt_{name}")(self.ctx, C.byref(s), arg, C.byref(r), n, n_actors, *extra,
                                                self._stream(stream)), name, stream, check_status)
        return out

    # ------------------------------------------------ Map::merge
    def map_mvreg_merge(self, S: "MapSlab", O: "MapSlab", n_actors, stream=None, check_status=True, out=None):
        """Map::merge (src/map.rs:191-268) of device slabs; returns the output slab
        (capacities = the sums of the inputs'). Only the used slots of the
        output are written (`out`, if given, is reused as it is)."""
        if out is None:
            out = MapSlab.alloc(S.n, n_actors, S.kcap + O.kcap, S.mcap + O.mcap, S.dcap + O.dcap, S.scap + O.scap,
                                device=S.a["clock"].device)
        o = O.cstruct()
        return self._map_call("map_mvreg_merge", S, C.byref(o), out, n_actors, stream, check_status)

    def map_map_merge(self, S: "MapMapSlab", O: "MapMapSlab", n_actors, stream=None, check_status=True, out=None):
        """Map::merge of nested maps (src/map.rs:191-268 with the inner map as
        the value: its merge and Causal::truncate) of device slabs; returns
        the output slab (capacities: the sums of the inputs', outer and inner)."""
        if out is None:
            out = MapMapSlab.alloc(S.n, n_actors, S.kcap + O.kcap, S.dcap + O.dcap, S.scap + O.scap,
                                   tuple(x + y for x, y in zip(S.inner_caps, O.inner_caps)),
                                   device=S.a["clock"].device)
        o = O.cstruct()
        return self._map_call("map_map_merge", S, C.byref(o), out, n_actors, stream, check_status,
                              scratch="_map_map_scratch")

    def map_orswot_merge(self, S: "MapOrswotSlab", O: "MapOrswotSlab", n_actors, out_caps=None, stream=None,
                         check_status=True, out=None):
        """Map::merge with Orswot values (src/map.rs:192-269) of device slabs;
        returns the output slab (default capacities: the sums of the inputs').
        Only the used slots of the output are written (`out`, if given, is
        reused as it is: compare `.canonical()` forms)."""
        caps = out_caps or {k: S.caps[k] + O.caps[k] for k in S.caps}
        if out is None:
            out = MapOrswotSlab.alloc(S.n, n_actors, device=S.a["clock"].device, **caps)
        o = O.cstruct()
        return self._map_call("map_orswot_merge", S, C.byref(o), out, n_actors, stream, check_status)

    # ------------------------------------------------ Map::apply
    def map_mvreg_apply(self, S: "MapSlab", ops: "MapOps", n_actors, out_caps=None, out=None, stream=None,
                        check_status=True):
        """out[i] = S[i] after Map::apply (src/map.rs:160-190) of object i's ops
        in order; returns the output slab (`out`, or a new one of capacities
        out_caps = (kcap, mcap, dcap, scap), default: S's plus one key, value
        and deferred clock per op of the longest op list, within the call's
        limits). Only the used slots of the output are written. Not in place."""
        if out is None:
            if out_caps is None:
                grow = ops.longest()
                out_caps = (min(8192, S.kcap + grow), min(256, S.mcap + grow), min(128, S.dcap + grow),
                            min(8192, S.scap + grow))
            out = MapSlab.alloc(S.n, n_actors, *out_caps, device=S.a["clock"].device)
        o = ops.cops()
        return self._map_call("map_mvreg_apply", S, C.byref(o), out, n_actors, stream, check_status)

    MAP_MAP_APPLY_CAP_MAX = ((8192, 128, 8192), (8192, 256, 128, 8192))  # outer (k, d, s), inner (k, m, d, s)

    def map_map_apply(self, S: "MapMapSlab", ops: "MapMapOps", n_actors, out_caps=None, inner_out_caps=None,
                      out=None, stream=None, check_status=True):
        """out[i] = S[i] after Map::apply (src/map.rs:160-190, the inner op by
        the same apply on the inner map) of object i's ops in order; returns
        the output slab (`out`, or a new one of capacities out_caps = (kcap,
        dcap, scap) and inner_out_caps = (kcap, mcap, dcap, scap), default:
        S's plus one slot per op of the longest op list, within the call's
        limits). Only the used slots of the output are written. Not in place."""
        if out is None:
            if out_caps is None or inner_out_caps is None:
                grow = ops.longest()
                mo, mi = self.MAP_MAP_APPLY_CAP_MAX
                if out_caps is None:
                    out_caps = tuple(min(m, c + grow) for m, c in zip(mo, (S.kcap, S.dcap, S.scap)))
                if inner_out_caps is None:
                    inner_out_caps = tuple(min(m, c + grow) for m, c in zip(mi, S.inner_caps))
            out = MapMapSlab.alloc(S.n, n_actors, *out_caps, tuple(inner_out_caps), device=S.a["clock"].device)
        o = ops.cops()
        return self._map_call("map_map_apply", S, C.byref(o), out, n_actors, stream, check_status,
                              scratch="_map_map_apply_scratch")

    MAP_ORSWOT_APPLY_CAP_MAX = {"kcap": 8192, "mcap": 512, "vdcap": 512, "vscap": 512, "dcap": 512, "scap": 8192}

    def map_orswot_apply(self, S: "MapOrswotSlab", ops: "MapOrswotOps", n_actors, out_caps=None, out=None,
                         stream=None, check_status=True):
        """out[i] = S[i] after Map::apply (src/map.rs:160-190) of object i's ops
        in order; returns the output slab (`out`, or a new one of capacities
        out_caps = dict(kcap, mcap, vdcap, vscap, dcap, scap), default: S's plus
        one slot per op of the longest op list, within the call's limits). Only
        the used slots of the output are written. Not in place."""
        if out is None:
            if out_caps is None:
                grow = ops.longest()
                out_caps = {k: min(self.MAP_ORSWOT_APPLY_CAP_MAX[k], S.caps[k] + grow) for k in S.caps}
            out = MapOrswotSlab.alloc(S.n, n_actors, device=S.a["clock"].device, **out_caps)
        o = ops.cops()
        return self._map_call("map_orswot_apply", S, C.byref(o), out, n_actors, stream, check_status)

    # ------------------------------------------------ Map::truncate
    def map_mvreg_truncate(self, S: "MapSlab", clock_rows, n_actors, out_caps=None, out=None, stream=None,
                           check_status=True):
        """out[i] = S[i] after Map::truncate (src/map.rs:131-158) by the dense
        clock row clock_rows[i] (int64 device tensor [n][n_actors], 0 = absent);
        returns the output slab (`out`, or a new one of capacities out_caps =
        (kcap, mcap, dcap, scap), default: S's). Only the used slots of the
        output are written. Not in place."""
        if out is None:
            out = MapSlab.alloc(S.n, n_actors, *(out_caps or (S.kcap, S.mcap, S.dcap, S.scap)),
                                device=S.a["clock"].device)
        return self._map_call("map_mvreg_truncate", S, C.c_void_p(clock_rows.data_ptr()), out, n_actors, stream,
                              check_status)

    def map_orswot_truncate(self, S: "MapOrswotSlab", clock_rows, n_actors, out_caps=None, out=None, stream=None,
                            check_status=True):
        """out[i] = S[i] after Map::truncate (src/map.rs:131-158, the sets by
        Orswot::truncate, src/orswot.rs:159-172) by clock_rows[i]; returns the
        output slab (`out`, or a new one of capacities out_caps = dict(kcap,
        mcap, vdcap, vscap, dcap, scap), default: S's). Only the used slots of
        the output are written. Not in place."""
        if out is None:
            out = MapOrswotSlab.alloc(S.n, n_actors, device=S.a["clock"].device, **(out_caps or S.caps))
        return self._map_call("map_orswot_truncate", S, C.c_void_p(clock_rows.data_ptr()), out, n_actors, stream,
                              check_status)

    def map_map_truncate(self, S: "MapMapSlab", clock_rows, n_actors, out_caps=None, inner_out_caps=None, out=None,
                         stream=None, check_status=True):
        """out[i] = S[i] after Map::truncate (src/map.rs:131-158, the inner maps
        by the same truncate) by clock_rows[i]; returns the output slab (`out`,
        or a new one of capacities out_caps = (kcap, dcap, scap) and
        inner_out_caps = (kcap, mcap, dcap, scap), default: S's). Only the
        used slots of the output are written. Not in place."""
        if out is None:
            out = MapMapSlab.alloc(S.n, n_actors, *(out_caps or (S.kcap, S.dcap, S.scap)),
                                   tuple(inner_out_caps or S.inner_caps), device=S.a["clock"].device)
        return self._map_call("map_map_truncate", S, C.c_void_p(clock_rows.data_ptr()), out, n_actors, stream,
                              check_status, scratch="_map_map_truncate_scratch")

    # ------------------------------------------------ the value of Map::get
    def map_mvreg_get(self, S: "MapSlab", queries: "ReadQueries", n_actors, out_cap=None, out=None, stream=None,
                      check_status=True):
        """The value of Map::get (src/map.rs:291-302) for Map<u64, MVReg>: query
        j's register as row j of an MVReg slab (n, clocks [n_q][cap][A], vals
        [n_q][cap]), unused slots zero-filled; n = 0 for an absent key."""
        cap = int(out[2].shape[1]) if out is not None else int(out_cap or S.mcap)
        outn, outc, outv = self._mvreg_out(queries.n_q, cap, n_actors, S.a["clock"].device, out)
        s, q = S.cstruct(), queries.cqueries()
        self._done(lib.crdt_map_mvreg_get(self.ctx, C.byref(s), C.byref(q), S.n, n_actors, ptr(outn), ptr(outc),
                                          ptr(outv), cap, self._stream(stream)), "map_mvreg_get", stream, check_status)
        return outn, outc, outv

    def map_orswot_get(self, S: "MapOrswotSlab", queries: "ReadQueries", n_actors, stream=None, check_status=True):
        """The value of Map::get (src/map.rs:291-302) for Map<u64, Orswot>: query
        j's set as record j of an OrswotBatch (dense top clocks), packed back to
        back: the sizes call, an exclusive scan, the write call. Returns (batch,
        present): present[j] = 1 where the record is the key's value; an absent
        key and an ALL query give Orswot::default()."""
        torch = _torch()
        dev = S.a["n_keys"].device
        n_q, n = queries.n_q, S.n
        st = self._stream(stream)
        s, q = S.cstruct(), queries.cqueries()
        sizes = torch.zeros(n_q, dtype=torch.int64, device=dev)
        present = torch.zeros(n_q, dtype=torch.int32, device=dev)
        check(lib.crdt_map_orswot_get_sizes(self.ctx, C.byref(s), C.byref(q), n, n_actors, ptr(sizes), ptr(present),
                                            st), "map_orswot_get_sizes")
        with on_stream(stream):
            ends = torch.cumsum(sizes, 0)
            total = int(ends[-1].item()) if n_q else 0
            off = ends - sizes
        base = torch.empty(max(16, total), dtype=torch.uint8, device=dev)
        self._done(lib.crdt_map_orswot_get(self.ctx, C.byref(s), C.byref(q), n, n_actors, ptr(base), ptr(off),
                                           int(base.numel()), st), "map_orswot_get", stream, check_status)
        return OrswotBatch(base, off, n_actors, int(base.numel()), 0), present

    def map_map_get(self, S: "MapMapSlab", queries: "ReadQueries", n_actors, out=None, stream=None,
                    check_status=True):
        """The value of Map::get for the nested map: query j's inner map as row j
        of a MapSlab (allocated at S.inner's capacities when out is None), ready
        for map_mvreg_merge / _apply / _truncate / _to_bincode and map_read.
        Returns (slab, present); an absent key and an ALL query give the empty
        map."""
        torch = _torch()
        dev = S.a["n_keys"].device
        n_q = queries.n_q
        if out is None:
            out = MapSlab.alloc(n_q, n_actors, *S.inner_caps, device=dev)
        present = torch.zeros(n_q, dtype=torch.int32, device=dev)
        s, q, o = S.cstruct(), queries.cqueries(), out.cstruct()
        self._done(lib.crdt_map_map_get(self.ctx, C.byref(s), C.byref(q), S.n, n_actors, C.byref(o), ptr(present),
                                        self._stream(stream)), "map_map_get", stream, check_status)
        return out, present
