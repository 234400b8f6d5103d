"""bincode codec of the states: Engine's from_bincode / to_bincode calls for
Orswot records, MVReg slabs and the three Map slabs — the reference's
`to_binary` / `from_binary` (src/lib.rs:62-83) on the device
(include/crdts_hip.h crdt_*_from_bincode, crdt_*_bincode_sizes,
crdt_*_to_bincode).

Blobs are uint8 device tensors; offsets, lengths and sizes int64 tensors
holding u64 values."""
from __future__ import annotations

import ctypes as C

from ._lib import CrdtError, check, lib
from ._util import _torch, dptr, on_stream
from .batches import OrswotBatch
from .slabs import MapMapSlab, MapOrswotSlab, MapSlab


class StateBincodeEngine:
    """Engine's state codec methods (mixed into crdts_hip.Engine)."""

    def _placed(self, lens, stream):
        """Exclusive scan of blob sizes -> (buffer, offsets): blobs packed back to back."""
        torch = _torch()
        n = int(lens.numel())
        with on_stream(stream):
            ends = torch.cumsum(lens, 0)
            total = int(ends[-1].item()) if n else 0
            off = ends - lens
        return torch.empty(max(32, total), dtype=torch.uint8, device=lens.device), off

    def _egest(self, name, lead, n, dev, stream, check_status):
        """The egest protocol — sizes, exclusive scan, write — of the codecs
        whose two calls share their leading arguments `lead`:
        crdt_<name>_bincode_sizes(ctx, *lead, lens, stream), then
        crdt_<name>_to_bincode(ctx, *lead, out, off, out_bytes, stream).
        Returns (blobs uint8, blob_off int64, blob_len int64), n blobs packed
        back to back."""
        st = self._stream(stream)
        lens = _torch().empty(n, dtype=_torch().int64, device=dev)
        check(getattr(lib, f"crdt_{name}_bincode_sizes")(self.ctx, *lead, dptr(lens), st), f"{name}_bincode_sizes")
        out, off = self._placed(lens, stream)
        self._done(getattr(lib, f"crdt_{name}_to_bincode")(self.ctx, *lead, dptr(out), dptr(off), int(out.numel()), st),
                   f"{name}_to_bincode", stream, check_status)
        return out, off, lens

    def _nested_to_bincode(self, name, S, n_actors, widths, stream, check_status):
        """_egest of a Map slab: widths are the call's byte widths in its order."""
        s = S.cstruct()
        return self._egest(name, (C.byref(s), S.n, n_actors, *widths), S.n, S.a["clock"].device, stream, check_status)

    def _map_from_bincode(self, name, alloc, blobs, blob_off, blob_len, n_actors, widths, out_caps, out, stream,
                          check_status):
        """The ingest call of a Map slab, crdt_<name>_from_bincode(ctx, blobs,
        blob_bytes, blob_off, blob_len, n, *widths, n_actors, out, stream),
        into `out`, or into alloc(n) when out_caps is given."""
        n = int(blob_off.numel())
        if out is None:
            if out_caps is None:
                raise CrdtError(-1, f"{name}_from_bincode needs out or out_caps")
            out = alloc(n)
        r = out.cstruct()
        self._done(getattr(lib, f"crdt_{name}_from_bincode")(self.ctx, dptr(blobs), int(blobs.numel()), dptr(blob_off),
                                                             dptr(blob_len), n, *widths, n_actors, C.byref(r),
                                                             self._stream(stream)),
                   f"{name}_from_bincode", stream, check_status)
        return out

    # ---------------------------------------------------------------- Orswot
    def orswot_from_bincode(self, blobs, blob_off, blob_len, n_actors, actor_bytes, member_bytes, flags=0,
                            stream=None, check_status=True, packed=True):
        """Records from the reference's binary form (`from_binary`, src/lib.rs:78-83).

        blobs: torch.uint8 device tensor; blob_off / blob_len: torch.int64 device
        tensors (u64). Returns an OrswotBatch of canonical records: packed
        (a sizes pass walks every blob first), or with packed=False placed by
        crdt_orswot_bincode_record_bounds (blob lengths only: every blob is
        read once; the batch has gaps)."""
        torch = _torch()
        n = int(blob_off.numel())
        dev = f"cuda:{self.device}"
        st = self._stream(stream)
        sizes = torch.empty(n, dtype=torch.int64, device=dev)
        if packed:
            check(lib.crdt_orswot_bincode_record_sizes(self.ctx, dptr(blobs), int(blobs.numel()), dptr(blob_off),
                                                       dptr(blob_len), n, actor_bytes, member_bytes, n_actors, flags,
                                                       dptr(sizes), st), "bincode_record_sizes")
        else:
            check(lib.crdt_orswot_bincode_record_bounds(self.ctx, dptr(blob_len), n, actor_bytes, member_bytes,
                                                        n_actors, flags, dptr(sizes), st), "bincode_record_bounds")
        with on_stream(stream):
            ends = torch.cumsum(sizes, 0)
            total = int(ends[-1].item()) if n else 0
            off = ends - sizes
        base = torch.empty(max(16, total), dtype=torch.uint8, device=dev)
        self._done(lib.crdt_orswot_from_bincode(self.ctx, dptr(blobs), int(blobs.numel()), dptr(blob_off),
                                                dptr(blob_len), n, actor_bytes, member_bytes, n_actors, flags,
                                                dptr(base), dptr(off), int(base.numel()), st),
                   "from_bincode", stream, check_status)
        return OrswotBatch(base, off, n_actors, int(base.numel()), flags)

    def orswot_to_bincode(self, B: "OrswotBatch", actor_bytes, member_bytes, stream=None, check_status=True):
        """The reference's binary form (`to_binary`, src/lib.rs:62-64) of every
        record: (blobs uint8, blob_off int64, blob_len int64) device tensors;
        blob i starts 16-B aligned and is zero-padded to 16."""
        torch = _torch()
        dev = f"cuda:{self.device}"
        st = self._stream(stream)
        b = B.cbatch()
        lens = torch.empty(B.n_obj, dtype=torch.int64, device=dev)
        check(lib.crdt_orswot_bincode_sizes(self.ctx, C.byref(b), B.n_actors, B.flags, actor_bytes, member_bytes,
                                            dptr(lens), st), "bincode_sizes")
        with on_stream(stream):
            padded = (lens + 15) // 16 * 16
            ends = torch.cumsum(padded, 0)
            total = int(ends[-1].item()) if B.n_obj else 0
            off = ends - padded
        out = torch.empty(max(16, total), dtype=torch.uint8, device=dev)
        self._done(lib.crdt_orswot_to_bincode(self.ctx, C.byref(b), B.n_actors, B.flags, actor_bytes, member_bytes,
                                              dptr(out), dptr(off), int(out.numel()), st),
                   "to_bincode", stream, check_status)
        return out, off, lens

    # ----------------------------------------------------------------- MVReg
    def mvreg_from_bincode(self, blobs, blob_off, blob_len, n_actors, actor_bytes, val_bytes, out_cap=None, out=None,
                           stream=None, check_status=True):
        """MVReg slabs (n, clocks[n][cap][A], vals[n][cap], as mvreg_merge takes
        them) from `to_binary` blobs of MVReg<V, A> (src/mvreg.rs:42-46; src/lib.rs:
        62-83). blobs: torch.uint8 device tensor; blob_off / blob_len: torch.int64
        device tensors (u64). Returns `out`, or a new slab of out_cap slots
        (required without `out`); every unused slot is zero-filled."""
        n = int(blob_off.numel())
        if out is None and not out_cap:
            raise CrdtError(-1, "mvreg_from_bincode needs out or out_cap")
        cap = int(out[2].shape[1]) if out is not None else int(out_cap)
        outn, outc, outv = self._mvreg_out(n, cap, n_actors, blobs.device, out)
        self._done(lib.crdt_mvreg_from_bincode(self.ctx, dptr(blobs), int(blobs.numel()), dptr(blob_off), dptr(blob_len),
                                               n, actor_bytes, val_bytes, n_actors, dptr(outn), dptr(outc), dptr(outv),
                                               cap, self._stream(stream)), "mvreg_from_bincode", stream, check_status)
        return outn, outc, outv

    def mvreg_to_bincode(self, slab, n_actors, actor_bytes, val_bytes, stream=None, check_status=True):
        """`to_binary` (src/lib.rs:62-64) of every register of an MVReg slab:
        (blobs uint8, blob_off int64, blob_len int64) device tensors, the blobs
        packed back to back (sizes, exclusive scan, write)."""
        sn, sc, sv = slab
        n, cap = int(sn.numel()), int(sv.shape[1])
        return self._egest("mvreg", (dptr(sn), dptr(sc), dptr(sv), cap, n, n_actors, actor_bytes, val_bytes), n,
                           sn.device, stream, check_status)

    # ------------------------------------------------------- the three Maps
    def map_mvreg_from_bincode(self, blobs, blob_off, blob_len, n_actors, actor_bytes, key_bytes, val_bytes,
                               out_caps=None, out=None, stream=None, check_status=True):
        """A MapSlab from `to_binary` blobs of Map<K, MVReg<V, A>, A> (src/map.rs:
        81-99), in the slab's canonical form (deferred clocks in CLOCK ORDER).
        Returns `out`, or a new slab of capacities out_caps = (kcap, mcap, dcap,
        scap) (required without `out`). Only the used slots are written."""
        return self._map_from_bincode(
            "map_mvreg", lambda n: MapSlab.alloc(n, n_actors, *out_caps, device=blobs.device), blobs, blob_off,
            blob_len, n_actors, (actor_bytes, key_bytes, val_bytes), out_caps, out, stream, check_status)

    def map_mvreg_to_bincode(self, S: "MapSlab", n_actors, actor_bytes, key_bytes, val_bytes, stream=None,
                             check_status=True):
        """`to_binary` of every map of a MapSlab, the deferred clocks in the
        slab's CLOCK ORDER: (blobs uint8, blob_off int64, blob_len int64) device
        tensors, the blobs packed back to back (sizes, exclusive scan, write)."""
        return self._nested_to_bincode("map_mvreg", S, n_actors, (actor_bytes, key_bytes, val_bytes), stream,
                                       check_status)

    def map_orswot_from_bincode(self, blobs, blob_off, blob_len, n_actors, actor_bytes, key_bytes, member_bytes,
                                out_caps=None, out=None, stream=None, check_status=True):
        """A MapOrswotSlab from `to_binary` blobs of Map<K, Orswot<M, A>, A>, in
        the slab's canonical form: members and deferred member sets sorted
        ascending, nested and map deferred clocks in CLOCK ORDER. Returns `out`,
        or a new slab of capacities out_caps = dict(kcap, mcap, vdcap, vscap,
        dcap, scap) (required without `out`). Only the used slots are written."""
        return self._map_from_bincode(
            "map_orswot", lambda n: MapOrswotSlab.alloc(n, n_actors, device=blobs.device, **out_caps), blobs,
            blob_off, blob_len, n_actors, (actor_bytes, key_bytes, member_bytes), out_caps, out, stream, check_status)

    def map_orswot_to_bincode(self, S: "MapOrswotSlab", n_actors, actor_bytes, key_bytes, member_bytes, stream=None,
                              check_status=True):
        """`to_binary` of every map of a MapOrswotSlab, every unordered
        container in the slab's order: (blobs uint8, blob_off int64, blob_len
        int64) device tensors, the blobs packed back to back (sizes, exclusive
        scan, write)."""
        return self._nested_to_bincode("map_orswot", S, n_actors, (actor_bytes, key_bytes, member_bytes), stream,
                                       check_status)

    def map_map_from_bincode(self, blobs, blob_off, blob_len, n_actors, actor_bytes, key_bytes, inner_key_bytes,
                             val_bytes, out_caps=None, out=None, stream=None, check_status=True):
        """A MapMapSlab from `to_binary` blobs of Map<K, Map<K2, MVReg<V, A>, A>,
        A> (the reference's TestMap), outer and inner deferred clocks in CLOCK
        ORDER. Returns `out`, or a new slab of capacities out_caps = (kcap, dcap,
        scap, inner_caps) with inner_caps = (kcap, mcap, dcap, scap) (required
        without `out`). Only the used slots are written."""
        return self._map_from_bincode(
            "map_map", lambda n: MapMapSlab.alloc(n, n_actors, *out_caps, device=blobs.device), blobs, blob_off,
            blob_len, n_actors, (actor_bytes, key_bytes, inner_key_bytes, val_bytes), out_caps, out, stream,
            check_status)

    def map_map_to_bincode(self, S: "MapMapSlab", n_actors, actor_bytes, key_bytes, inner_key_bytes, val_bytes,
                           stream=None, check_status=True):
        """`to_binary` of every map of a MapMapSlab, deferred clocks in the
        slab's CLOCK ORDER: (blobs uint8, blob_off int64, blob_len int64) device
        tensors, the blobs packed back to back (sizes, exclusive scan, write)."""
        return self._nested_to_bincode("map_map", S, n_actors, (actor_bytes, key_bytes, inner_key_bytes, val_bytes),
                                       stream, check_status)
