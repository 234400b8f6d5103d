"""The dense fixed-capacity slabs of the three Map types (crdt_map_mvreg_slab,
crdt_map_map_slab, crdt_map_orswot_slab). Each class names its struct's
layout (_lib.SlabLayout); shapes, dtypes, host <-> device moves, the C struct
and the used-slot bookkeeping come from the layout."""
from __future__ import annotations

import numpy as np

from ._lib import MAP_MAP_SLAB, MAP_MVREG_SLAB, MAP_ORSWOT_SLAB, MapReadViewC
from ._util import _torch, dptr


def _read_view(a, kcap):
    """crdt_map_read_view of a Map slab's arrays (device tensors)."""
    return MapReadViewC(*[dptr(a[f]) for f, _ in MapReadViewC._fields_[:4]], kcap)


class Slab:
    """A batch of states in one layout: `a`, {member: array} — numpy (host) or
    torch (device), dtypes u32 / u64 (torch: int32 / int64) — and `caps`,
    {capacity: slots}. Only the used slots of a slab mean anything: the
    kernels write no others (include/crdts_hip.h)."""

    LAYOUT = None  # the struct's _lib.SlabLayout

    def _like(self, arrays):
        """A slab of this one's class and capacities over other arrays."""
        raise NotImplementedError

    @property
    def n(self):
        return int(self.a["n_keys"].shape[0])

    @classmethod
    def _shapes(cls, n, A, caps):
        return {f: (n,) + tuple(A if cap == "A" else caps[cap] for cap, _ in ax) for f, ax in cls.LAYOUT.axes.items()}

    @classmethod
    def _zeros(cls, shapes, device):
        out = {}
        for f, shp in shapes.items():
            u32 = f in cls.LAYOUT.u32
            if device is None:
                out[f] = np.zeros(shp, np.uint32 if u32 else np.uint64)
            else:
                torch = _torch()
                out[f] = torch.zeros(shp, dtype=torch.int32 if u32 else torch.int64, device=device)
        return out

    def to(self, device):
        torch = _torch()
        return self._like({f: torch.from_numpy(np.ascontiguousarray(v).view(np.int32 if v.dtype == np.uint32
                                                                            else np.int64)).to(device)
                           for f, v in self.a.items()})

    def host(self):
        return self._like({f: (v.cpu().numpy().view(np.uint32 if v.dtype.itemsize == 4 else np.uint64)
                               if hasattr(v, "cpu") else v) for f, v in self.a.items()})

    def used_masks(self):
        """Per member, a boolean array of its shape: the slots the state uses.
        A slot is used iff, on every counted axis of the member, its index is
        below the count of the slot that holds it (keys below n_keys, a key's
        values below its count, deferred clocks below n_def, set elements
        below their set's size); the actor axis is always used. Host slabs."""
        a = self.host().a
        out = {}
        for f, axes in self.LAYOUT.axes.items():
            m = np.ones(a[f].shape[:1], bool)
            for cap, count in axes:
                m = m[..., None] if count is None else m[..., None] & (np.arange(self.caps[cap]) < a[count][..., None])
            out[f] = np.broadcast_to(m, a[f].shape)
        return out

    def canonical(self):
        """Host copy with every slot past its count zeroed: the kernels write
        only the used slots (include/crdts_hip.h), so two slabs hold the same
        states iff their canonical forms are equal."""
        h = self.host()
        a = {f: np.array(v, copy=True) for f, v in h.a.items()}
        for f, m in h.used_masks().items():
            a[f][~m] = 0
        return h._like(a)

    def used_bytes(self):
        """Bytes of the used slots (the state's own bytes, not its capacity)."""
        h = self.host()
        return int(sum(int(m.sum()) * h.a[f].dtype.itemsize for f, m in h.used_masks().items()))

    def cstruct(self):
        lay = self.LAYOUT
        p = [v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data for v in (self.a[f] for f in lay.fields)]
        return lay.ctype(*p, *[self.caps[c] for c in lay.caps])

    def read_view(self):
        """crdt_map_read_view: the map's own clock, keys and entry clocks."""
        return _read_view(self.a, self.caps["kcap"])


class MapSlab(Slab):
    """Dense fixed-capacity slab of Map<u64, MVReg<u64, A>, A> states
    (crdt_map_mvreg_slab, include/crdts_hip.h). Arrays are numpy (host) or
    torch (device) with the shapes below; dtypes u32 / u64 (torch: int32 / int64)."""

    LAYOUT = MAP_MVREG_SLAB
    FIELDS = LAYOUT.fields

    def __init__(self, arrays, kcap, mcap, dcap, scap):
        self.a = dict(arrays)
        self.kcap, self.mcap, self.dcap, self.scap = kcap, mcap, dcap, scap

    @property
    def caps(self):
        return {"kcap": self.kcap, "mcap": self.mcap, "dcap": self.dcap, "scap": self.scap}

    def _like(self, arrays):
        return MapSlab(arrays, self.kcap, self.mcap, self.dcap, self.scap)

    @staticmethod
    def shapes(n, A, kcap, mcap, dcap, scap):
        return MapSlab._shapes(n, A, dict(kcap=kcap, mcap=mcap, dcap=dcap, scap=scap))

    @classmethod
    def alloc(cls, n, A, kcap, mcap, dcap, scap, device=None):
        return cls(cls._zeros(cls.shapes(n, A, kcap, mcap, dcap, scap), device), kcap, mcap, dcap, scap)


class MapMapSlab(Slab):
    """Dense slab of Map<u64, Map<u64, MVReg<u64, A>, A>, A> states — the
    reference's TestMap (crdt_map_map_slab, include/crdts_hip.h): the outer
    map's arrays (shapes below) and `inner`, a MapSlab of n * kcap nested
    maps (key slot k of object i: inner object i * kcap + k)."""

    LAYOUT = MAP_MAP_SLAB
    FIELDS = LAYOUT.fields

    def __init__(self, arrays, kcap, dcap, scap, inner):
        self.a = dict(arrays)
        self.kcap, self.dcap, self.scap = kcap, dcap, scap
        self.inner = inner

    @property
    def caps(self):
        return {"kcap": self.kcap, "dcap": self.dcap, "scap": self.scap}

    @property
    def inner_caps(self):
        return (self.inner.kcap, self.inner.mcap, self.inner.dcap, self.inner.scap)

    def _like(self, arrays, inner=None):
        return MapMapSlab(arrays, self.kcap, self.dcap, self.scap, inner or self.inner)

    @staticmethod
    def shapes(n, A, kcap, dcap, scap):
        return MapMapSlab._shapes(n, A, dict(kcap=kcap, dcap=dcap, scap=scap))

    @classmethod
    def alloc(cls, n, A, kcap, dcap, scap, inner_caps, device=None):
        """inner_caps: (kcap, mcap, dcap, scap) of the nested maps."""
        return cls(cls._zeros(cls.shapes(n, A, kcap, dcap, scap), device), kcap, dcap, scap,
                   MapSlab.alloc(n * kcap, A, *inner_caps, device=device))

    def to(self, device):
        return self._like(super().to(device).a, self.inner.to(device))

    def host(self):
        return self._like(super().host().a, self.inner.host())

    def _used_keys(self):
        """Per nested map (inner object), whether its key slot is used. Host slabs."""
        return self.used_masks()["keys"].reshape(-1)

    def canonical(self):
        """Host copy with every slot past its count zeroed, outer and inner
        (nested maps of unused key slots zeroed whole)."""
        out = super().canonical()
        out.inner = out.inner.canonical()
        dead = ~out._used_keys()
        for v in out.inner.a.values():
            v[dead] = 0
        return out

    def used_bytes(self):
        """Bytes of the used slots: the outer map's, and the nested maps' of
        its used key slots (the state's own bytes, not the capacity)."""
        h = self.host()
        used = h._used_keys()
        inner = int(sum(int((m.reshape(m.shape[0], -1)[used]).sum()) * h.inner.a[f].dtype.itemsize
                        for f, m in h.inner.used_masks().items()))
        return super(MapMapSlab, h).used_bytes() + inner

    def cstruct(self):
        c = super().cstruct()
        c.inner = self.inner.cstruct()
        return c

    def read_view(self):
        """The outer map's view; the nested maps are read through inner.read_view()."""
        return super().read_view()


class MapOrswotSlab(Slab):
    """Dense fixed-capacity slab of Map<u64, Orswot<u64, A>, A> states
    (crdt_map_orswot_slab, include/crdts_hip.h): numpy (host) or torch
    (device) arrays with the shapes below; dtypes u32 / u64 (torch: int32 /
    int64). `caps` = dict(kcap, mcap, vdcap, vscap, dcap, scap)."""

    LAYOUT = MAP_ORSWOT_SLAB
    U32 = LAYOUT.u32

    def __init__(self, arrays, caps):
        self.a = dict(arrays)
        self.caps = dict(caps)

    def _like(self, arrays):
        return MapOrswotSlab(arrays, self.caps)

    @staticmethod
    def shapes(n, A, kcap, mcap, vdcap, vscap, dcap, scap):
        return MapOrswotSlab._shapes(n, A, dict(kcap=kcap, mcap=mcap, vdcap=vdcap, vscap=vscap, dcap=dcap, scap=scap))

    @classmethod
    def alloc(cls, n, A, device=None, **caps):
        return cls(cls._zeros(cls.shapes(n, A, **caps), device), caps)
