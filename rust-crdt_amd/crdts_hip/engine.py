"""Engine: one crdt_ctx bound to a device. This module holds the context, the
stream and status plumbing and the diagnostic setters; the calls themselves
are mixins, one module per family."""
from __future__ import annotations

import ctypes as C

from ._lib import CrdtError, check, lib
from ._util import _torch
from .clock_bincode import ClockBincodeEngine
from .clocks import ClockEngine
from .lwwreg import LWWEngine
from .maps import MapEngine
from .mvreg import MVRegEngine
from .ops_bincode import OpsBincodeEngine
from .orswot import OrswotEngine
from .reads import ReadEngine
from .replica_engine import ReplicaEngine
from .state_bincode import StateBincodeEngine


class Engine(OrswotEngine, ClockEngine, MVRegEngine, MapEngine, ReadEngine, StateBincodeEngine, ReplicaEngine,
             LWWEngine, ClockBincodeEngine, OpsBincodeEngine):
    """One crdt_ctx bound to a device. All merges run on the GPU (the calls
    live with their family: orswot.py, clocks.py, mvreg.py, maps.py, reads.py,
    replica_engine.py, lwwreg.py, and the codecs in state_bincode.py,
    clock_bincode.py and ops_bincode.py)."""

    def __init__(self, device=0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise CrdtError(-6, "Engine needs a visible gfx950 GPU")
        self.device = int(device)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        check(lib.crdt_ctx_create(C.byref(ctx), self.device), "crdt_ctx_create")
        self.ctx = ctx

    def __del__(self):
        if getattr(self, "ctx", None) is not None and lib is not None:
            lib.crdt_ctx_destroy(self.ctx)
            self.ctx = None

    def _stream(self, stream=None):
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return C.c_void_p(s.cuda_stream)

    def status(self, stream=None):
        rc = lib.crdt_ctx_status(self.ctx, self._stream(stream))
        check(rc, "kernel status")

    def _done(self, rc, what, stream, check_status):
        """The tail of a call: its return code, then — unless the caller
        defers it (check_status=False: the call stays asynchronous) — the
        status the kernels latched."""
        check(rc, what)
        if check_status:
            self.status(stream)

    def _scratch(self, name, nbytes, dev):
        """The engine's grow-only scratch tensor `name`, at least nbytes on
        dev: kept on the engine, so a launch in flight on another stream never
        sees it freed."""
        sc = getattr(self, name, None)
        if sc is None or sc.numel() < nbytes or sc.device != dev:
            sc = _torch().empty(max(16, nbytes), dtype=_torch().uint8, device=dev)
            setattr(self, name, sc)
        return sc

    @staticmethod
    def _diag(name):
        if not hasattr(lib, name):
            raise RuntimeError(f"{name}: diagnostic build only (make -C rust-crdt_amd diag; CRDTS_HIP_DIAG=1)")
        return getattr(lib, name)

    def set_blocks_per_cu(self, k):
        """Diagnostic build only: workgroups per CU of the Orswot kernel."""
        check(self._diag("crdt_ctx_set_blocks_per_cu")(self.ctx, int(k)), "set_blocks_per_cu")

    def set_variant(self, v):
        """Diagnostic build only: Orswot kernel variant (0 = the product kernel)."""
        check(self._diag("crdt_ctx_set_variant")(self.ctx, int(v)), "set_variant")

    def set_list_cap(self, cap):
        """Test knob: capacity of the general-path object list (overflow -> full scan)."""
        check(lib.crdt_ctx_set_list_cap(self.ctx, int(cap)), "set_list_cap")

    def set_arena_limit(self, max_bytes):
        """Largest replica-exchange arena the context may allocate (0: no limit; crdt_ctx_set_arena_limit)."""
        check(lib.crdt_ctx_set_arena_limit(self.ctx, int(max_bytes)), "set_arena_limit")

    def host_syncs(self):
        """Host synchronisations the context's replica joins made so far (crdt_ctx_host_syncs)."""
        return int(lib.crdt_ctx_host_syncs(self.ctx))
