"""Engine's replica anti-entropy calls: the RCCL communicator of the context,
the u64 max collectives and the owner-sharded Orswot join, over RCCL, over a
caller transport, or with every replica on this device (include/crdts_hip.h
crdt_comm_*, crdt_replica_*, crdt_orswot_replica_join*). replica.py is the
torch.distributed front end over them."""
from __future__ import annotations

import ctypes as C

from ._lib import CRDT_COMM_ID_BYTES, Batch, CrdtError, check, lib
from ._util import _torch, dptr
from .batches import OrswotBatch


class ReplicaEngine:
    """Engine's replica methods (mixed into crdts_hip.Engine)."""

    @staticmethod
    def comm_unique_id() -> bytes:
        """crdt_comm_unique_id: the RCCL id rank 0 hands to every rank."""
        buf = (C.c_uint8 * CRDT_COMM_ID_BYTES)()
        check(lib.crdt_comm_unique_id(buf), "comm_unique_id")
        return bytes(buf)

    def comm_init(self, uid: bytes, n_ranks: int, rank: int):
        """crdt_comm_init (collective): this context owns an RCCL communicator."""
        if len(uid) != CRDT_COMM_ID_BYTES:
            raise CrdtError(-1, "comm id must be CRDT_COMM_ID_BYTES bytes")
        buf = (C.c_uint8 * CRDT_COMM_ID_BYTES).from_buffer_copy(uid)
        check(lib.crdt_comm_init(self.ctx, buf, int(n_ranks), int(rank)), "comm_init")
        self.n_ranks, self.rank = int(n_ranks), int(rank)

    @property
    def has_comm(self):
        return getattr(self, "n_ranks", 0) > 0

    def comm_destroy(self):
        check(lib.crdt_comm_destroy(self.ctx), "comm_destroy")
        self.n_ranks = 0

    def comm_count(self):
        """Ranks of the context's RCCL communicator (ncclCommCount)."""
        n = C.c_int(0)
        check(lib.crdt_comm_count(self.ctx, C.byref(n)), "comm_count")
        return n.value

    # ------------------------------------------------ u64 max over ranks
    def replica_allreduce_max(self, rows, stream=None):
        """In place: rows := max over ranks (u64 order), ncclUint64 + ncclMax
        (src/vclock.rs:131-137 across replicas). rows: int64 device tensor of u64."""
        check(lib.crdt_replica_allreduce_max(self.ctx, C.c_void_p(rows.data_ptr()), rows.numel(),
                                             self._stream(stream)), "replica_allreduce_max")
        return rows

    def replica_reduce_scatter_max(self, rows, stream=None):
        """The owner shard of the u64 max over ranks: rank r gets words
        [r n/N, (r+1) n/N) (crdt_replica_reduce_scatter_max). Returns a new
        int64 device tensor of n/N words."""
        torch = _torch()
        flat = rows.reshape(-1)
        n_ranks = self.n_ranks
        if flat.numel() % n_ranks:
            raise CrdtError(-1, "reduce_scatter: word count not a multiple of the rank count")
        out = torch.empty(flat.numel() // n_ranks, dtype=torch.int64, device=flat.device)
        check(lib.crdt_replica_reduce_scatter_max(self.ctx, C.c_void_p(flat.data_ptr()), flat.numel(),
                                                  C.c_void_p(out.data_ptr()), self._stream(stream)),
              "replica_reduce_scatter_max")
        return out

    def replica_allreduce_max_transport(self, rows, transport, stream=None):
        """rows (a device int64 tensor read as u64) := its max over ranks, in
        place, over a caller transport (crdt_replica_allreduce_max_transport:
        owner-sharded reduce-scatter with the dense max kernel + all-gather;
        `transport` has a `.c` TransportC, e.g. replica.GlooTransport)."""
        check(lib.crdt_replica_allreduce_max_transport(self.ctx, C.byref(transport.c), C.c_void_p(rows.data_ptr()),
                                                       rows.numel(), self._stream(stream)),
              "replica_allreduce_max_transport")
        return rows

    def replica_reduce_scatter_max_transport(self, rows, transport, stream=None):
        """The owner shard of the u64 max over ranks over a caller transport
        (crdt_replica_reduce_scatter_max_transport): rank r gets words
        [r n/N, (r+1) n/N). Returns a new int64 device tensor of n/N words.
        A word count N does not divide is CRDT_EINVAL on EVERY rank: the C ABI
        checks it with the peers (a local early return here would leave them
        waiting in the exchange)."""
        torch = _torch()
        flat = rows.reshape(-1)
        out = torch.empty(max(1, flat.numel() // transport.world), dtype=torch.int64, device=flat.device)
        check(lib.crdt_replica_reduce_scatter_max_transport(self.ctx, C.byref(transport.c),
                                                            C.c_void_p(flat.data_ptr()), flat.numel(),
                                                            C.c_void_p(out.data_ptr()), self._stream(stream)),
              "replica_reduce_scatter_max_transport")
        return out[: flat.numel() // transport.world]

    # ------------------------------------------------ the owner-sharded Orswot join
    def orswot_replica_join_bound(self, B: OrswotBatch, stream=None):
        """Output bytes that suffice for crdt_orswot_replica_join (collective:
        the sum of every rank's replica bytes)."""
        b = B.cbatch()
        bound = C.c_size_t(0)
        check(lib.crdt_orswot_replica_join_bound(self.ctx, C.byref(b), C.byref(bound), self._stream(stream)),
              "replica_join_bound")
        return max(16, bound.value)

    def orswot_replica_alloc_out(self, B: OrswotBatch, bound: int):
        torch = _torch()
        dev = f"cuda:{self.device}"
        return OrswotBatch(torch.empty(max(16, bound), dtype=torch.uint8, device=dev),
                           torch.empty(B.n_obj, dtype=torch.int64, device=dev), B.n_actors, max(16, bound), B.flags)

    def orswot_replica_join(self, B: OrswotBatch, out: OrswotBatch | None = None, stream=None):
        """((r0 ⊔ r1) ⊔ ...) of every rank's replica, owner-sharded over RCCL;
        the same packed batch on every rank (crdt_orswot_replica_join). `out`
        (from orswot_replica_alloc_out with a bound from
        orswot_replica_join_bound) is reused when given, so a repeated join
        runs no bound collective and allocates nothing."""
        if out is None:
            out = self.orswot_replica_alloc_out(B, self.orswot_replica_join_bound(B, stream))
        b = B.cbatch()
        used = C.c_size_t(0)
        check(lib.crdt_orswot_replica_join(self.ctx, C.byref(b), B.n_actors, B.flags, dptr(out.base), dptr(out.off),
                                           out.base.numel(), C.byref(used), self._stream(stream)),
              "orswot_replica_join")
        return OrswotBatch(out.base, out.off, B.n_actors, max(16, used.value), B.flags)

    def orswot_replica_join_transport(self, B: OrswotBatch, transport, out: OrswotBatch | None = None,
                                      out_bytes: int | None = None, stream=None):
        """The same owner-sharded join over a caller transport
        (crdt_orswot_replica_join_transport; `transport` has a `.c` TransportC,
        e.g. replica.GlooTransport). out_bytes defaults to world x this
        replica's bytes rounded up (enough when replicas are of similar size;
        pass the all-reduced sum otherwise)."""
        if out is None:
            cap = out_bytes if out_bytes is not None else transport.world * ((B.bytes + 15) // 16 * 16 + 16)
            out = self.orswot_replica_alloc_out(B, cap)
        b = B.cbatch()
        used = C.c_size_t(0)
        check(lib.crdt_orswot_replica_join_transport(self.ctx, C.byref(transport.c), C.byref(b), B.n_actors, B.flags,
                                                     dptr(out.base), dptr(out.off), out.base.numel(), C.byref(used),
                                                     self._stream(stream)), "orswot_replica_join_transport")
        return OrswotBatch(out.base, out.off, B.n_actors, max(16, used.value), B.flags)

    def orswot_replica_join_local(self, batches, stream=None):
        """The same owner-sharded join with every replica a virtual rank on this
        device (crdt_orswot_replica_join_local)."""
        torch = _torch()
        arr = (Batch * len(batches))(*[x.cbatch() for x in batches])
        cap = sum((x.bytes + 15) // 16 * 16 for x in batches)
        dev = f"cuda:{self.device}"
        base = torch.empty(max(16, cap), dtype=torch.uint8, device=dev)
        off = torch.empty(batches[0].n_obj, dtype=torch.int64, device=dev)
        used = C.c_size_t(0)
        check(lib.crdt_orswot_replica_join_local(self.ctx, arr, len(batches), batches[0].n_actors, batches[0].flags,
                                                 dptr(base), dptr(off), base.numel(), C.byref(used),
                                                 self._stream(stream)), "orswot_replica_join_local")
        return OrswotBatch(base, off, batches[0].n_actors, max(16, used.value), batches[0].flags)
