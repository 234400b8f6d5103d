"""ctypes binding of libcrdts_hip.so (C ABI: include/crdts_hip.h).

The shared library is the product; this module only declares its symbols.
There is no CPU fallback anywhere: if the library is missing, importing the
package raises.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)  # rust-crdt_amd/
LIB_PATH = os.path.join(ROOT, "lib", "libcrdts_hip.so")
# tools/ may select the diagnostic build (make -C rust-crdt_amd diag: kernel
# variants, phase stamps, tuning knobs) with CRDTS_HIP_DIAG=1; never the product.
if os.environ.get("CRDTS_HIP_DIAG") == "1":
    LIB_PATH = os.path.join(ROOT, "lib", "libcrdts_hip_diag.so")
# A/B builds of a compile-time knob (tools/): CRDTS_HIP_AB=<tag> loads
# lib/libcrdts_hip_ab_<tag>.so; never the product.
if os.environ.get("CRDTS_HIP_AB"):
    LIB_PATH = os.path.join(ROOT, "lib", f"libcrdts_hip_ab_{os.environ['CRDTS_HIP_AB']}.so")
DIAG_SYMBOLS = {"crdt_ctx_set_blocks_per_cu", "crdt_ctx_set_variant", "crdt_ctx_debug_read"}

CRDT_OK = 0
CRDT_EINVAL = -1
CRDT_ENONCANON = -2
CRDT_EHIP = -3
CRDT_ECAPACITY = -4
CRDT_ECOMM = -5
CRDT_ENODEV = -6


class CrdtError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = lib.crdt_strerror(code).decode() if lib is not None else str(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


class Batch(C.Structure):
    _fields_ = [("base", C.c_void_p), ("off", C.c_void_p), ("n_obj", C.c_size_t), ("bytes", C.c_size_t)]


class GenParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_actors", "member_universe", "ancestor_adds", "min_div_ops",
                                          "max_div_ops", "pct_add", "pct_future_rm", "pct_deferred_obj",
                                          "pct_shared_actor")]


class RepParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("universe", "pool_actors", "own_actors", "member_universe",
                                          "ancestor_adds", "min_div_ops", "max_div_ops", "pct_add",
                                          "pct_future_rm", "pct_deferred_obj")]


SPARSE_CLOCK = 1  # CRDT_ORSWOT_SPARSE_CLOCK

# Every symbol include/crdts_hip.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "crdt_ctx_create", "crdt_ctx_destroy", "crdt_ctx_status", "crdt_strerror", "crdt_abi_version",
    "crdt_vclock_dense_merge", "crdt_gcounter_merge", "crdt_pncounter_merge",
    "crdt_orswot_record_bytes", "crdt_orswot_merge", "crdt_orswot_merge_host", "crdt_orswot_validate",
    "crdt_orswot_compact_scratch_bytes", "crdt_orswot_compact",
    "crdt_orswot_generate", "crdt_orswot_gen_side", "crdt_orswot_gen_free", "crdt_dense_generate",
    "crdt_host_orswot_new", "crdt_host_orswot_clone", "crdt_host_orswot_free",
    "crdt_host_orswot_apply_add", "crdt_host_orswot_apply_rm", "crdt_host_orswot_encode",
    "crdt_host_orswot_decode", "crdt_orswot_record_bytes_ex", "crdt_orswot_merge_ex",
    "crdt_orswot_validate_ex", "crdt_orswot_generate_replicas", "crdt_host_orswot_encode_ex",
    "crdt_orswot_bincode_record_sizes", "crdt_orswot_from_bincode", "crdt_orswot_bincode_sizes",
    "crdt_orswot_to_bincode", "crdt_orswot_apply", "crdt_vclock_partial_cmp", "crdt_mvreg_merge",
    "crdt_map_mvreg_merge", "crdt_map_orswot_merge", "crdt_ctx_set_list_cap", "crdt_orswot_bincode_record_bounds",
    "crdt_comm_unique_id", "crdt_comm_init", "crdt_comm_destroy", "crdt_replica_allreduce_max",
    "crdt_replica_reduce_scatter_max",
    "crdt_orswot_replica_join_bound", "crdt_orswot_replica_join", "crdt_orswot_replica_join_local",
    "crdt_comm_count", "crdt_orswot_replica_join_transport", "crdt_orswot_generate_replicas_subset",
    "crdt_dense_merge_host", "crdt_vclock_csr_merge", "crdt_gcounter_csr_merge", "crdt_pncounter_csr_merge",
    "crdt_orswot_truncate", "crdt_ctx_host_syncs", "crdt_orswot_fold", "crdt_ctx_set_arena_limit",
    "crdt_map_map_merge_scratch_bytes", "crdt_map_map_merge", "crdt_replica_allreduce_max_transport",
    "crdt_replica_reduce_scatter_max_transport", "crdt_map_mvreg_apply", "crdt_map_orswot_apply",
    "crdt_map_map_apply_scratch_bytes", "crdt_map_map_apply",
    "crdt_mvreg_apply", "crdt_mvreg_truncate", "crdt_mvreg_read_clock",
    "crdt_map_mvreg_truncate", "crdt_map_orswot_truncate", "crdt_map_map_truncate_scratch_bytes",
    "crdt_map_map_truncate",
    "crdt_mvreg_from_bincode", "crdt_mvreg_bincode_sizes", "crdt_mvreg_to_bincode",
    "crdt_map_mvreg_from_bincode", "crdt_map_mvreg_bincode_sizes", "crdt_map_mvreg_to_bincode",
    "crdt_map_orswot_from_bincode", "crdt_map_orswot_bincode_sizes", "crdt_map_orswot_to_bincode",
    "crdt_map_map_from_bincode", "crdt_map_map_bincode_sizes", "crdt_map_map_to_bincode",
    "crdt_vclock_dense_apply", "crdt_gcounter_apply", "crdt_pncounter_apply", "crdt_vclock_dense_truncate",
    "crdt_vclock_dense_subtract", "crdt_vclock_dense_intersection", "crdt_gcounter_value", "crdt_pncounter_value",
    "crdt_vclock_dense_get", "crdt_vclock_csr_truncate", "crdt_vclock_csr_subtract", "crdt_vclock_csr_intersection",
    "crdt_vclock_csr_apply", "crdt_gcounter_csr_apply", "crdt_gcounter_csr_value", "crdt_vclock_csr_get",
    "crdt_orswot_read_sizes", "crdt_orswot_read", "crdt_map_read_sizes", "crdt_map_read", "crdt_map_mvreg_get",
    "crdt_map_orswot_get_sizes", "crdt_map_orswot_get", "crdt_map_map_get",
    "crdt_lwwreg_merge", "crdt_lwwreg_apply", "crdt_lwwreg_fold", "crdt_lwwreg_from_bincode",
    "crdt_lwwreg_to_bincode", "crdt_mvreg_fold",
    "crdt_clock_dense_from_bincode", "crdt_clock_dense_bincode_sizes", "crdt_clock_dense_to_bincode",
    "crdt_clock_csr_bincode_lens", "crdt_clock_csr_from_bincode", "crdt_clock_csr_bincode_sizes",
    "crdt_clock_csr_to_bincode", "crdt_clock_ops_from_bincode", "crdt_clock_ops_to_bincode",
    "crdt_ops_bincode_clk_lens", "crdt_ops_from_bincode", "crdt_ops_bincode_sizes", "crdt_ops_to_bincode",
    "crdt_clock_dense_fold", "crdt_clock_csr_fold",
]

CRDT_COMM_ID_BYTES = 128
CLOCK_FOLD_MAX_REPS = 32  # CRDT_CLOCK_FOLD_MAX_REPS
CLOCK_FOLD_STAGE_ENTRIES = 512  # CRDT_CLOCK_FOLD_STAGE_ENTRIES: the longest sum of an object's runs that is folded in LDS


def hip_runtime():
    """The HIP runtime library this process already has loaded (torch's), found
    in /proc/self/maps — not a fixed soname, so a ROCm major version change does
    not load a second runtime. Falls back to the unversioned soname."""
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.split()[-1] if line.strip() else ""
                if os.path.basename(path).startswith("libamdhip64.so"):
                    return C.CDLL(path)
    except OSError:
        pass
    return C.CDLL("libamdhip64.so")


def _spec(words):
    """"kind:u32 key" -> (("kind", True), ("key", False)): array members in ABI
    order, u64 elements unless marked u32."""
    return tuple((w.split(":")[0], w.endswith(":u32")) for w in words.split())


def _cstruct(pyname, cname, members):
    return type(pyname, (C.Structure,), {"__doc__": f"{cname} (include/crdts_hip.h).", "_fields_": members})


class OpLayout:
    """One op / query struct of the ABI: its array members in ABI order with
    their element type, then `counts`, the trailing size_t members, each with
    the array whose length it is. `op_type` is the struct's CRDT_OPS_* code on
    the wire (None: not an op stream of crdt_ops_*_bincode) and `wire`, for
    an op stream, its arrays after obj_end under their crdt_op_arrays names
    (None otherwise); `batch` is the Python class that carries it. The ctypes struct, the batch classes and ops_bincode all
    read this one description."""

    def __init__(self, pyname, cname, words, counts, op_type=None, batch=None, wire=()):
        spec = _spec(words)
        self.cname, self.counts, self.op_type, self.batch = cname, tuple(counts), op_type, batch
        self.fields = tuple(f for f, _ in spec)
        self.u32 = tuple(f for f, u in spec if u)
        self.wire = None if op_type is None else tuple(dict(wire).get(f, f) for f in self.fields[1:])
        self.ctype = _cstruct(pyname, cname, [(f, C.c_void_p) for f in self.fields] +
                              [(c, C.c_size_t) for c, _ in self.counts])


_OPS_CLK = (("n_ops", "kind"), ("n_clk", "clk_act"))
OP_LAYOUTS = {l.cname: l for l in (
    OpLayout("Ops", "crdt_orswot_ops", "obj_end kind:u32 member actor:u32 counter clk_end clk_act:u32 clk_ctr",
             _OPS_CLK, 0, "OrswotOps", wire={"member": "key2"}),
    OpLayout("MVRegOpsC", "crdt_mvreg_ops", "obj_end val clk_end clk_act:u32 clk_ctr",
             (("n_ops", "val"), ("n_clk", "clk_act")), 1, "MVRegOps"),
    OpLayout("MapOpsC", "crdt_map_mvreg_ops",
             "obj_end kind:u32 key actor:u32 counter val clk_end clk_act:u32 clk_ctr", _OPS_CLK, 2, "MapOps"),
    OpLayout("MapOrswotOpsC", "crdt_map_orswot_ops",
             "obj_end kind:u32 key actor:u32 counter member clk_end clk_act:u32 clk_ctr", _OPS_CLK, 3, "MapOrswotOps",
             wire={"member": "key2"}),
    OpLayout("MapMapOpsC", "crdt_map_map_ops",
             "obj_end kind:u32 key actor:u32 counter key2 actor2:u32 counter2 val clk_end clk_act:u32 clk_ctr",
             _OPS_CLK, 4, "MapMapOps"),
    OpLayout("ClockOpsC", "crdt_clock_ops", "obj_end actor:u32 counter dir:u32", (("n_ops", "actor"),)),
    OpLayout("LWWOpsC", "crdt_lwwreg_ops", "obj_end val marker", (("n_ops", "val"),)),
    OpLayout("ReadQueriesC", "crdt_read_queries", "obj_end kind:u32 key actor:u32", (("n_q", "kind"),)),
    OpLayout("OpArraysC", "crdt_op_arrays",
             "kind:u32 key actor:u32 counter key2 actor2:u32 counter2 val clk_end clk_act:u32 clk_ctr", _OPS_CLK),
)}
Ops = OP_LAYOUTS["crdt_orswot_ops"].ctype
MVRegOpsC = OP_LAYOUTS["crdt_mvreg_ops"].ctype
MapOpsC = OP_LAYOUTS["crdt_map_mvreg_ops"].ctype
MapOrswotOpsC = OP_LAYOUTS["crdt_map_orswot_ops"].ctype
MapMapOpsC = OP_LAYOUTS["crdt_map_map_ops"].ctype
ClockOpsC = OP_LAYOUTS["crdt_clock_ops"].ctype
LWWOpsC = OP_LAYOUTS["crdt_lwwreg_ops"].ctype
ReadQueriesC = OP_LAYOUTS["crdt_read_queries"].ctype
OpArraysC = OP_LAYOUTS["crdt_op_arrays"].ctype
OP_ARRAYS_FIELDS = OP_LAYOUTS["crdt_op_arrays"].fields


class SlabLayout:
    """One Map slab struct of the ABI: per array member, in ABI order, its
    element type and its axes after the object axis — each a capacity with the
    count array that bounds it ("kcap<n_keys": slot k of object i is used iff
    k < n_keys[i], and so down the nesting), or "A", the actor axis, which is
    always used — then the u32 capacities `caps`, then `inner`, the layout of
    a nested slab struct. The ctypes struct and the slab classes (shapes,
    dtypes, used-slot masks) read this one description."""

    def __init__(self, pyname, cname, caps, members, inner=None):
        spec = [(_spec(m.split()[0])[0], m.split()[1:]) for m in members]
        self.cname, self.caps, self.inner = cname, tuple(caps), inner
        self.fields = tuple(f for (f, _), _ in spec)
        self.u32 = tuple(f for (f, u), _ in spec if u)
        self.axes = {f: tuple(tuple(x.split("<")) if "<" in x else (x, None) for x in ax) for (f, _), ax in spec}
        self.ctype = _cstruct(pyname, cname, [(f, C.c_void_p) for f in self.fields] +
                              [(c, C.c_uint32) for c in self.caps] + ([("inner", inner.ctype)] if inner else []))


_MAP_OUTER = ("clock A", "n_keys:u32", "keys kcap<n_keys", "eclock kcap<n_keys A")
_MAP_DEFERRED = ("n_def:u32", "dclock dcap<n_def A", "dset_n:u32 dcap<n_def", "dset dcap<n_def scap<dset_n")
MAP_MVREG_SLAB = SlabLayout("MapSlabC", "crdt_map_mvreg_slab", ("kcap", "mcap", "dcap", "scap"), _MAP_OUTER + (
    "mv_n:u32 kcap<n_keys", "mv_clock kcap<n_keys mcap<mv_n A", "mv_val kcap<n_keys mcap<mv_n") + _MAP_DEFERRED)
MAP_MAP_SLAB = SlabLayout("MapMapSlabC", "crdt_map_map_slab", ("kcap", "dcap", "scap"), _MAP_OUTER + _MAP_DEFERRED,
                          inner=MAP_MVREG_SLAB)  # the nested maps: key slot k of object i is inner object i * kcap + k
MAP_ORSWOT_SLAB = SlabLayout("MapOrswotSlabC", "crdt_map_orswot_slab",
                             ("kcap", "mcap", "vdcap", "vscap", "dcap", "scap"), _MAP_OUTER + (
    "vclock kcap<n_keys A", "vn_mem:u32 kcap<n_keys", "vmem kcap<n_keys mcap<vn_mem",
    "vmclock kcap<n_keys mcap<vn_mem A", "vn_def:u32 kcap<n_keys", "vdclock kcap<n_keys vdcap<vn_def A",
    "vdset_n:u32 kcap<n_keys vdcap<vn_def", "vdset kcap<n_keys vdcap<vn_def vscap<vdset_n") + _MAP_DEFERRED)
MapSlabC, MapMapSlabC, MapOrswotSlabC = MAP_MVREG_SLAB.ctype, MAP_MAP_SLAB.ctype, MAP_ORSWOT_SLAB.ctype


class ClockCsr(C.Structure):
    """crdt_clock_csr (include/crdts_hip.h)."""
    _fields_ = [("off", C.c_void_p), ("len", C.c_void_p), ("act", C.c_void_p), ("ctr", C.c_void_p),
                ("n_obj", C.c_size_t), ("n_entries", C.c_size_t)]


class LWWViewC(C.Structure):
    """crdt_lwwreg_view (include/crdts_hip.h)."""
    _fields_ = [("val", C.c_void_p), ("marker", C.c_void_p)]


class MVRegViewC(C.Structure):
    """crdt_mvreg_view (include/crdts_hip.h)."""
    _fields_ = [("n", C.c_void_p), ("clk", C.c_void_p), ("val", C.c_void_p), ("cap", C.c_uint32)]


READ_SIZES_FIELDS = ("val", "slot", "dot_ctr", "add_len", "rm_len", "list_len")


class ReadSizesC(C.Structure):
    """crdt_read_sizes (include/crdts_hip.h)."""
    _fields_ = [(f, C.c_void_p) for f in READ_SIZES_FIELDS]


class ReadOutC(C.Structure):
    """crdt_read_out (include/crdts_hip.h)."""
    _fields_ = [("add_end", C.c_void_p), ("add_act", C.c_void_p), ("add_ctr", C.c_void_p), ("n_add", C.c_size_t),
                ("rm_end", C.c_void_p), ("rm_act", C.c_void_p), ("rm_ctr", C.c_void_p), ("n_rm", C.c_size_t),
                ("list_end", C.c_void_p), ("list_key", C.c_void_p), ("n_list", C.c_size_t)]


class MapReadViewC(C.Structure):
    """crdt_map_read_view (include/crdts_hip.h)."""
    _fields_ = [(f, C.c_void_p) for f in ("clock", "n_keys", "keys", "eclock")] + [("kcap", C.c_uint32)]


class ClockCsrOut(C.Structure):
    """crdt_clock_csr_out (include/crdts_hip.h)."""
    _fields_ = [("off", C.c_void_p), ("len", C.c_void_p), ("act", C.c_void_p), ("ctr", C.c_void_p),
                ("n_entries", C.c_size_t)]


class OpWidthsC(C.Structure):
    """crdt_op_widths (include/crdts_hip.h)."""
    _fields_ = [(f, C.c_uint32) for f in ("actor_bytes", "key_bytes", "key2_bytes", "val_bytes")]


class Xfer(C.Structure):
    """crdt_xfer (include/crdts_hip.h)."""
    _fields_ = [("peer", C.c_int), ("src", C.c_void_p), ("dst", C.c_void_p), ("bytes", C.c_size_t)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64))
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Xfer), C.c_size_t, C.POINTER(Xfer), C.c_size_t,
                          C.c_void_p)


class TransportC(C.Structure):
    """crdt_transport (include/crdts_hip.h): a caller-provided transport."""
    _fields_ = [("n_ranks", C.c_int), ("rank", C.c_int), ("user", C.c_void_p), ("allgather", ALLGATHER_FN),
                ("exchange", EXCHANGE_FN)]


def _load():
    # One HIP runtime per process: torch ships its own libamdhip64.so.7. Load
    # torch first so this library's libamdhip64.so.7 dependency binds to the
    # already-loaded copy (same SONAME) instead of a second runtime from
    # /opt/rocm, which would fail to open the device next to torch's.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"crdts_hip: native library missing at {LIB_PATH}; build it with "
            "`make -C rust-crdt_amd` or `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    P, I, SZ, U32, U64 = C.c_void_p, C.c_int, C.c_size_t, C.c_uint32, C.c_uint64
    BP = C.POINTER(Batch)
    sig = {
        "crdt_ctx_create": (I, [C.POINTER(P), I]),
        "crdt_ctx_destroy": (I, [P]),
        "crdt_ctx_status": (I, [P, P]),
        "crdt_ctx_set_blocks_per_cu": (I, [P, I]),
        "crdt_ctx_set_list_cap": (I, [P, U32]),
        "crdt_ctx_host_syncs": (U64, [P]),
        "crdt_ctx_set_arena_limit": (I, [P, SZ]),
        "crdt_orswot_fold": (I, [P, BP, U32, U32, U32, P, P, SZ, P]),
        "crdt_ctx_set_variant": (I, [P, I]),
        "crdt_ctx_debug_read": (I, [P, P, SZ, P]),
        "crdt_strerror": (C.c_char_p, [I]),
        "crdt_abi_version": (I, []),
        "crdt_vclock_dense_merge": (I, [P, P, P, SZ, U32, P]),
        "crdt_gcounter_merge": (I, [P, P, P, SZ, U32, P]),
        "crdt_pncounter_merge": (I, [P, P, P, SZ, U32, P]),
        "crdt_orswot_record_bytes": (SZ, [U32] * 6),
        "crdt_orswot_merge": (I, [P, BP, BP, P, P, SZ, U32, P]),
        "crdt_orswot_merge_host": (I, [P, P, P, SZ, P, P, SZ, SZ, U32, P, P, SZ, C.POINTER(SZ)]),
        "crdt_orswot_validate": (I, [P, BP, U32, P]),
        "crdt_orswot_compact_scratch_bytes": (SZ, [SZ]),
        "crdt_orswot_compact": (I, [P, BP, P, P, SZ, P, P]),
        "crdt_orswot_generate": (I, [U64, SZ, SZ, C.POINTER(GenParams), I, C.POINTER(P)]),
        "crdt_orswot_gen_side": (I, [P, I, C.POINTER(P), C.POINTER(P), C.POINTER(SZ)]),
        "crdt_orswot_gen_free": (None, [P]),
        "crdt_dense_generate": (I, [U64, SZ, SZ, U32, U32, U32, I, P]),
        "crdt_host_orswot_new": (P, []),
        "crdt_host_orswot_clone": (P, [P]),
        "crdt_host_orswot_free": (None, [P]),
        "crdt_host_orswot_apply_add": (I, [P, U32, U64, U64]),
        "crdt_host_orswot_apply_rm": (I, [P, U64, P, P, U32]),
        "crdt_host_orswot_encode": (C.c_long, [P, U32, P, SZ]),
        "crdt_host_orswot_decode": (P, [P, SZ]),
        "crdt_orswot_record_bytes_ex": (SZ, [U32] * 7),
        "crdt_orswot_merge_ex": (I, [P, BP, BP, P, P, SZ, U32, U32, P]),
        "crdt_orswot_validate_ex": (I, [P, BP, U32, U32, P]),
        "crdt_orswot_generate_replicas": (I, [U64, SZ, SZ, C.POINTER(RepParams), U32, U32, I, C.POINTER(P)]),
        "crdt_host_orswot_encode_ex": (C.c_long, [P, U32, U32, P, SZ]),
        "crdt_orswot_bincode_record_sizes": (I, [P, P, SZ, P, P, SZ, U32, U32, U32, U32, P, P]),
        "crdt_orswot_bincode_record_bounds": (I, [P, P, SZ, U32, U32, U32, U32, P, P]),
        "crdt_orswot_from_bincode": (I, [P, P, SZ, P, P, SZ, U32, U32, U32, U32, P, P, SZ, P]),
        "crdt_orswot_bincode_sizes": (I, [P, BP, U32, U32, U32, U32, P, P]),
        "crdt_orswot_to_bincode": (I, [P, BP, U32, U32, U32, U32, P, P, SZ, P]),
        "crdt_orswot_apply": (I, [P, BP, C.POINTER(Ops), U32, U32, P, P, SZ, P]),
        "crdt_vclock_partial_cmp": (I, [P, P, P, SZ, U32, P, P]),
        "crdt_mvreg_merge": (I, [P, P, P, P, U32, P, P, P, U32, P, P, P, U32, SZ, U32, P]),
        "crdt_mvreg_apply": (I, [P, P, P, P, U32, C.POINTER(MVRegOpsC), P, P, P, U32, SZ, U32, P]),
        "crdt_mvreg_truncate": (I, [P, P, P, P, U32, P, P, P, P, U32, SZ, U32, P]),
        "crdt_mvreg_read_clock": (I, [P, P, P, U32, P, SZ, U32, P]),
        "crdt_map_mvreg_merge": (I, [P, C.POINTER(MapSlabC), C.POINTER(MapSlabC), C.POINTER(MapSlabC), SZ, U32, P]),
        "crdt_map_mvreg_apply": (I, [P, C.POINTER(MapSlabC), C.POINTER(MapOpsC), C.POINTER(MapSlabC), SZ, U32, P]),
        "crdt_map_orswot_merge": (I, [P, C.POINTER(MapOrswotSlabC), C.POINTER(MapOrswotSlabC),
                                      C.POINTER(MapOrswotSlabC), SZ, U32, P]),
        "crdt_map_orswot_apply": (I, [P, C.POINTER(MapOrswotSlabC), C.POINTER(MapOrswotOpsC),
                                      C.POINTER(MapOrswotSlabC), SZ, U32, P]),
        "crdt_map_map_merge_scratch_bytes": (SZ, [C.POINTER(MapMapSlabC), SZ, U32]),
        "crdt_map_map_merge": (I, [P, C.POINTER(MapMapSlabC), C.POINTER(MapMapSlabC), C.POINTER(MapMapSlabC), SZ,
                                   U32, P, SZ, P]),
        "crdt_map_map_apply_scratch_bytes": (SZ, [C.POINTER(MapMapSlabC), SZ, U32]),
        "crdt_map_map_apply": (I, [P, C.POINTER(MapMapSlabC), C.POINTER(MapMapOpsC), C.POINTER(MapMapSlabC), SZ,
                                   U32, P, SZ, P]),
        "crdt_map_mvreg_truncate": (I, [P, C.POINTER(MapSlabC), P, C.POINTER(MapSlabC), SZ, U32, P]),
        "crdt_map_orswot_truncate": (I, [P, C.POINTER(MapOrswotSlabC), P, C.POINTER(MapOrswotSlabC), SZ, U32, P]),
        "crdt_map_map_truncate_scratch_bytes": (SZ, [C.POINTER(MapMapSlabC), SZ, U32]),
        "crdt_map_map_truncate": (I, [P, C.POINTER(MapMapSlabC), P, C.POINTER(MapMapSlabC), SZ, U32, P, SZ, P]),
        "crdt_mvreg_from_bincode": (I, [P, P, SZ, P, P, SZ, U32, U32, U32, P, P, P, U32, P]),
        "crdt_mvreg_bincode_sizes": (I, [P, P, P, P, U32, SZ, U32, U32, U32, P, P]),
        "crdt_mvreg_to_bincode": (I, [P, P, P, P, U32, SZ, U32, U32, U32, P, P, SZ, P]),
        "crdt_map_mvreg_from_bincode": (I, [P, P, SZ, P, P, SZ, U32, U32, U32, U32, C.POINTER(MapSlabC), P]),
        "crdt_map_mvreg_bincode_sizes": (I, [P, C.POINTER(MapSlabC), SZ, U32, U32, U32, U32, P, P]),
        "crdt_map_mvreg_to_bincode": (I, [P, C.POINTER(MapSlabC), SZ, U32, U32, U32, U32, P, P, SZ, P]),
        "crdt_map_orswot_from_bincode": (I, [P, P, SZ, P, P, SZ, U32, U32, U32, U32, C.POINTER(MapOrswotSlabC), P]),
        "crdt_map_orswot_bincode_sizes": (I, [P, C.POINTER(MapOrswotSlabC), SZ, U32, U32, U32, U32, P, P]),
        "crdt_map_orswot_to_bincode": (I, [P, C.POINTER(MapOrswotSlabC), SZ, U32, U32, U32, U32, P, P, SZ, P]),
        "crdt_map_map_from_bincode": (I, [P, P, SZ, P, P, SZ, U32, U32, U32, U32, U32, C.POINTER(MapMapSlabC), P]),
        "crdt_map_map_bincode_sizes": (I, [P, C.POINTER(MapMapSlabC), SZ, U32, U32, U32, U32, U32, P, P]),
        "crdt_map_map_to_bincode": (I, [P, C.POINTER(MapMapSlabC), SZ, U32, U32, U32, U32, U32, P, P, SZ, P]),
        "crdt_comm_unique_id": (I, [P]),
        "crdt_comm_init": (I, [P, P, I, I]),
        "crdt_comm_destroy": (I, [P]),
        "crdt_replica_allreduce_max": (I, [P, P, SZ, P]),
        "crdt_replica_reduce_scatter_max": (I, [P, P, SZ, P, P]),
        "crdt_orswot_replica_join_bound": (I, [P, BP, C.POINTER(SZ), P]),
        "crdt_orswot_replica_join": (I, [P, BP, U32, U32, P, P, SZ, C.POINTER(SZ), P]),
        "crdt_orswot_replica_join_local": (I, [P, BP, U32, U32, U32, P, P, SZ, C.POINTER(SZ), P]),
        "crdt_comm_count": (I, [P, C.POINTER(I)]),
        "crdt_dense_merge_host": (I, [P, P, P, SZ, U32]),
        "crdt_orswot_truncate": (I, [P, BP, C.POINTER(ClockCsr), U32, U32, P, P, SZ, P]),
        "crdt_vclock_csr_merge": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockCsr), C.POINTER(ClockCsrOut), P]),
        "crdt_gcounter_csr_merge": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockCsr), C.POINTER(ClockCsrOut), P]),
        "crdt_pncounter_csr_merge": (I, [P] + [C.POINTER(ClockCsr)] * 4 + [C.POINTER(ClockCsrOut)] * 2 + [P]),
        "crdt_clock_dense_fold": (I, [P, C.POINTER(P), U32, P, SZ, U32, P]),
        "crdt_clock_csr_fold": (I, [P, C.POINTER(ClockCsr), U32, C.POINTER(ClockCsrOut), P]),
        "crdt_vclock_dense_apply": (I, [P, P, C.POINTER(ClockOpsC), SZ, U32, P]),
        "crdt_gcounter_apply": (I, [P, P, C.POINTER(ClockOpsC), SZ, U32, P]),
        "crdt_pncounter_apply": (I, [P, P, C.POINTER(ClockOpsC), SZ, U32, P]),
        "crdt_vclock_dense_truncate": (I, [P, P, P, SZ, U32, P]),
        "crdt_vclock_dense_subtract": (I, [P, P, P, SZ, U32, P]),
        "crdt_vclock_dense_intersection": (I, [P, P, P, SZ, U32, P]),
        "crdt_gcounter_value": (I, [P, P, P, SZ, U32, P]),
        "crdt_pncounter_value": (I, [P, P, P, SZ, U32, P]),
        "crdt_vclock_dense_get": (I, [P, P, C.POINTER(ClockOpsC), P, SZ, U32, P]),
        "crdt_vclock_csr_truncate": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockCsr), C.POINTER(ClockCsrOut), P]),
        "crdt_vclock_csr_subtract": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockCsr), C.POINTER(ClockCsrOut), P]),
        "crdt_vclock_csr_intersection": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockCsr), C.POINTER(ClockCsrOut), P]),
        "crdt_vclock_csr_apply": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockOpsC), C.POINTER(ClockCsrOut), P]),
        "crdt_gcounter_csr_apply": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockOpsC), C.POINTER(ClockCsrOut), P]),
        "crdt_gcounter_csr_value": (I, [P, C.POINTER(ClockCsr), P, P]),
        "crdt_vclock_csr_get": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockOpsC), P, P]),
        "crdt_orswot_read_sizes": (I, [P, BP, C.POINTER(ReadQueriesC), U32, U32, C.POINTER(ReadSizesC), P]),
        "crdt_orswot_read": (I, [P, BP, C.POINTER(ReadQueriesC), U32, U32, C.POINTER(ReadOutC), P]),
        "crdt_map_read_sizes": (I, [P, C.POINTER(MapReadViewC), C.POINTER(ReadQueriesC), SZ, U32,
                                    C.POINTER(ReadSizesC), P]),
        "crdt_map_read": (I, [P, C.POINTER(MapReadViewC), C.POINTER(ReadQueriesC), SZ, U32, C.POINTER(ReadOutC), P]),
        "crdt_map_mvreg_get": (I, [P, C.POINTER(MapSlabC), C.POINTER(ReadQueriesC), SZ, U32, P, P, P, U32, P]),
        "crdt_map_orswot_get_sizes": (I, [P, C.POINTER(MapOrswotSlabC), C.POINTER(ReadQueriesC), SZ, U32, P, P, P]),
        "crdt_map_orswot_get": (I, [P, C.POINTER(MapOrswotSlabC), C.POINTER(ReadQueriesC), SZ, U32, P, P, SZ, P]),
        "crdt_map_map_get": (I, [P, C.POINTER(MapMapSlabC), C.POINTER(ReadQueriesC), SZ, U32, C.POINTER(MapSlabC), P,
                                 P]),
        "crdt_lwwreg_merge": (I, [P, P, P, P, P, SZ, U32, P, P, P]),
        "crdt_lwwreg_apply": (I, [P, P, P, C.POINTER(LWWOpsC), SZ, U32, P, P, P]),
        "crdt_lwwreg_fold": (I, [P, C.POINTER(LWWViewC), U32, SZ, U32, P, P, P, P]),
        "crdt_mvreg_fold": (I, [P, C.POINTER(MVRegViewC), U32, P, P, P, U32, SZ, U32, P]),
        "crdt_lwwreg_from_bincode": (I, [P, P, SZ, SZ, U32, U32, U32, U32, P, P, P]),
        "crdt_lwwreg_to_bincode": (I, [P, P, P, SZ, U32, U32, U32, U32, P, SZ, P]),
        "crdt_clock_dense_from_bincode": (I, [P, P, SZ, P, P, SZ, U32, U32, U32, P, P]),
        "crdt_clock_dense_bincode_sizes": (I, [P, P, SZ, U32, U32, U32, P, P]),
        "crdt_clock_dense_to_bincode": (I, [P, P, SZ, U32, U32, U32, P, P, SZ, P]),
        "crdt_clock_csr_bincode_lens": (I, [P, P, SZ, P, P, SZ, U32, U32, P, P, P]),
        "crdt_clock_csr_from_bincode": (I, [P, P, SZ, P, P, SZ, U32, U32, C.POINTER(ClockCsrOut),
                                            C.POINTER(ClockCsrOut), P]),
        "crdt_clock_csr_bincode_sizes": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockCsr), U32, P, P]),
        "crdt_clock_csr_to_bincode": (I, [P, C.POINTER(ClockCsr), C.POINTER(ClockCsr), U32, P, P, SZ, P]),
        "crdt_clock_ops_from_bincode": (I, [P, P, SZ, SZ, U32, U32, P, P, P, P]),
        "crdt_clock_ops_to_bincode": (I, [P, P, P, P, SZ, U32, U32, P, SZ, P]),
        "crdt_ops_bincode_clk_lens": (I, [P, P, SZ, P, P, SZ, U32, C.POINTER(OpWidthsC), P, P]),
        "crdt_ops_from_bincode": (I, [P, P, SZ, P, P, U32, C.POINTER(OpWidthsC), C.POINTER(OpArraysC), P, P]),
        "crdt_ops_bincode_sizes": (I, [P, U32, C.POINTER(OpWidthsC), C.POINTER(OpArraysC), P, P]),
        "crdt_ops_to_bincode": (I, [P, U32, C.POINTER(OpWidthsC), C.POINTER(OpArraysC), P, P, SZ, P]),
        "crdt_orswot_generate_replicas_subset": (I, [U64, SZ, SZ, C.POINTER(RepParams), U32, U32, U32, U32, I,
                                                     C.POINTER(P)]),
        "crdt_orswot_replica_join_transport": (I, [P, C.POINTER(TransportC), BP, U32, U32, P, P, SZ, C.POINTER(SZ),
                                                   P]),
        "crdt_replica_allreduce_max_transport": (I, [P, C.POINTER(TransportC), P, SZ, P]),
        "crdt_replica_reduce_scatter_max_transport": (I, [P, C.POINTER(TransportC), P, SZ, P, P]),
    }
    for name, (res, args) in sig.items():
        if name in DIAG_SYMBOLS and not hasattr(L, name):
            continue  # product build: diagnostic knobs are not exported
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L


lib = None
lib = _load()


def check(rc, what=""):
    if rc != CRDT_OK:
        raise CrdtError(rc, what)
    return rc
