"""crdts_hip — MI355X batched state-based CRDT merge (host side, Python).

Mirrors the reference's `CvRDT::merge(&mut self, &other)` (src/traits.rs:9-12)
for VClock / GCounter / PNCounter / Orswot, executed on the GPU through the C
ABI of libcrdts_hip.so (include/crdts_hip.h):

    eng = Engine(0)
    out = eng.orswot_merge(self_batch, other_batch)      # batch join on HBM
    a.merge(b)                                           # one pair, same kernel

Device memory and streams come from torch (plumbing only).
"""
from __future__ import annotations

import ctypes as C  # noqa: F401  (C, os and np: names the package has always exposed, kept importable)
import os  # noqa: F401

import numpy as np  # noqa: F401

from ._lib import (CLOCK_FOLD_MAX_REPS, CLOCK_FOLD_STAGE_ENTRIES, CRDT_COMM_ID_BYTES, CRDT_ECAPACITY, CRDT_EINVAL, CRDT_ENONCANON, CRDT_OK, EXPORTS, LIB_PATH, SPARSE_CLOCK, Batch, CrdtError,
                   GenParams, RepParams, check, lib)
from ._util import _nullctx, _torch
from .batches import ClockBatch, OrswotBatch
from .clock_bincode import ClockBincodeEngine
from .engine import Engine
from .generators import (CONFIG3, CONFIG3_SEED, CONFIG5, CONFIG5_SEED, TAIL_SEED, TAIL_SIZES, _copy_sides, _params, _tail_batch,
                         generate_clocks_csr, generate_dense, generate_orswot, generate_orswot_csr_tail, generate_orswot_tail,
                         generate_replicas)
# (_default_engine is the name's value at import, None: the engine default_engine() caches lives in host_model)
from .host_model import (GCounter, HostOrswot, Orswot, PNCounter, VClock, _default_engine, build_record, default_engine,
                         merge_batch)
from .lwwreg import (LWWREG_MAX_REPS, LWWREG_WAVE_MIN_OPS, ConflictingMarker, LWWBatch, LWWEngine, LWWOps, LWWReg)
from .ops import ClockOps, MapMapOps, MapOps, MapOrswotOps, MVRegOps, OrswotOps, ReadQueries
from .ops_bincode import OpsBincodeEngine
from .reads import READ_WANTS
from .record import decode_record, encode_record, record_bytes
from .slabs import MapMapSlab, MapOrswotSlab, MapSlab, _read_view

__all__ = [
    "Engine", "OrswotBatch", "GenParams", "CrdtError", "generate_orswot", "generate_dense", "HostOrswot",
    "Orswot", "VClock", "GCounter", "PNCounter", "merge_batch", "decode_record", "encode_record",
    "record_bytes", "CONFIG3", "EXPORTS", "LIB_PATH", "CONFIG5", "SPARSE_CLOCK", "generate_replicas", "ClockBatch",
    "generate_clocks_csr", "MapMapSlab", "MapOps", "MapMapOps", "MVRegOps", "ClockOps",
    "ReadQueries", "LWWReg", "LWWBatch", "LWWOps", "ConflictingMarker", "LWWREG_WAVE_MIN_OPS", "LWWREG_MAX_REPS",
    "MapSlab", "MapOrswotSlab", "OrswotOps", "MapOrswotOps", "generate_orswot_tail", "generate_orswot_csr_tail",
    "default_engine", "build_record", "CLOCK_FOLD_MAX_REPS", "CLOCK_FOLD_STAGE_ENTRIES",
]
