"""Host plumbing shared by the package's modules: torch on demand, the
numpy <-> torch views of u32 / u64 arrays, and the pointer a tensor crosses
the C ABI as."""
from __future__ import annotations

import ctypes as C

import numpy as np


def _torch():
    import torch

    return torch


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def on_stream(stream):
    """The context torch work of a call runs in: the caller's stream, or the current one."""
    return _torch().cuda.stream(stream) if stream is not None else _nullctx()


def dptr(t):
    """The pointer of a tensor the ABI requires (an array that is never optional)."""
    return C.c_void_p(t.data_ptr())


def ptr(t):
    """The pointer of an array the ABI lets be absent: NULL for None and for an empty tensor."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def put(x, u32, device):
    """A host array as u32 / u64 -> an int32 / int64 tensor of the same bits
    on cuda:<device> (None: it stays on the host); None stays None."""
    if x is None:
        return None
    x = np.ascontiguousarray(np.asarray(x, dtype=np.uint32 if u32 else np.uint64))
    t = _torch().from_numpy(x.view(np.int32 if u32 else np.int64))
    return t if device is None else t.to(f"cuda:{device}")


def longest_op_list(obj_end):
    """The longest per-object op list of a host obj_end array (u64 inclusive
    ends). A decreasing obj_end is the kernel's to reject: its wrapped
    difference only sizes a default output."""
    ends = np.asarray(obj_end, dtype=np.uint64)
    return int(np.diff(ends, prepend=np.uint64(0)).max()) if ends.size else 0
