"""The reference's LWWReg restated in plain Python, sequential semantics only
(etsangsplk/rust-crdt src/lwwreg.rs). Independent of crdts_hip's host mirror:
a register is a (val, marker) tuple, a marker an int or a tuple of ints
(Python tuple order is Rust tuple `Ord`), a Result is True for
Err(ConflictingMarker) and False for Ok(())."""


def default():
    """Default for LWWReg<u64, u64> (src/lwwreg.rs:34-41)."""
    return (0, 0)


def merge(reg, other):
    """FunkyCvRDT::merge (src/lwwreg.rs:56-66) -> (new reg, err)."""
    val, marker = reg
    oval, omarker = other
    if omarker > marker:  # :57-60
        return (oval, omarker), False
    if omarker == marker and oval != val:  # :61-62
        return reg, True
    return reg, False  # :63-65


def apply(reg, op):
    """FunkyCmRDT::apply (src/lwwreg.rs:74-76): the op is a whole register."""
    return merge(reg, op)


def update(reg, val, marker):
    """LWWReg::update (src/lwwreg.rs:104-118) -> (new reg, err)."""
    cval, cmarker = reg
    if cmarker < marker:  # :105-108
        return (val, marker), False
    if cmarker == marker and val != cval:  # :109-110
        return reg, True
    return reg, False  # :111-117


def apply_list(reg, ops):
    """ops in order: an erring op changes nothing, later ops still apply.
    -> (final reg, [err per op])."""
    errs = []
    for op in ops:
        reg, e = apply(reg, op)
        errs.append(e)
    return reg, errs


def fold(regs):
    """regs[0].merge(regs[1]).merge(regs[2])... -> (reg, erring merges)."""
    acc, n = regs[0], 0
    for r in regs[1:]:
        acc, e = merge(acc, r)
        n += e
    return acc, n


def to_binary(reg, val_bytes, marker_bytes):
    """bincode of the struct's fields in order (src/lwwreg.rs:27-32): val, then
    the marker words, each fixed-width little-endian."""
    val, marker = reg
    words = marker if isinstance(marker, tuple) else (marker,)
    widths = marker_bytes if isinstance(marker_bytes, tuple) else (marker_bytes,)
    out = val.to_bytes(val_bytes, "little")
    for w, b in zip(words, widths):
        out += w.to_bytes(b, "little")
    return out
