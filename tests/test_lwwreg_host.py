"""CPU: LWWReg's ABI surface, host mirror, containers and argument checks
(include/crdts_hip.h "LWWReg<u64, M>, batched"; reference src/lwwreg.rs).

No device work: the argument checks are made before any device call, so they
are exercised with a null context and with a zeroed stand-in for one."""
import ctypes as C
import json
import os
import sys

import pytest

import lwwreg_cases as cases
import lwwreg_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crdt_lwwreg_merge", "crdt_lwwreg_apply", "crdt_lwwreg_fold", "crdt_lwwreg_from_bincode",
       "crdt_lwwreg_to_bincode")


def _kats():
    with open(os.path.join(REPO, "tests", "golden", "kat_lwwreg.json")) as f:
        return json.load(f)


def _r(d):
    return (d["val"], d["marker"])


# ------------------------------------------------------------------- surface
def test_new_functions_are_declared_exported_and_typed():
    import crdts_hip
    from crdts_hip._lib import lib

    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_ffi_rs

    header = {name: len(args) for name, _, args in gen_ffi_rs.parse_header()}
    for name in NEW:
        assert name in header, name
        assert name in crdts_hip.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == header[name], name
        assert fn.restype is C.c_int


def test_tier_constant_matches_the_header():
    import re

    import crdts_hip

    src = open(os.path.join(REPO, "include", "crdts_hip.h")).read()
    assert int(re.search(r"#define CRDT_LWWREG_WAVE_MIN_OPS (\d+)", src).group(1)) == crdts_hip.LWWREG_WAVE_MIN_OPS
    assert int(re.search(r"#define CRDT_LWWREG_MAX_REPS (\d+)", src).group(1)) == crdts_hip.LWWREG_MAX_REPS == 32
    assert 2 <= crdts_hip.LWWREG_WAVE_MIN_OPS <= 64


# ---------------------------------------------------------------------- KATs
def _run_script(script, step):
    """step(state, val, marker) -> (state, err); checks every step of a KAT script."""
    s = _r(script["start"])
    for st in script["steps"]:
        s, err = step(s, st["update"]["val"], st["update"]["marker"])
        assert err == (not st["ok"]), st
        assert s == _r(st["state"]), st


def _mirror_update(s, val, marker):
    import crdts_hip

    reg = crdts_hip.LWWReg(*s)
    try:
        reg.update(val, marker)
        err = False
    except crdts_hip.ConflictingMarker:
        err = True
    return (reg.val, reg.marker), err


def test_reference_restatement_reproduces_the_kats():
    k = _kats()
    assert ref.default() == _r(k["test_default"])
    _run_script(k["test_update"], ref.update)
    _run_script(k["update_doctest"], ref.update)
    m = k["merge_doctest"]
    assert ref.merge(_r(m["self"]), _r(m["other"])) == (_r(m["state"]), not m["ok"])


def test_mirror_reproduces_the_kats():
    import crdts_hip

    k = _kats()
    d = crdts_hip.LWWReg()
    assert (d.val, d.marker) == _r(k["test_default"])
    _run_script(k["test_update"], _mirror_update)
    _run_script(k["update_doctest"], _mirror_update)
    m = k["merge_doctest"]
    a, b = crdts_hip.LWWReg(*_r(m["self"])), crdts_hip.LWWReg(*_r(m["other"]))
    with pytest.raises(crdts_hip.ConflictingMarker):
        a.merge(b)
    assert a == crdts_hip.LWWReg(*_r(m["state"]))
    with pytest.raises(crdts_hip.ConflictingMarker):
        a.apply(b)
    assert a == crdts_hip.LWWReg(*_r(m["state"]))


# ------------------------------------------------------- random op lists
@pytest.mark.parametrize("marker_words", [1, 2])
def test_mirror_and_closed_form_equal_the_reference_on_random_lists(marker_words):
    import crdts_hip

    n_err = n_noop = 0
    for start, ops in cases.rnd_lists(0x11E6 + marker_words, 2000, marker_words):
        exp, exp_errs = ref.apply_list(start, ops)
        reg, errs = crdts_hip.LWWReg(*start), []
        for i, (v, m) in enumerate(ops):
            before = (reg.val, reg.marker)
            try:  # the three entry points in turn: they are one rule
                if i % 3 == 0:
                    reg.update(v, m)
                elif i % 3 == 1:
                    reg.merge(crdts_hip.LWWReg(v, m))
                else:
                    reg.apply(crdts_hip.LWWReg(v, m))
                errs.append(False)
            except crdts_hip.ConflictingMarker:
                errs.append(True)
                assert (reg.val, reg.marker) == before  # an Err leaves the state
            n_noop += (not errs[-1]) and before == (v, m)
        n_err += sum(errs)
        assert ((reg.val, reg.marker), errs) == (exp, exp_errs)
        assert cases.closed_form(start, ops) == (exp, exp_errs)
    assert n_err >= 1 and n_noop >= 1  # the alphabets are small enough to meet both


# ------------------------------------------------------------- containers
def test_batch_and_ops_pack_the_header_layout():
    import crdts_hip

    big = (1 << 64) - 1
    B = crdts_hip.LWWBatch.from_lists([(5, 9), (big, big), crdts_hip.LWWReg(1, 0)], device=None)
    assert (B.n, B.marker_words) == (3, 1)
    assert B.val.dtype == B.marker.dtype and str(B.val.dtype) == "torch.int64"
    assert tuple(B.marker.shape) == (3, 1) and B.marker.is_contiguous()
    v, m = B.to_host()
    assert v.tolist() == [5, big, 1] and m.ravel().tolist() == [9, big, 0]
    assert B.to_lists() == [(5, 9), (big, big), (1, 0)]
    B2 = crdts_hip.LWWBatch.from_lists([(5, (1, 2)), (6, (big, 0))], marker_words=2, device=None)
    # row-major [n][marker_words]
    assert B2.to_host()[1].ravel().tolist() == [1, 2, big, 0]
    assert B2.to_lists() == [(5, (1, 2)), (6, (big, 0))]
    with pytest.raises(crdts_hip.CrdtError):
        crdts_hip.LWWBatch.from_lists([(5, (1, 2))], marker_words=1, device=None)
    E = crdts_hip.LWWBatch.from_lists([], marker_words=2, device=None)
    assert E.n == 0 and E.to_lists() == []

    ops = crdts_hip.LWWOps.from_lists([[(1, (2, 3))], [], [(4, (5, 6)), (7, (8, 9))]], marker_words=2, device=None)
    assert (ops.n_obj, ops.n_ops, ops.marker_words) == (3, 3, 2)
    ends, val, mk = ops.host
    assert ends.tolist() == [1, 1, 3] and val.tolist() == [1, 4, 7]
    assert mk.ravel().tolist() == [2, 3, 5, 6, 8, 9]
    c = ops.cops()
    assert c.n_ops == 3 and c.obj_end == ops.obj_end.data_ptr() and c.marker == ops.marker.data_ptr()
    e = crdts_hip.LWWOps.from_lists([[], []], device=None).cops()
    assert e.n_ops == 0 and e.val is None and e.marker is None and e.obj_end is not None


# --------------------------------------------------------- argument checks
A, B_, C_, D_, E_ = (C.c_void_p(0x1000 * k) for k in range(1, 6))  # never dereferenced: every case returns first


def _contexts():
    """A null context, and a zeroed stand-in for one (the checks come before
    the first use of the context)."""
    return [None, C.cast(C.create_string_buffer(4096), C.c_void_p)]


def test_merge_argument_checks():
    from crdts_hip._lib import lib

    f = lib.crdt_lwwreg_merge
    assert f(None, A, B_, C_, D_, 4, 1, None, None, None) == -1
    assert f(None, None, None, None, None, 0, 1, None, None, None) == -1
    ctx = _contexts()[1]
    for k in range(4):  # a null required array with n > 0
        p = [A, B_, C_, D_]
        p[k] = None
        assert f(ctx, *p, 4, 1, None, None, None) == -1
    for mw in (0, 3):
        assert f(ctx, A, B_, C_, D_, 4, mw, None, None, None) == -1
        assert f(ctx, None, None, None, None, 0, mw, None, None, None) == -1
    assert f(ctx, A, B_, A, D_, 4, 1, None, None, None) == -1  # self == other
    assert f(ctx, A, B_, C_, B_, 4, 2, None, None, None) == -1
    assert f(ctx, None, None, None, None, 0, 1, None, None, None) == 0  # n == 0: nothing to do
    assert f(ctx, None, None, None, None, 0, 2, E_, E_, None) == 0


def test_apply_argument_checks():
    from crdts_hip._lib import LWWOpsC, lib

    f = lib.crdt_lwwreg_apply
    ops = LWWOpsC(C_, D_, E_, 5)
    for ctx in _contexts():
        assert f(ctx, A, B_, None, 2, 1, C_, None, None) == -1  # a null ops struct
        assert f(ctx, A, B_, None, 0, 1, C_, None, None) == -1
    assert f(None, A, B_, C.byref(ops), 2, 1, C.c_void_p(0x9000), None, None) == -1
    ctx = _contexts()[1]
    n_err = C.c_void_p(0x9000)
    assert f(ctx, None, B_, C.byref(ops), 2, 1, n_err, None, None) == -1
    assert f(ctx, A, None, C.byref(ops), 2, 1, n_err, None, None) == -1
    assert f(ctx, A, B_, C.byref(ops), 2, 1, None, None, None) == -1  # d_n_err is required
    assert f(ctx, A, B_, C.byref(ops), 2, 3, n_err, None, None) == -1
    assert f(ctx, A, B_, C.byref(ops), 2, 0, n_err, None, None) == -1
    for bad in (LWWOpsC(None, D_, E_, 5), LWWOpsC(C_, None, E_, 5), LWWOpsC(C_, D_, None, 5)):
        assert f(ctx, A, B_, C.byref(bad), 2, 1, n_err, None, None) == -1
    assert f(ctx, None, None, C.byref(LWWOpsC(None, None, E_, 5)), 0, 1, None, None, None) == -1  # count says non-empty
    for alias in (LWWOpsC(A, D_, E_, 5), LWWOpsC(C_, A, E_, 5), LWWOpsC(C_, D_, B_, 5), LWWOpsC(C_, B_, E_, 5)):
        assert f(ctx, A, B_, C.byref(alias), 2, 1, n_err, None, None) == -1  # an op array is a state array
    assert f(ctx, None, None, C.byref(LWWOpsC(None, None, None, 0)), 0, 1, None, None, None) == 0


def test_fold_argument_checks():
    from crdts_hip._lib import LWWViewC, lib

    f = lib.crdt_lwwreg_fold
    two = (LWWViewC * 2)(LWWViewC(A, B_), LWWViewC(C_, D_))
    out_v, out_m = C.c_void_p(0x8000), C.c_void_p(0x9000)
    assert f(None, two, 2, 4, 1, out_v, out_m, None, None) == -1
    ctx = _contexts()[1]
    assert f(ctx, None, 2, 4, 1, out_v, out_m, None, None) == -1
    many = (LWWViewC * 33)(*[LWWViewC(0x100000 + 0x100 * k, 0x200000 + 0x100 * k) for k in range(33)])
    for n_reps in (0, 33):
        assert f(ctx, many, n_reps, 4, 1, out_v, out_m, None, None) == -1
        assert f(ctx, many, n_reps, 0, 1, None, None, None, None) == -1
    assert f(ctx, two, 2, 4, 3, out_v, out_m, None, None) == -1
    assert f(ctx, two, 2, 4, 1, None, out_m, None, None) == -1
    assert f(ctx, two, 2, 4, 1, out_v, None, None, None) == -1
    for hole in ((LWWViewC * 2)(LWWViewC(A, B_), LWWViewC(None, D_)), (LWWViewC * 2)(LWWViewC(A, None), LWWViewC(C_, D_))):
        assert f(ctx, hole, 2, 4, 1, out_v, out_m, None, None) == -1  # a null view pointer
    assert f(ctx, two, 2, 4, 1, C_, out_m, None, None) == -1  # out is replica 1
    assert f(ctx, two, 2, 4, 2, out_v, D_, None, None) == -1
    assert f(ctx, two, 2, 0, 1, None, None, None, None) == 0
    assert f(ctx, many, 32, 0, 2, None, None, None, None) == 0


def test_bincode_argument_checks():
    from crdts_hip._lib import lib

    fi, fo = lib.crdt_lwwreg_from_bincode, lib.crdt_lwwreg_to_bincode
    assert fi(None, A, 16, 4, 8, 1, 8, 8, B_, C_, None) == -1
    assert fo(None, B_, C_, 4, 8, 1, 8, 8, A, 16, None) == -1
    ctx = _contexts()[1]

    def both(vb, mw, mb0, mb1, stride, n=4, blobs=A, val=B_, marker=C_):
        return (fi(ctx, blobs, stride, n, vb, mw, mb0, mb1, val, marker, None),
                fo(ctx, val, marker, n, vb, mw, mb0, mb1, blobs, stride, None))

    for w in (0, 3, 5, 16):  # a byte width outside {1, 2, 4, 8}
        assert both(w, 1, 8, 8, 64) == (-1, -1)
        assert both(8, 1, w, 8, 64) == (-1, -1)
        assert both(8, 2, 8, w, 64) == (-1, -1)
        assert both(w, 1, 8, 8, 64, n=0) == (-1, -1)
    for mw in (0, 3):
        assert both(8, mw, 8, 8, 64) == (-1, -1)
    assert both(8, 1, 8, 3, 16, n=0) == (0, 0)  # the second width is not read with one marker word
    assert both(1, 2, 2, 1, 3) == (-1, -1)  # stride below the 4-byte blob
    assert both(8, 1, 8, 8, 15) == (-1, -1)
    assert both(8, 1, 8, 8, 16, blobs=None) == (-1, -1)
    assert both(8, 1, 8, 8, 16, val=None) == (-1, -1)
    assert both(8, 1, 8, 8, 16, marker=None) == (-1, -1)
    assert both(8, 1, 8, 8, 16, blobs=B_) == (-1, -1)  # blobs alias a state array
    assert both(1, 2, 2, 1, 4, n=0, blobs=None, val=None, marker=None) == (0, 0)


def test_engine_methods_exist():
    import crdts_hip

    for name in ("lwwreg_merge", "lwwreg_apply", "lwwreg_fold", "lwwreg_from_bincode", "lwwreg_to_bincode"):
        assert callable(getattr(crdts_hip.Engine, name)), name
