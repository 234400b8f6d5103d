#!/usr/bin/env python3
"""Timing of the op-stream codec (ops_bincode.hip) beside the apply its ops
feed, in one process.

Op batches (those of the existing apply benches, tiled the same way):
  orswot      bench.py's `apply` workload: 8 ops per config-3 object
  mvreg       tools/mvreg_apply_bench.py: 4 Puts per register, A = 16
  map_mvreg   tools/map_apply_bench.py: the generated Map<u64, MVReg> streams
  map_orswot  tools/map_orswot_apply_bench.py
  map_map     tools/map_map_apply_bench.py
Calls per batch: `lens` (crdt_ops_bincode_clk_lens), `from` (crdt_ops_from_bincode
with the caller's clk_end in place), `sizes`, `to` (egest at packed offsets) and
the yardstick `apply` (the type's crdt_*_apply over the same ops); and, as the
fixed-size reference point, `dots.from`: crdt_clock_ops_from_bincode on
--n-dots Dot blobs. Every call is timed with device events after a warm-up, in
rounds that run each call once in an order drawn anew per round, on
preallocated outputs (the Orswot apply allocates its output from the caching
allocator, outside the events' stream work). Before any time is taken,
ingest(egest(x)) == x is checked on every op and the first 512 blobs are
compared with tests/ops_bincode_ref.py. Each entry gives the median / min / max
time, G ops/s, the bytes the call must move (blob bytes + array bytes) and that
traffic over the median as a fraction of the 8 TB/s HBM peak; "ratios" holds
each call over its batch's apply. There is no gate. One JSON line (also
written to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

HBM_PEAK = 8e12  # bytes/s
SAMPLE = 512
WIDTHS = (4, 8, 8, 8)  # actor, key, key2, val: the generators draw keys above 2^63


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-orswot", type=int, default=1_000_000, help="objects of the Orswot apply workload")
    ap.add_argument("--n-mvreg", type=int, default=4_000_000, help="registers of the MVReg apply bench")
    ap.add_argument("--n-map", type=int, default=200_000, help="objects of each of the three Map apply benches")
    ap.add_argument("--n-dots", type=int, default=8_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import ops_bincode_cases as cases
    import ops_bincode_ref as ref
    from crdts_hip import ops_bincode as ob
    from crdts_hip._lib import OP_ARRAYS_FIELDS, OpArraysC, OpWidthsC, lib

    if not torch.cuda.is_available():
        raise SystemExit("ops_bincode_bench: no GPU visible")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    st = C.c_void_p(s.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    shift = lambda e, step, reps: np.concatenate([e + np.uint64(r * step) for r in range(reps)])  # noqa: E731

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"ops_bincode_bench: {what} returned {rc}")

    def tile_ops(cls, arrays, reps):
        """The packer's host arrays (obj_end first) tiled reps times: ends shifted, the rest repeated."""
        names = ("obj_end",) + ob.LAYOUT[cls.__name__][1]
        a_ = dict(zip(names, arrays))
        step = {"obj_end": len(a_[names[1]]), "clk_end": len(a_["clk_act"])}
        return cls.from_arrays(*[shift(a_[f], step[f], reps) if f in step else np.tile(a_[f], reps) for f in names])

    # ---- the five batches: (ops on the device, apply, objects)
    def orswot():
        import bench

        n = a.n_orswot
        (lb, lo), _ = crdts_hip.generate_orswot(n, threads=8)
        B = crdts_hip.OrswotBatch.from_host(lb, lo, 16)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(  # noqa: E731
            np.int32 if x.dtype == np.uint32 else np.int64)).cuda()
        ops = crdts_hip.OrswotOps(*[t(x) for x in bench._apply_ops(lb, lo, n)])
        return ops, (lambda: eng.orswot_apply(B, ops, stream=s, check_status=False)), n

    def mvreg():
        import mvreg_opgen as mo

        BASE, A, CAP, OUT_CAP, N_OPS, HI = 4000, 16, 4, 8, 4, 3
        reps = max(1, a.n_mvreg // BASE)
        n = reps * BASE
        b = mo.gen_batch(0xBE5C, BASE, A, CAP, HI, N_OPS, N_OPS)

        def dev(x):
            x = np.ascontiguousarray(x)
            t = torch.from_numpy(x.view(np.int32 if x.dtype == np.uint32 else np.int64)).cuda()
            return t.repeat((reps,) + (1,) * (t.dim() - 1)).contiguous()

        dS = tuple(dev(x) for x in mo.slab(b["regs0"], CAP, A))
        ops = tile_ops(crdts_hip.MVRegOps, crdts_hip.MVRegOps.arrays_from_lists(b["ops"]), reps)
        out = (torch.empty(n, dtype=torch.int32, device="cuda"),
               torch.empty((n, OUT_CAP, A), dtype=torch.int64, device="cuda"),
               torch.empty((n, OUT_CAP), dtype=torch.int64, device="cuda"))
        return ops, (lambda: eng.mvreg_apply(dS, ops, A, out=out, stream=s, check_status=False)), n

    def map_mvreg():
        import map_opgen
        import map_slab
        from map_slab import crdts_ref

        BASE, A, IN_CAPS, OUT_CAPS = 2000, 16, (4, 4, 4, 4), (8, 8, 8, 8)
        reps = max(1, a.n_map // BASE)
        batch = map_opgen.gen_batch(0xA991, BASE, A)
        S = crdts_hip.MapSlab.alloc(BASE, A, *IN_CAPS)
        for i, (pre, _) in enumerate(batch):
            m = crdts_ref.Map(crdts_ref.MVReg)
            for op in pre:
                map_opgen.apply_op(m, op)
            map_slab.mvreg_map_to_row(m, S, i, A)
        d = S.to("cuda")
        dS = crdts_hip.MapSlab({f: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous() for f, v in d.a.items()},
                               *IN_CAPS)
        ops = tile_ops(crdts_hip.MapOps, crdts_hip.MapOps.arrays_from_lists([o for _, o in batch]), reps)
        out = crdts_hip.MapSlab.alloc(reps * BASE, A, *OUT_CAPS, device="cuda")
        return ops, (lambda: eng.map_mvreg_apply(dS, ops, A, out=out, stream=s, check_status=False)), reps * BASE

    def map_orswot():
        import map_orswot_opgen as og
        import map_slab

        BASE, A = 2000, 16
        in_caps, out_caps = og.caps(4), og.caps(8)
        reps = max(1, a.n_map // BASE)
        batch = og.gen_batch(0x0A57, BASE, A)
        S = crdts_hip.MapOrswotSlab.alloc(BASE, A, **in_caps)
        for i, (pre, _) in enumerate(batch):
            m = og.new_map()
            for op in pre:
                og.apply_op(m, op)
            map_slab.orswot_map_to_row(m, S, i, A)
        d = S.to("cuda")
        dS = crdts_hip.MapOrswotSlab({f: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()
                                      for f, v in d.a.items()}, S.caps)
        ops = tile_ops(crdts_hip.MapOrswotOps, crdts_hip.MapOrswotOps.arrays_from_lists([o for _, o in batch]), reps)
        out = crdts_hip.MapOrswotSlab.alloc(reps * BASE, A, device="cuda", **out_caps)
        return ops, (lambda: eng.map_orswot_apply(dS, ops, A, out=out, stream=s, check_status=False)), reps * BASE

    def map_map():
        import nested_opgen as ng

        BASE, A = 2000, 16
        reps = max(1, a.n_map // BASE)
        batch, S, _ = ng.reference(0x0A55, BASE, A)
        d = S.to("cuda")
        rep = lambda v: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()  # noqa: E731
        dS = crdts_hip.MapMapSlab({f: rep(v) for f, v in d.a.items()}, S.kcap, S.dcap, S.scap, crdts_hip.MapSlab(
            {f: rep(v) for f, v in d.inner.a.items()}, S.inner.kcap, S.inner.mcap, S.inner.dcap, S.inner.scap))
        ops = tile_ops(crdts_hip.MapMapOps, crdts_hip.MapMapOps.arrays_from_lists([o for _, o in batch]), reps)
        out = crdts_hip.MapMapSlab.alloc(reps * BASE, A, *ng.OUT_CAPS, ng.OUT_INNER, device="cuda")
        return ops, (lambda: eng.map_map_apply(dS, ops, A, out=out, stream=s, check_status=False)), reps * BASE

    calls, models, shapes = {}, {}, {}
    keep = []  # the tensors behind the raw pointers of the OpArraysC structs

    def codec(name, build):
        ops, apply, n_obj = build()
        op_type, fields = ob.LAYOUT[type(ops).__name__]
        cw = OpWidthsC(*WIDTHS)
        arrays = dict(zip(fields, ops.t[1:]))
        n, n_clk = ops.n_ops, ops.n_clk
        blobs, off, lens = eng.ops_to_bincode(op_type, WIDTHS, arrays)
        back = eng.ops_from_bincode(blobs, off, lens, op_type, WIDTHS)
        for f in fields:  # every op, on the device
            if not torch.equal(back[f], arrays[f]):
                raise SystemExit(f"ops_bincode_bench: {name}: ingest(egest(ops)) != ops in {f}")
        k = min(n, SAMPLE)
        h = {f: v[:k].cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint64).tolist()
             for f, v in arrays.items() if f not in ("clk_act", "clk_ctr")}
        kc = h["clk_end"][k - 1] if k else 0
        pa = arrays["clk_act"][:kc].cpu().numpy().view(np.uint32).tolist()
        pc = arrays["clk_ctr"][:kc].cpu().numpy().view(np.uint64).tolist()
        ho, hl = off[:k].cpu().tolist(), lens[:k].cpu().tolist()
        hb = blobs[:ho[-1] + hl[-1] if k else 0].cpu().numpy()  # packed back to back: the sample is a prefix
        g = lambda f, j: h[f][j] if f in h else 0  # noqa: E731
        for j in range(k):
            b0 = h["clk_end"][j - 1] if j else 0
            op = cases.make_op(op_type, g("kind", j), (g("actor", j), g("counter", j)), g("key", j), g("key2", j),
                               (g("actor2", j), g("counter2", j)), g("val", j),
                               list(zip(pa[b0:h["clk_end"][j]], pc[b0:h["clk_end"][j]])))
            if hb[ho[j]:ho[j] + hl[j]].tobytes() != ref.encode(op_type, op, WIDTHS):
                raise SystemExit(f"ops_bincode_bench: {name}: op blob {j} differs from the restatement")
        blob_bytes, nb = int(lens.sum().item()), int(blobs.numel())
        array_bytes = sum(v.numel() * v.element_size() for v in arrays.values())
        out = dict(back)  # the ingest's preallocated outputs; clk_end stays the scan's
        ca_out = OpArraysC(*[p(out.get(f)) for f in OP_ARRAYS_FIELDS], n, n_clk)
        ca_in = OpArraysC(*[p(arrays.get(f)) for f in OP_ARRAYS_FIELDS], n, n_clk)
        keep.append((out, arrays))
        len_out = torch.empty(n, dtype=torch.int32, device="cuda")
        sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        calls[name + ".lens"] = lambda: ok(lib.crdt_ops_bincode_clk_lens(
            eng.ctx, p(blobs), nb, p(off), p(lens), n, op_type, C.byref(cw), p(len_out), st), name + " lens")
        calls[name + ".from"] = lambda: ok(lib.crdt_ops_from_bincode(
            eng.ctx, p(blobs), nb, p(off), p(lens), op_type, C.byref(cw), C.byref(ca_out), None, st), name + " from")
        calls[name + ".sizes"] = lambda: ok(lib.crdt_ops_bincode_sizes(
            eng.ctx, op_type, C.byref(cw), C.byref(ca_in), p(sizes), st), name + " sizes")
        calls[name + ".to"] = lambda: ok(lib.crdt_ops_to_bincode(
            eng.ctx, op_type, C.byref(cw), C.byref(ca_in), p(blobs), p(off), nb, st), name + " to")
        calls[name + ".apply"] = apply
        models[name + ".lens"] = blob_bytes + 20 * n
        models[name + ".from"] = blob_bytes + 16 * n + array_bytes
        models[name + ".sizes"] = array_bytes + 8 * n
        models[name + ".to"] = array_bytes + 8 * n + blob_bytes
        models[name + ".apply"] = None  # the apply benches model their own traffic
        shapes[name] = {"ops": n, "objects": n_obj, "clock_pairs": n_clk, "blob_bytes": blob_bytes,
                        "array_bytes": array_bytes, "bytes_per_op": round(blob_bytes / max(n, 1), 2)}

    for name, build in (("orswot", orswot), ("mvreg", mvreg), ("map_mvreg", map_mvreg), ("map_orswot", map_orswot),
                        ("map_map", map_map)):
        codec(name, build)

    # ---- the fixed-size reference point: Dot blobs
    m = a.n_dots
    rng = np.random.default_rng(0x0B5)
    dots = crdts_hip.ClockOps.from_arrays(np.array([m], np.uint64),
                                          rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32),
                                          rng.integers(1, 1 << 40, m, dtype=np.uint64))
    dblob = dots.to_bincode(4, engine=eng)
    da, dc = torch.empty_like(dots.t[1]), torch.empty_like(dots.t[2])
    calls["dots.from"] = lambda: ok(lib.crdt_clock_ops_from_bincode(eng.ctx, p(dblob), 12, m, 4, 0, p(da), p(dc), None,
                                                                    st), "dots from")
    models["dots.from"] = 24 * m
    shapes["dots"] = {"ops": m, "blob_bytes": 12 * m, "array_bytes": 12 * m}

    # ---- timing
    torch.cuda.synchronize()
    eng.status()  # raises for a status latched by the checks above
    t = {k: [] for k in calls}
    order = np.random.default_rng(0x0DE5)
    for r in range(a.warmup + a.rounds):
        for k in order.permutation(list(calls)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                calls[k]()
                e1.record(s)
            s.synchronize()
            ok(lib.crdt_ctx_status(eng.ctx, st), f"the status after {k}")
            if r >= a.warmup:
                t[k].append(e0.elapsed_time(e1))

    res = {"tool": "ops_bincode_bench", "rounds": a.rounds, "warmup": a.warmup, "hbm_peak_TB_per_s": HBM_PEAK / 1e12,
           "widths": dict(zip(ob.WIDTH_NAMES, WIDTHS)), "parity": "unpinned by reference output", "gate": None,
           "traffic_model": "blob bytes + array bytes (lens: the blobs + off / len / lens; the apply: not modelled "
                            "here)",
           "shapes": shapes, "calls": {}, "ratios": {}}
    med = {}
    for k, ms in t.items():
        med[k] = float(np.median(ms))
        n_ops = shapes[k.split(".")[0]]["ops"]
        e = {"median_ms": round(med[k], 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
             "G_ops_per_s": round(n_ops / med[k] / 1e6, 3),
             "spread_over_median": [round(float(np.min(ms)) / med[k], 3), round(float(np.max(ms)) / med[k], 3)]}
        if models[k] is not None:
            e["bytes"] = int(models[k])
            e["fraction_of_hbm_peak"] = round(models[k] / (med[k] * 1e-3) / HBM_PEAK, 4)
        res["calls"][k] = e
    for k in med:
        shape, call = k.split(".")
        if call != "apply" and shape + ".apply" in med:
            res["ratios"][k + "_over_apply"] = round(med[k] / med[shape + ".apply"], 3)
    for shape in shapes:
        if shape + ".apply" in med:
            res["ratios"][shape + ".lens_plus_from_over_apply"] = round(
                (med[shape + ".lens"] + med[shape + ".from"]) / med[shape + ".apply"], 3)
            res["ratios"][shape + ".from_ops_per_s_over_dots"] = round(
                (shapes[shape]["ops"] / med[shape + ".from"]) / (m / med["dots.from"]), 3)
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
