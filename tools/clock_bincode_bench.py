#!/usr/bin/env python3
"""Timing of the clocks' bincode codec (clock_bincode.hip) beside the merge of
the same objects, in one process.

Shapes (--n objects, --n-ops ops):
  dense16_ab1 / dense16_ab8   --n rows of 16 actors (bench config 1's shape),
                              actor_bytes 1 and 8
  dense64_ab8                 --n rows of 64 actors
  csr_ab2                     --n sparse clocks of generate_clocks_csr (the
                              clock_csr workload: ~48 of a 1024-actor universe)
  dot_ab4 / pnop_ab4          --n-ops Dot blobs / PNCounter Op blobs
Calls per shape: `from` (ingest; CSR: with the caller's offsets in place),
`lens` (CSR framing pass), `sizes` and `to` (egest at packed offsets), and the
yardstick `merge` (crdt_vclock_dense_merge / crdt_vclock_csr_merge of the same
objects). Every call is timed with device events after a warm-up, in rounds
that run each call once in an order drawn anew per round, on preallocated
outputs. Before any time is printed, ingest(egest(x)) == x is checked on every
object and the first blobs are compared with tests/clock_bincode_ref.py.
Each entry gives the median / min / max time, objects per second, the bytes the
call must move (blob bytes + row or run bytes) and that traffic over the
median as a fraction of the 8 TB/s HBM peak; "ratios" holds each call over its
shape's merge. One JSON line (also written to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK = 8e12  # bytes/s
SAMPLE = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--n-ops", type=int, default=8_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import clock_bincode_ref as ref
    import crdts_hip
    from crdts_hip._lib import ClockCsrOut, lib

    if not torch.cuda.is_available():
        raise SystemExit("clock_bincode_bench: no GPU visible")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    st = C.c_void_p(s.cuda_stream)
    n = a.n
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()  # noqa: E731

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"clock_bincode_bench: {what} returned {rc}")

    calls, models, shapes = {}, {}, {}

    # ---- dense rows
    def dense(name, A, ab):
        rows_h = crdts_hip.generate_dense(n, A, seed=A + ab)
        rows, other = dev(rows_h), dev(crdts_hip.generate_dense(n, A, seed=A + ab + 100))
        blobs, off, lens = eng.clock_to_bincode(rows, A, ab, "vclock")
        back = eng.clock_from_bincode(blobs, off, lens, A, ab, "vclock")
        if not (u64(back).reshape(n, A) == rows_h).all():
            raise SystemExit(f"clock_bincode_bench: {name}: ingest(egest(rows)) != rows")
        hb, ho, hl = blobs.cpu().numpy().tobytes(), off.cpu().tolist(), lens.cpu().tolist()
        for i in range(min(n, SAMPLE)):
            if hb[ho[i]:ho[i] + hl[i]] != ref.encode_state(ref.row_state(rows_h[i], A), ab):
                raise SystemExit(f"clock_bincode_bench: {name}: blob {i} differs from the restatement")
        blob_bytes, row_bytes = int(lens.sum().item()), 8 * A * n
        sizes = torch.empty_like(lens)
        nb = int(blobs.numel())
        calls[name + ".from"] = lambda: ok(lib.crdt_clock_dense_from_bincode(
            eng.ctx, p(blobs), nb, p(off), p(lens), n, ab, A, 1, p(back), st), name)
        calls[name + ".sizes"] = lambda: ok(lib.crdt_clock_dense_bincode_sizes(
            eng.ctx, p(rows), n, A, 1, ab, p(sizes), st), name)
        calls[name + ".to"] = lambda: ok(lib.crdt_clock_dense_to_bincode(
            eng.ctx, p(rows), n, A, 1, ab, p(blobs), p(off), nb, st), name)
        calls[name + ".merge"] = lambda: eng.dense_merge(other, rows, A, "vclock", stream=s)
        models[name + ".from"] = models[name + ".to"] = blob_bytes + row_bytes
        models[name + ".sizes"] = row_bytes + 8 * n
        models[name + ".merge"] = 3 * row_bytes
        shapes[name] = {"objects": n, "n_actors": A, "actor_bytes": ab, "blob_bytes": blob_bytes,
                        "row_bytes": row_bytes}

    dense("dense16_ab1", 16, 1)
    dense("dense16_ab8", 16, 8)
    dense("dense64_ab8", 64, 8)

    # ---- CSR runs
    hs, ho_ = crdts_hip.generate_clocks_csr(n, seed=0xC5)
    S, O = crdts_hip.ClockBatch.from_host(*hs), crdts_hip.ClockBatch.from_host(*ho_)
    ab = 2
    blobs, off, lens = eng.clock_csr_to_bincode(S, ab)
    back = eng.clock_csr_from_bincode(blobs, off, lens, ab)
    bo, bl, ba, bc = back.to_host()
    if not ((bo == hs[0]).all() and (bl == hs[1]).all() and (ba[:hs[2].size] == hs[2]).all()
            and (bc[:hs[3].size] == hs[3]).all()):
        raise SystemExit("clock_bincode_bench: csr: ingest(egest(runs)) != runs")
    hb, hof, hl = blobs.cpu().numpy().tobytes(), off.cpu().tolist(), lens.cpu().tolist()
    k = min(n, SAMPLE)
    runs = [list(zip(hs[2][o:o + ln].tolist(), hs[3][o:o + ln].tolist()))
            for o, ln in zip(hs[0][:k].tolist(), hs[1][:k].tolist())]
    for i, run in enumerate(runs):
        if hb[hof[i]:hof[i] + hl[i]] != ref.encode_state([run], ab):
            raise SystemExit(f"clock_bincode_bench: csr: blob {i} differs from the restatement")
    entries, blob_bytes = int(hs[1].sum()), int(lens.sum().item())
    run_bytes = 12 * entries + 12 * n
    w = ClockCsrOut(p(back.off), p(back.len), p(back.act), p(back.ctr), back.n_entries)
    sp, nb = S.cstruct(), int(blobs.numel())
    len_out, sizes = torch.empty_like(back.len), torch.empty_like(lens)
    merged = eng.clock_csr_alloc_out(S, O)
    calls["csr_ab2.lens"] = lambda: ok(lib.crdt_clock_csr_bincode_lens(
        eng.ctx, p(blobs), nb, p(off), p(lens), n, ab, 1, p(len_out), None, st), "csr lens")
    calls["csr_ab2.from"] = lambda: ok(lib.crdt_clock_csr_from_bincode(
        eng.ctx, p(blobs), nb, p(off), p(lens), n, ab, 1, C.byref(w), None, st), "csr from")
    calls["csr_ab2.sizes"] = lambda: ok(lib.crdt_clock_csr_bincode_sizes(
        eng.ctx, C.byref(sp), None, ab, p(sizes), st), "csr sizes")
    calls["csr_ab2.to"] = lambda: ok(lib.crdt_clock_csr_to_bincode(
        eng.ctx, C.byref(sp), None, ab, p(blobs), p(off), nb, st), "csr to")
    calls["csr_ab2.merge"] = lambda: eng.clock_csr_merge(S, O, out=merged, stream=s, check_status=False)
    models["csr_ab2.lens"] = 24 * n + 4 * n
    models["csr_ab2.from"] = models["csr_ab2.to"] = blob_bytes + run_bytes
    models["csr_ab2.sizes"] = run_bytes + 8 * n
    models["csr_ab2.merge"] = run_bytes + 12 * int(ho_[1].sum()) + 12 * n + 12 * entries + 12 * n
    shapes["csr_ab2"] = {"objects": n, "universe": 1024, "actor_bytes": ab, "entries": entries,
                         "blob_bytes": blob_bytes, "run_bytes": run_bytes,
                         "merge_traffic_model": "both inputs' runs read, an output of self's size written"}

    # ---- ops
    m = a.n_ops
    rng = np.random.default_rng(0x0B5)
    act = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    ctr = rng.integers(1, 1 << 40, m, dtype=np.uint64)
    dr = rng.integers(0, 2, m, dtype=np.uint64).astype(np.uint32)
    for name, wd in (("dot_ab4", False), ("pnop_ab4", True)):
        ops = crdts_hip.ClockOps.from_arrays(np.array([m], np.uint64), act, ctr, dr if wd else None)
        size = 4 + 8 + (4 if wd else 0)
        ob = ops.to_bincode(4, engine=eng)
        got = crdts_hip.ClockOps.from_bincode(ob, None, ops.t[0], 4, wd, engine=eng)
        if not ((got.t[1].cpu().numpy().view(np.uint32) == act).all() and (u64(got.t[2]) == ctr).all()
                and (not wd or (got.t[3].cpu().numpy().view(np.uint32) == dr).all())):
            raise SystemExit(f"clock_bincode_bench: {name}: ingest(egest(ops)) != ops")
        hob = ob[:size * SAMPLE].cpu().numpy().tobytes()
        for j in range(min(m, SAMPLE)):
            if hob[j * size:(j + 1) * size] != ref.encode_op(int(act[j]), int(ctr[j]), 4, int(dr[j]) if wd else None):
                raise SystemExit(f"clock_bincode_bench: {name}: op blob {j} differs from the restatement")
        _, ta, tc, td = ops.t
        _, ga, gc, gd = got.t
        pd, pgd = (p(td), p(gd)) if wd else (None, None)
        calls[name + ".from"] = (lambda ob=ob, size=size, wd=wd, ga=ga, gc=gc, pgd=pgd, name=name: ok(
            lib.crdt_clock_ops_from_bincode(eng.ctx, p(ob), size, m, 4, int(wd), p(ga), p(gc), pgd, st), name))
        calls[name + ".to"] = (lambda ob=ob, size=size, wd=wd, ta=ta, tc=tc, pd=pd, name=name: ok(
            lib.crdt_clock_ops_to_bincode(eng.ctx, p(ta), p(tc), pd, m, 4, int(wd), p(ob), size, st), name))
        models[name + ".from"] = models[name + ".to"] = (size + 12 + (4 if wd else 0)) * m
        shapes[name] = {"objects": m, "actor_bytes": 4, "blob_bytes": size * m}

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
            if r >= a.warmup:
                t[k].append(e0.elapsed_time(e1))
    eng.status(s)

    res = {"tool": "clock_bincode_bench", "rounds": a.rounds, "warmup": a.warmup, "hbm_peak_TB_per_s": HBM_PEAK / 1e12,
           "parity": "unpinned by reference output", "traffic_model": "blob bytes + row or run bytes",
           "shapes": shapes, "calls": {}, "ratios": {}}
    med = {}
    for k, ms in t.items():
        med[k] = float(np.median(ms))
        objs = shapes[k.split(".")[0]]["objects"]
        res["calls"][k] = {"median_ms": round(med[k], 4), "min_ms": round(float(np.min(ms)), 4),
                           "max_ms": round(float(np.max(ms)), 4), "M_objects_per_s": round(objs / med[k] / 1e3, 2),
                           "spread_over_median": [round(float(np.min(ms)) / med[k], 3),
                                                  round(float(np.max(ms)) / med[k], 3)],
                           "bytes": int(models[k]),
                           "fraction_of_hbm_peak": round(models[k] / (med[k] * 1e-3) / HBM_PEAK, 4)}
    for k in med:
        shape, call = k.split(".")
        if call != "merge" and shape + ".merge" in med:
            res["ratios"][k + "_over_merge"] = round(med[k] / med[shape + ".merge"], 3)
    for shape in shapes:
        if shape + ".merge" in med:
            res["ratios"][shape + ".sizes_plus_to_over_merge"] = round(
                (med[shape + ".sizes"] + med[shape + ".to"]) / med[shape + ".merge"], 3)
            res["ratios"][shape + ".merge_spread_over_median"] = res["calls"][shape + ".merge"]["spread_over_median"]
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
