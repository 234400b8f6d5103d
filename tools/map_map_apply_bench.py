#!/usr/bin/env python3
"""Timing of the batched Map<u64, Map<u64, MVReg>>::apply (crdt_map_map_apply)
beside the merge of the same maps (crdt_map_map_merge) — the only other way
to bring a remote change into a device-resident nested map.

The 2,000-object generated batch of the tests (tests/nested_opgen.py, A = 16)
is tiled to --n-obj objects on the device. Both calls are timed with device
events after a warm-up, alternating, on preallocated outputs; the merge takes
the same `self` rows against partners of the same size (the rows shifted by
one object). The apply's first and last tile are checked against the Python
restatement before any time is printed. Rates: ops/s, and used-state bytes/s
= the used bytes (MapMapSlab.used_bytes) of the rows a call reads and writes
over its time. The call's two launches (the edits, the placement) are told
apart by a kernel trace of this tool (profiles/README.md), not here. One JSON
line (also written to --out)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

BASE, A, SEED = 2000, 16, 0x0A55


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-obj", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import nested_opgen as ng

    if not torch.cuda.is_available():
        raise SystemExit("map_map_apply_bench: no GPU visible")
    reps = max(1, a.n_obj // BASE)
    n = reps * BASE
    batch, S, E = ng.reference(SEED, BASE, A)
    mk = lambda X, arrs, inner: crdts_hip.MapMapSlab(arrs, X.kcap, X.dcap, X.scap, crdts_hip.MapSlab(  # noqa: E731
        inner, X.inner.kcap, X.inner.mcap, X.inner.dcap, X.inner.scap))
    # the partner of object i: object i - 1 (its inner maps with it: kcap inner rows per object)
    O = mk(S, {f: np.roll(v, 1, axis=0) for f, v in S.a.items()},
           {f: np.roll(v, S.kcap, axis=0) for f, v in S.inner.a.items()})

    def tiled(X):
        d = X.to("cuda")
        rep = lambda v: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()  # noqa: E731
        return mk(X, {f: rep(v) for f, v in d.a.items()}, {f: rep(v) for f, v in d.inner.a.items()})

    def tile(X, t):  # tile t of a tiled device slab
        return mk(X, {f: v[t * BASE:(t + 1) * BASE] for f, v in X.a.items()},
                  {f: v[t * BASE * X.kcap:(t + 1) * BASE * X.kcap] for f, v in X.inner.a.items()})

    arrs = dict(zip(ng.OPS_FIELDS, crdts_hip.MapMapOps.arrays_from_lists([ops for _, ops in batch])))
    n_ops, n_clk = len(arrs["kind"]), len(arrs["clk_act"])
    step = {"obj_end": n_ops, "clk_end": n_clk}
    ops = crdts_hip.MapMapOps.from_arrays(*[
        np.concatenate([arrs[f] + np.uint64(r * step[f]) for r in range(reps)]) if f in step else np.tile(arrs[f], reps)
        for f in ng.OPS_FIELDS])
    eng = crdts_hip.Engine(0)
    dS, dO = tiled(S), tiled(O)
    out_a = crdts_hip.MapMapSlab.alloc(n, A, *ng.OUT_CAPS, ng.OUT_INNER, device="cuda")
    out_m = eng.map_map_merge(dS, dO, A)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    t_apply, t_merge = [], []
    for r in range(a.warmup + a.rounds):
        for which in ("apply", "merge"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if which == "apply":
                eng.map_map_apply(dS, ops, A, out=out_a, stream=s, check_status=False)
            else:
                eng.map_map_merge(dS, dO, A, out=out_m, stream=s, check_status=False)
            e1.record(s)
            s.synchronize()
            eng.status(s)
            if r >= a.warmup:
                (t_apply if which == "apply" else t_merge).append(e0.elapsed_time(e1))
    for t in (0, reps - 1):  # the first and the last tile against the restatement, before any time is printed
        try:
            ng.assert_rows(tile(out_a, t), E, what=f"tile {t}")
        except AssertionError as e:
            raise SystemExit(f"map_map_apply_bench: the apply's output differs from the Python restatement: {e}")
    # used bytes: the tiles are copies of the base rows
    b_apply = reps * (S.used_bytes() + E.used_bytes())
    b_merge = reps * (S.used_bytes() + O.used_bytes() + tile(out_m, 0).used_bytes())
    ma, mm = float(np.median(t_apply)), float(np.median(t_merge))
    res = {"tool": "map_map_apply_bench", "n_obj": n, "A": A, "in_caps": [list(ng.IN_CAPS), list(ng.IN_INNER)],
           "out_caps": [list(ng.OUT_CAPS), list(ng.OUT_INNER)], "n_ops": n_ops * reps,
           "ops_per_obj": round(n_ops / BASE, 2), "rounds": a.rounds, "exact": True,
           "apply": {"median_ms": round(ma, 4), "min_ms": round(float(np.min(t_apply)), 4),
                     "max_ms": round(float(np.max(t_apply)), 4), "M_ops_per_s": round(n_ops * reps / ma / 1e3, 2),
                     "M_obj_per_s": round(n / ma / 1e3, 2), "used_bytes": b_apply,
                     "used_GB_per_s": round(b_apply / ma / 1e6, 2)},
           "merge": {"median_ms": round(mm, 4), "min_ms": round(float(np.min(t_merge)), 4),
                     "max_ms": round(float(np.max(t_merge)), 4), "M_obj_per_s": round(n / mm / 1e3, 2),
                     "used_bytes": b_merge, "used_GB_per_s": round(b_merge / mm / 1e6, 2)},
           "apply_over_merge": round(ma / mm, 3),
           "build": crdts_hip.build_record()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
