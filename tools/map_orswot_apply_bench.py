#!/usr/bin/env python3
"""Timing of the batched Map<u64, Orswot>::apply (crdt_map_orswot_apply) beside
the merge of the same maps (crdt_map_orswot_merge) — the only other way to
bring a remote change into a device-resident map.

The 2,000-object generated batch of the tests (tests/map_orswot_opgen.py,
A = 16) is tiled to --n-obj objects on the device. Both calls are timed with
device events after a warm-up, alternating, on preallocated outputs; the merge
takes the same `self` rows against partners of the same size (the rows shifted
by one object). The apply's first and last 2,000 output rows are checked
against the Python restatement before any time is reported. Rates: ops/s, and
used-state bytes/s = the used bytes (MapOrswotSlab.used_bytes) of the rows a
call reads and writes over its time. One JSON line (also written to --out)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

BASE, A = 2000, 16


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
    import map_orswot_opgen as og
    import map_slab

    if not torch.cuda.is_available():
        raise SystemExit("map_orswot_apply_bench: no GPU visible")
    in_caps, out_caps = og.caps(4), og.caps(8)
    reps = max(1, a.n_obj // BASE)
    n = reps * BASE
    batch = og.gen_batch(0x0A57, BASE, A)
    S = crdts_hip.MapOrswotSlab.alloc(BASE, A, **in_caps)
    E = crdts_hip.MapOrswotSlab.alloc(BASE, A, **out_caps)
    same_key = total = 0
    for i, (pre, ops) in enumerate(batch):
        m = og.new_map()
        for op in pre:
            og.apply_op(m, op)
        map_slab.orswot_map_to_row(m, S, i, A)
        for op in ops:
            og.apply_op(m, op)
        map_slab.orswot_map_to_row(m, E, i, A)
        keys = [op[3] if op[0] != "rm" else op[1] for op in ops if op[0] != "nop"]
        same_key += sum(x == y for x, y in zip(keys, keys[1:]))
        total += max(0, len(keys) - 1)
    O = crdts_hip.MapOrswotSlab({f: np.roll(v, 1, axis=0) for f, v in S.a.items()}, in_caps)

    def tiled(X):
        d = X.to("cuda")
        return crdts_hip.MapOrswotSlab({f: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()
                                        for f, v in d.a.items()}, X.caps)

    ends, kind, key, act, ctr, mem, cend, cact, cctr = crdts_hip.MapOrswotOps.arrays_from_lists(
        [ops for _, ops in batch])
    n_ops, n_clk = len(kind), len(cact)
    shift = lambda e, step: np.concatenate([e + np.uint64(r * step) for r in range(reps)])  # noqa: E731
    ops = crdts_hip.MapOrswotOps.from_arrays(shift(ends, n_ops), np.tile(kind, reps), np.tile(key, reps),
                                             np.tile(act, reps), np.tile(ctr, reps), np.tile(mem, reps),
                                             shift(cend, n_clk), np.tile(cact, reps), np.tile(cctr, reps))
    eng = crdts_hip.Engine(0)
    dS, dO = tiled(S), tiled(O)
    out_a = crdts_hip.MapOrswotSlab.alloc(n, A, device="cuda", **out_caps)
    out_m = eng.map_orswot_merge(dS, dO, A)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    t_apply, t_merge = [], []
    for r in range(a.warmup + a.rounds):
        for which in ("apply", "merge"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if which == "apply":
                eng.map_orswot_apply(dS, ops, A, out=out_a, stream=s, check_status=False)
            else:
                eng.map_orswot_merge(dS, dO, A, out=out_m, stream=s, check_status=False)
            e1.record(s)
            s.synchronize()
            eng.status(s)
            if r >= a.warmup:
                (t_apply if which == "apply" else t_merge).append(e0.elapsed_time(e1))
    sub = lambda X, lo, hi: crdts_hip.MapOrswotSlab({f: v[lo:hi] for f, v in X.a.items()}, X.caps)  # noqa: E731
    exp = E.canonical()
    exact = True
    for lo in (0, n - BASE):  # the first and the last tile
        got = sub(out_a, lo, lo + BASE).canonical()
        exact = exact and all(bool((np.asarray(got.a[f]) == np.asarray(exp.a[f])).all()) for f in exp.a)
    # used bytes: the tiles are copies of the base rows
    b_apply = reps * (S.used_bytes() + E.used_bytes())
    b_merge = reps * (S.used_bytes() + O.used_bytes() + sub(out_m, 0, BASE).used_bytes())
    ma, mm = float(np.median(t_apply)), float(np.median(t_merge))
    res = {"tool": "map_orswot_apply_bench", "n_obj": n, "A": A, "in_caps": in_caps, "out_caps": out_caps,
           "n_ops": n_ops * reps, "ops_per_obj": round(n_ops / BASE, 2),
           "same_key_as_previous_op": round(same_key / max(1, total), 3), "rounds": a.rounds, "exact": exact,
           "apply": {"median_ms": round(ma, 4), "min_ms": round(float(np.min(t_apply)), 4),
                     "max_ms": round(float(np.max(t_apply)), 4), "M_ops_per_s": round(n_ops * reps / ma / 1e3, 2),
                     "M_obj_per_s": round(n / ma / 1e3, 2), "used_bytes": b_apply,
                     "used_GB_per_s": round(b_apply / ma / 1e6, 2)},
           "merge": {"median_ms": round(mm, 4), "min_ms": round(float(np.min(t_merge)), 4),
                     "max_ms": round(float(np.max(t_merge)), 4), "M_obj_per_s": round(n / mm / 1e3, 2),
                     "used_bytes": b_merge, "used_GB_per_s": round(b_merge / mm / 1e6, 2)},
           "build": crdts_hip.build_record()}
    if not exact:
        raise SystemExit("map_orswot_apply_bench: the apply's output differs from the Python restatement")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
