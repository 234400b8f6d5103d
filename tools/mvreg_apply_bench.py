#!/usr/bin/env python3
"""Timing of the batched MVReg op path (crdt_mvreg_apply, crdt_mvreg_truncate)
beside crdt_mvreg_merge over the same slabs, in one process.

A base batch of generated registers and Put lists (tests/mvreg_opgen.py:
A = 16, self_cap 4, 4 Puts per register — read-derived contexts, replays of a
stored clock, clocks one step below one, random concurrent clocks, ~5 % empty
clocks) is tiled to --n-obj registers on the device; out_cap 8. The merge
takes the same `self` slab against the slab shifted by one register. All three
calls are timed with device events after a warm-up, alternating, on
preallocated outputs. The apply's and the truncate's first and last tiles are
checked against the Python restatement. Algorithmic bytes: the used input
slots (clock row + value) and slot counts, the op arrays (or the truncating
clock rows), and the whole zero-filled output block; the fraction is of 8 TB/s.
One JSON line (also written to --out)."""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

BASE, A, CAP, OUT_CAP, N_OPS, HI = 4000, 16, 4, 8, 4, 3
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-obj", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import mvreg_opgen as mo
    from mvreg_opgen import crdts_ref

    if not torch.cuda.is_available():
        raise SystemExit("mvreg_apply_bench: no GPU visible")
    reps = max(1, a.n_obj // BASE)
    n = reps * BASE
    b = mo.gen_batch(0xBE5C, BASE, A, CAP, HI, N_OPS, N_OPS)
    S = mo.slab(b["regs0"], CAP, A)
    E = mo.slab(b["regs"], OUT_CAP, A)
    # truncating clocks: random rows, 30 % all zero; the restatement's result
    rng = random.Random(0xBE5D)
    T = np.zeros((BASE, A), np.uint64)
    trunc = []
    for i, r in enumerate(b["regs0"]):
        c = crdts_ref.VClock() if rng.random() < 0.3 else \
            crdts_ref.VClock([(x, v) for x in range(A) for v in [rng.randrange(HI)] if v])
        for x, v in c.dots.items():
            T[i, x] = v
        t = r.clone()
        t.truncate(c)
        trunc.append(t)
    ET = mo.slab(trunc, CAP, A)

    def dev(x, tile=True):
        x = np.ascontiguousarray(x)
        t = torch.from_numpy(x.view(np.int32 if x.dtype == np.uint32 else np.int64)).to("cuda:0")
        return t.repeat((reps,) + (1,) * (t.dim() - 1)).contiguous() if tile else t

    dS = tuple(dev(x) for x in S)
    dO = tuple(dev(np.roll(x, 1, axis=0)) for x in S)
    dT = dev(T)
    ends, val, cend, cact, cctr = crdts_hip.MVRegOps.arrays_from_lists(b["ops"])
    n_ops, n_clk = len(val), len(cact)
    shift = lambda e, step: np.concatenate([e + np.uint64(r * step) for r in range(reps)])  # noqa: E731
    ops = crdts_hip.MVRegOps.from_arrays(shift(ends, n_ops), np.tile(val, reps), shift(cend, n_clk),
                                         np.tile(cact, reps), np.tile(cctr, reps))
    eng = crdts_hip.Engine(0)

    def alloc(cap):
        return (torch.empty(n, dtype=torch.int32, device="cuda:0"),
                torch.empty((n, cap, A), dtype=torch.int64, device="cuda:0"),
                torch.empty((n, cap), dtype=torch.int64, device="cuda:0"))

    out_a, out_t, out_m = alloc(OUT_CAP), alloc(CAP), alloc(OUT_CAP)
    p = lambda t: crdts_hip.C.c_void_p(t.data_ptr())  # noqa: E731
    s = torch.cuda.Stream()

    def merge():
        crdts_hip.check(crdts_hip.lib.crdt_mvreg_merge(
            eng.ctx, p(dS[0]), p(dS[1]), p(dS[2]), CAP, p(dO[0]), p(dO[1]), p(dO[2]), CAP, p(out_m[0]), p(out_m[1]),
            p(out_m[2]), OUT_CAP, n, A, eng._stream(s)), "mvreg_merge")

    calls = {"apply": lambda: eng.mvreg_apply(dS, ops, A, out=out_a, stream=s, check_status=False),
             "truncate": lambda: eng.mvreg_truncate(dS, dT, A, out=out_t, stream=s, check_status=False),
             "merge": merge}
    times = {k: [] for k in calls}
    torch.cuda.synchronize()
    for r in range(a.warmup + a.rounds):
        for which, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            s.synchronize()
            eng.status(s)
            if r >= a.warmup:
                times[which].append(e0.elapsed_time(e1))

    def tiles_equal(out, exp):
        ok = True
        for lo in (0, n - BASE):
            for g, e in zip(out, exp):
                g = g[lo:lo + BASE].cpu().numpy()
                ok = ok and bool((g.view(e.dtype) == e).all())
        return ok

    exact = {"apply": tiles_equal(out_a, E), "truncate": tiles_equal(out_t, ET)}
    slot = 8 * A + 8
    used_in = reps * (int(S[0].sum()) * slot + 4 * BASE)
    bytes_ = {"apply": used_in + reps * (8 * BASE + 16 * n_ops + 12 * n_clk) + n * (OUT_CAP * slot + 4),
              "truncate": used_in + n * 8 * A + n * (CAP * slot + 4),
              "merge": used_in + reps * (int(np.roll(S[0], 1).sum()) * slot + 4 * BASE) + n * (OUT_CAP * slot + 4)}
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"tool": "mvreg_apply_bench", "n_obj": n, "A": A, "self_cap": CAP, "out_cap": OUT_CAP,
           "n_ops": n_ops * reps, "ops_per_obj": N_OPS, "n_clk": n_clk * reps, "classes": b["classes"],
           "rounds": a.rounds, "exact": exact}
    for k in calls:
        res[k] = {"median_ms": round(med[k], 4), "min_ms": round(float(np.min(times[k])), 4),
                  "max_ms": round(float(np.max(times[k])), 4), "M_obj_per_s": round(n / med[k] / 1e3, 2),
                  "algorithmic_bytes": bytes_[k], "GB_per_s": round(bytes_[k] / med[k] / 1e6, 2),
                  "fraction_of_8TBps": round(bytes_[k] / (med[k] * 1e-3) / PEAK, 4)}
    res["apply"]["M_ops_per_s"] = round(n_ops * reps / med["apply"] / 1e3, 2)
    res["apply_over_merge"] = round(med["apply"] / med["merge"], 3)
    res["truncate_over_merge"] = round(med["truncate"] / med["merge"], 3)
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(exact.values()):
        raise SystemExit(f"mvreg_apply_bench: output differs from the Python restatement: {exact}")


if __name__ == "__main__":
    main()
