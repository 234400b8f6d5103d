#!/usr/bin/env python3
"""Timing of crdt_mvreg_fold (mvreg_fold.hip) beside the only other way to the
same registers, the chain of R - 1 crdt_mvreg_merge calls, in one process.

Shape: --n registers (4M), A = 16, 4 slots per replica, R in {2, 4, 8}: the
bench.py --workload mvreg shape extended to R replicas. The registers are a
4,000-register batch of tests/mvreg_foldgen.py::gen (structured: dominance and
equal clocks across and inside the replicas, poisoned unused slots), repeated
on the device to --n. Per R, three legs:
  fold    one crdt_mvreg_fold over the R replicas, out_cap = 4 R
  chain   R - 1 Engine.mvreg_merge calls into preallocated outputs of the
          running-sum capacity (8, 12, ..., 4 R): the only other way to the
          same registers, so it is the yardstick
  merge   one mvreg_merge of replicas 0 and 1 (out_cap 8)
Every leg is timed with device events after a warm-up, in rounds that run each
leg once in an order drawn anew per round, on preallocated outputs. Before any
time is printed the fold's output must equal the chain's bit for bit over all
--n registers, and the chained C++ oracle's on the generated batch.
Each entry gives median / min / max, registers per second, the bytes the leg
must move (counts, used input rows and values, every output slot) and that
traffic over the median as a fraction of the 8 TB/s HBM peak. "ratios" holds
fold / chain per R and, at R = 2, fold / merge with the merge's own min-max
spread, the margin the design allows the fold there. One JSON line (also
written to --out)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK = 8e12  # bytes/s
A, CAP, BASE_N = 16, 4, 4000
REPS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", default=",".join(map(str, REPS)), help="replica counts, comma-separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import mvreg_foldgen as fg

    if not torch.cuda.is_available():
        raise SystemExit("mvreg_fold_bench: no GPU visible")
    if a.n % BASE_N:
        raise SystemExit(f"mvreg_fold_bench: --n must be a multiple of {BASE_N}")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    n, times = a.n, a.n // BASE_N
    res = {"tool": "mvreg_fold_bench", "n": n, "n_actors": A, "slots_per_replica": CAP, "rounds": a.rounds,
           "warmup": a.warmup, "hbm_peak_TB_per_s": HBM_PEAK / 1e12, "replicas": {}, "ratios": {}}
    slot = 8 * A + 8  # a clock row and its value

    def dev(t):
        t = np.ascontiguousarray(t)
        t = torch.from_numpy(t.view(np.int32 if t.dtype == np.uint32 else np.int64)).cuda()
        return t.repeat((times,) + (1,) * (t.dim() - 1))

    def new_out(cap):
        return (torch.empty(n, dtype=torch.int32, device="cuda"),
                torch.empty((n, cap, A), dtype=torch.int64, device="cuda"),
                torch.empty((n, cap), dtype=torch.int64, device="cuda"))

    rs = [int(x) for x in a.reps.split(",")]
    for R in rs:
        host = fg.gen(0xB0 + R, BASE_N, A, (CAP,) * R)
        exp = fg.chain_oracle(host, CAP * R)
        reps = [tuple(dev(x) for x in r) for r in host]
        fold_out, merge_out = new_out(CAP * R), new_out(2 * CAP)
        chain_out = [new_out(CAP * (k + 1)) for k in range(1, R)]

        def fold():
            eng.mvreg_fold(reps, A, out=fold_out, stream=s, check_status=False)

        def chain():
            acc = reps[0]
            for k in range(1, R):
                acc = eng.mvreg_merge(acc, reps[k], A, out=chain_out[k - 1], stream=s, check_status=False)

        def merge():
            eng.mvreg_merge(reps[0], reps[1], A, out=merge_out, stream=s, check_status=False)

        calls = {"fold": fold, "chain": chain, "merge": merge}
        # ---- correctness: fold == chain over all n registers, == the chained oracle on the generated batch
        with torch.cuda.stream(s):
            fold()
            chain()
        s.synchronize()
        eng.status(s)
        if not all(torch.equal(f, c) for f, c in zip(fold_out, chain_out[-1])):
            raise SystemExit(f"mvreg_fold_bench: R={R}: the fold differs from the merge chain")
        got = [t[:BASE_N].cpu().numpy() for t in fold_out]
        if not all((g.view(e.dtype) == e).all() for g, e in zip(got, exp)):
            raise SystemExit(f"mvreg_fold_bench: R={R}: the fold differs from the chained oracle")
        # ---- timing
        t = {k: [] for k in calls}
        order = np.random.default_rng(0x0F01D + R)
        for r in range(a.warmup + a.rounds):
            for k in order.permutation(list(calls)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(s):
                    e0.record(s)
                    calls[k]()
                    e1.record(s)
                s.synchronize()
                eng.status(s)
                if r >= a.warmup:
                    t[k].append(e0.elapsed_time(e1))
        # ---- the bytes each leg must move: counts, used rows and values read; every output slot written
        used = [int(r[0].sum()) * times for r in host]
        inter = [int(x.sum()) * times for x in _chain_counts(fg, host)]  # survivors after each merge of the chain
        nbytes = {
            "fold": n * 4 * R + sum(used) * slot + n * (4 + CAP * R * slot),
            "chain": sum(n * 8 + ((used[0] if k == 1 else inter[k - 2]) + used[k]) * slot
                         + n * (4 + CAP * (k + 1) * slot) for k in range(1, R)),
            "merge": n * 8 + (used[0] + used[1]) * slot + n * (4 + 2 * CAP * slot),
        }
        entry = {"used_slots_per_register": round(sum(used) / n, 3), "survivors_per_register": round(inter[-1] / n, 3),
                 "legs": {}}
        med = {}
        for k, ms in t.items():
            med[k] = float(np.median(ms))
            entry["legs"][k] = {"median_ms": round(med[k], 4), "min_ms": round(float(np.min(ms)), 4),
                                "max_ms": round(float(np.max(ms)), 4), "M_registers_per_s": round(n / med[k] / 1e3, 2),
                                "bytes": int(nbytes[k]),
                                "fraction_of_hbm_peak": round(nbytes[k] / (med[k] * 1e-3) / HBM_PEAK, 4)}
        res["replicas"][str(R)] = entry
        res["ratios"][f"fold_over_chain_R{R}"] = round(med["fold"] / med["chain"], 3)
        if R == 2:
            spread = float(np.max(t["merge"]) - np.min(t["merge"]))
            res["ratios"].update({"fold_over_merge_R2": round(med["fold"] / med["merge"], 3),
                                  "fold_minus_merge_R2_ms": round(med["fold"] - med["merge"], 4),
                                  "merge_min_max_spread_R2_ms": round(spread, 4),
                                  "fold_within_merge_spread_R2": bool(med["fold"] - med["merge"] <= spread)})
        del reps, fold_out, merge_out, chain_out
        torch.cuda.empty_cache()
    res["claims"] = {f"fold_faster_than_chain_R{R}": res["ratios"][f"fold_over_chain_R{R}"] < 1.0 for R in rs if R > 2}
    if 2 in rs:
        res["claims"]["fold_within_merge_spread_R2"] = res["ratios"]["fold_within_merge_spread_R2"]
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def _chain_counts(fg, host):
    """The survivor counts after each merge of the chain, on the generated batch."""
    return [fg.chain_np(host[:k + 1], CAP * (k + 1))[0] for k in range(1, len(host))]


if __name__ == "__main__":
    main()
