#!/usr/bin/env python3
"""Timing of the LWWReg calls (lwwreg.hip: merge, apply, fold, the bincode
codec) beside their yardsticks, in one process.

Shape: --n registers (4M) of one marker word. Values come from 3 keys and
markers from [0, 2^12), so a few hundred equal markers conflict per merge.
  merge          crdt_lwwreg_merge with the conflict bitmap and the count
  merge_bare     the same with both outputs null
  dense_merge    crdt_vclock_dense_merge over n rows of 2 slots: the same
                 48 B per object, the merge's yardstick
  apply          4 ops per register (the lane-per-register tier), n_err only
  fold           8 replicas in one pass, with n_err
  merge_chain    7 chained crdt_lwwreg_merge calls (bare) over the same 8
                 replicas: the fold's yardstick
  from_bincode / to_bincode   LWWReg<u64, u64> blobs, 16 bytes, stride 16
Every call is timed with device events after a warm-up, in rounds that run
each call once in an order drawn anew per round, on preallocated outputs; the
in-place calls keep running on their own result (their traffic does not
depend on the values). Every result is checked against numpy before any time
is printed. Each entry gives the median / min / max time, registers per
second, the bytes the call must move and that traffic over the median as a
fraction of the 8 TB/s HBM peak; the ratios the design records are under
"ratios". One JSON line (also written to --out)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))

HBM_PEAK = 8e12  # bytes/s
OPS = 4
REPS = 8


def np_merge(sv, sm, ov, om):
    """-> (val, marker, conflict) of self.merge(other), elementwise (src/lwwreg.rs:56-66)."""
    import numpy as np

    gt = om > sm
    return np.where(gt, ov, sv), np.where(gt, om, sm), (om == sm) & (ov != sv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip

    if not torch.cuda.is_available():
        raise SystemExit("lwwreg_bench: no GPU visible")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    n = a.n
    rng = np.random.default_rng(0x11E6)
    keys = np.array([7, 8, (1 << 64) - 1], np.uint64)
    hv = [keys[rng.integers(0, 3, n)] for _ in range(REPS)]
    hm = [rng.integers(0, 1 << 12, n, dtype=np.uint64) for _ in range(REPS)]
    reps = [crdts_hip.LWWBatch.from_arrays(v, m) for v, m in zip(hv, hm)]
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731

    # ---- correctness, on fresh copies
    S = reps[0].clone()
    bitmap, count = eng.lwwreg_merge(S, reps[1])
    ev, em, ec = np_merge(hv[0], hm[0], hv[1], hm[1])
    bits = np.unpackbits(u64(bitmap).view(np.uint8), bitorder="little")[:n].astype(bool)
    if not ((u64(S.val) == ev).all() and (u64(S.marker)[:, 0] == em).all() and (bits == ec).all()
            and int(count.item()) == int(ec.sum())):
        raise SystemExit("lwwreg_bench: merge differs from numpy")
    conflicts = int(ec.sum())
    fv, fm, fe = hv[0], hm[0], np.zeros(n, np.int64)
    for r in range(1, REPS):
        fv, fm, c = np_merge(fv, fm, hv[r], hm[r])
        fe += c
    fold_out, fold_err = eng.lwwreg_fold(reps)
    if not ((u64(fold_out.val) == fv).all() and (u64(fold_out.marker)[:, 0] == fm).all()
            and (fold_err.cpu().numpy() == fe).all()):
        raise SystemExit("lwwreg_bench: fold differs from numpy")
    chain = reps[0].clone()
    for r in range(1, REPS):
        eng.lwwreg_merge(chain, reps[r], want_bitmap=False, want_count=False)
    if not ((u64(chain.val) == fv).all() and (u64(chain.marker)[:, 0] == fm).all()):
        raise SystemExit("lwwreg_bench: the merge chain differs from numpy")
    # 4 ops per register: register i's ops are replicas 1..4's register i
    ends = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(OPS)
    ov = np.stack(hv[1:1 + OPS], axis=1).reshape(-1)
    om = np.stack(hm[1:1 + OPS], axis=1).reshape(-1)
    ops = crdts_hip.LWWOps.from_arrays(ends, ov, om)
    A = reps[0].clone()
    n_err = eng.lwwreg_apply(A, ops)
    av, am, ae = hv[0], hm[0], np.zeros(n, np.int64)
    for r in range(1, 1 + OPS):
        av, am, c = np_merge(av, am, hv[r], hm[r])
        ae += c
    if not ((u64(A.val) == av).all() and (u64(A.marker)[:, 0] == am).all() and (n_err.cpu().numpy() == ae).all()):
        raise SystemExit("lwwreg_bench: apply differs from numpy")
    blobs = eng.lwwreg_to_bincode(reps[0], 8, 8)
    hb = np.stack([hv[0], hm[0]], axis=1).astype("<u8").view(np.uint8).reshape(-1)
    if not (blobs.cpu().numpy() == hb).all():
        raise SystemExit("lwwreg_bench: to_bincode differs from numpy")
    back = eng.lwwreg_from_bincode(blobs, n, 8, 8)
    if not ((u64(back.val) == hv[0]).all() and (u64(back.marker)[:, 0] == hm[0]).all()):
        raise SystemExit("lwwreg_bench: from_bincode differs from numpy")

    # ---- timing
    dense_a = torch.from_numpy(np.stack([hv[0], hm[0]], axis=1).view(np.int64)).cuda()
    dense_b = torch.from_numpy(np.stack([hv[1], hm[1]], axis=1).view(np.int64)).cuda()
    W, Wb, Wc, Wa = reps[0].clone(), reps[0].clone(), reps[0].clone(), reps[0].clone()

    def chain7():
        for r in range(1, REPS):
            eng.lwwreg_merge(Wc, reps[r], want_bitmap=False, want_count=False, stream=s)

    calls = {
        "merge": lambda: eng.lwwreg_merge(W, reps[1], bitmap=bitmap, count=count, stream=s),
        "merge_bare": lambda: eng.lwwreg_merge(Wb, reps[1], want_bitmap=False, want_count=False, stream=s),
        "dense_merge": lambda: eng.dense_merge(dense_a, dense_b, 2, "vclock", stream=s),
        "apply": lambda: eng.lwwreg_apply(Wa, ops, n_err=n_err, stream=s, check_status=False),
        "fold": lambda: eng.lwwreg_fold(reps, out=fold_out, n_err=fold_err, stream=s),
        "merge_chain": chain7,
        "from_bincode": lambda: eng.lwwreg_from_bincode(blobs, n, 8, 8, out=back, stream=s),
        "to_bincode": lambda: eng.lwwreg_to_bincode(reps[0], 8, 8, out=blobs, stream=s, check_status=False),
    }
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    order = np.random.default_rng(0x0DE5)
    for r in range(a.warmup + a.rounds):
        for k in order.permutation(list(calls)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):  # the calls' own output tensors are made on the timed stream too
                e0.record(s)
                calls[k]()
                e1.record(s)
            s.synchronize()
            eng.status(s)
            if r >= a.warmup:
                t[k].append(e0.elapsed_time(e1))

    models = {
        "merge": (48 + 1 / 8, "48 B per register (2 x 16 B read, 16 B written) + 1 bit of the bitmap"),
        "merge_bare": (48, "48 B per register"),
        "dense_merge": (48, "24 B per slot, 2 slots per row"),
        "apply": (8 + 32 + 4 + 16 * OPS, "8 B obj_end + 16 B state read + 16 B written + 4 B n_err + 16 B per op"),
        "fold": (16 * REPS + 16 + 4, "16 B per replica read + 16 B written + 4 B n_err"),
        "merge_chain": (48 * (REPS - 1), "7 merges of 48 B per register"),
        "from_bincode": (32, "16 B blob read + 16 B state written"),
        "to_bincode": (32, "16 B state read + 16 B blob written"),
    }
    res = {"tool": "lwwreg_bench", "n": n, "marker_words": 1, "rounds": a.rounds, "warmup": a.warmup,
           "ops_per_register": OPS, "replicas": REPS, "conflicts_per_merge": conflicts,
           "wave_min_ops": crdts_hip.LWWREG_WAVE_MIN_OPS, "hbm_peak_TB_per_s": HBM_PEAK / 1e12, "calls": {}}
    med = {}
    for k, ms in t.items():
        med[k] = float(np.median(ms))
        nbytes = models[k][0] * n
        res["calls"][k] = {"median_ms": round(med[k], 4), "min_ms": round(float(np.min(ms)), 4),
                           "max_ms": round(float(np.max(ms)), 4), "M_registers_per_s": round(n / med[k] / 1e3, 2),
                           "spread_over_median": [round(float(np.min(ms)) / med[k], 3),
                                                  round(float(np.max(ms)) / med[k], 3)],
                           "bytes": int(nbytes), "traffic_model": models[k][1],
                           "fraction_of_hbm_peak": round(nbytes / (med[k] * 1e-3) / HBM_PEAK, 4)}
    res["ratios"] = {"merge_over_dense_merge": round(med["merge"] / med["dense_merge"], 3),
                     "merge_bare_over_dense_merge": round(med["merge_bare"] / med["dense_merge"], 3),
                     "dense_merge_spread_over_median": res["calls"]["dense_merge"]["spread_over_median"],
                     "fold_over_merge_chain": round(med["fold"] / med["merge_chain"], 3),
                     "merge_chain_over_fold": round(med["merge_chain"] / med["fold"], 3)}
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not med["fold"] < med["merge_chain"]:
        raise SystemExit("lwwreg_bench: the fold is not faster than 7 chained merges")


if __name__ == "__main__":
    main()
