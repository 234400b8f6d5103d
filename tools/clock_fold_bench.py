#!/usr/bin/env python3
"""Timing of crdt_clock_csr_fold and crdt_clock_dense_fold (clock_fold.hip)
beside the only other way to the same clocks, the chain of R - 1
crdt_vclock_csr_merge / crdt_vclock_dense_merge calls, in one process.

Workloads, R in {2, 4, 8} each:
  csr     --n sparse clocks (1M) of generate_clocks_csr (1024-actor universe,
          ~48 entries a clock), replica r from seed 0xC10C + r
  dense   --n rows of 16 slots (u64 counters of 40 bits, a quarter absent)
Legs:
  fold    one fold call over the R replicas into a preallocated output
  chain   R - 1 merge calls: the CSR chain into preallocated intermediates
          sized for the sum of their inputs (allocation is not timed), the
          dense chain in place on an accumulator that holds replica 0 (a max is
          idempotent: every round moves the same bytes). At R = 2 the chain is
          one merge, and its min-max spread over the rounds is the margin the
          design allows the fold there.
Every leg is timed with device events after a warm-up, in rounds that run each
leg once in an order drawn anew per round. Before any time is printed the
fold's output must equal the chain's: offsets, lengths and used entries (CSR),
every word (dense). Each entry gives median / min / max and the bytes a fold
must move over the leg's median (CSR: 12 B per input entry and per output
entry, 12 B of offset and length per object per replica and for the output;
dense: R + 1 words per slot), also as a fraction of the 8 TB/s HBM peak. One
JSON line (also written to --out)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))

HBM_PEAK = 8e12  # bytes/s
SLOTS = 16
REPS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", default=",".join(map(str, REPS)), help="replica counts, comma-separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip

    if not torch.cuda.is_available():
        raise SystemExit("clock_fold_bench: no GPU visible")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    n = a.n
    rs = [int(x) for x in a.reps.split(",")]
    res = {"tool": "clock_fold_bench", "n": n, "dense_slots": SLOTS, "rounds": a.rounds, "warmup": a.warmup,
           "hbm_peak_TB_per_s": HBM_PEAK / 1e12, "stage_entries": crdts_hip.CLOCK_FOLD_STAGE_ENTRIES, "csr": {},
           "dense": {}, "ratios": {}}

    def timed(calls, seed):
        t = {k: [] for k in calls}
        order = np.random.default_rng(seed)
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
        return t

    def legs(t, fold_bytes):
        out, med = {}, {}
        for k, ms in t.items():
            med[k] = float(np.median(ms))
            out[k] = {"median_ms": round(med[k], 4), "min_ms": round(float(np.min(ms)), 4),
                      "max_ms": round(float(np.max(ms)), 4), "M_objects_per_s": round(n / med[k] / 1e3, 2),
                      "fold_bytes_per_s": round(fold_bytes / (med[k] * 1e-3), 1),
                      "fraction_of_hbm_peak": round(fold_bytes / (med[k] * 1e-3) / HBM_PEAK, 4)}
        return out, med

    def ratios(tag, R, t, med):
        res["ratios"][f"{tag}_fold_over_chain_R{R}"] = round(med["fold"] / med["chain"], 3)
        if R == 2:
            spread = float(np.max(t["chain"]) - np.min(t["chain"]))
            res["ratios"].update({f"{tag}_fold_minus_merge_R2_ms": round(med["fold"] - med["chain"], 4),
                                  f"{tag}_merge_min_max_spread_R2_ms": round(spread, 4),
                                  f"{tag}_fold_within_merge_spread_R2": bool(med["fold"] - med["chain"] <= spread)})

    def used(b):
        """The used entries of a device batch, in object order."""
        ln = b.len.to(torch.int64)
        idx = torch.repeat_interleave(b.off - (torch.cumsum(ln, 0) - ln), ln) + torch.arange(int(ln.sum()),
                                                                                             device=ln.device)
        return b.act[idx], b.ctr[idx]

    # ------------------------------------------------------------------ CSR
    host = [crdts_hip.generate_clocks_csr(n, seed=0xC10C + r)[r % 2] for r in range(max(rs))]
    for R in rs:
        reps = [crdts_hip.ClockBatch.from_host(*h) for h in host[:R]]
        total = sum(r.n_entries for r in reps)
        fold_out = eng._csr_out(n, total)
        chain_out = [eng._csr_out(n, sum(r.n_entries for r in reps[:k + 1])) for k in range(1, R)]

        def fold():
            eng.clock_csr_fold(reps, out=fold_out, stream=s, check_status=False)

        def chain():
            acc = reps[0]
            for k in range(1, R):
                acc = eng.clock_csr_merge(acc, reps[k], out=chain_out[k - 1], stream=s, check_status=False)

        with torch.cuda.stream(s):
            fold()
            chain()
        s.synchronize()
        eng.status(s)
        c = chain_out[-1]
        same = torch.equal(fold_out.off, c.off) and torch.equal(fold_out.len, c.len)
        if same:
            (fa, fc), (ca, cc) = used(fold_out), used(c)
            same = torch.equal(fa, ca) and torch.equal(fc, cc)
            del fa, fc, ca, cc
        if not same:
            raise SystemExit(f"clock_fold_bench: csr R={R}: the fold differs from the merge chain")
        t = timed({"fold": fold, "chain": chain}, 0xF01D + R)
        out_entries = int(fold_out.len.sum())
        nbytes = 12 * total + 12 * out_entries + 12 * n * (R + 1)
        entry, med = legs(t, nbytes)
        res["csr"][str(R)] = {"input_entries_per_object": round(total / n, 3),
                              "union_entries_per_object": round(out_entries / n, 3), "fold_bytes": nbytes,
                              "legs": entry}
        ratios("csr", R, t, med)
        del reps, fold_out, chain_out, c
        torch.cuda.empty_cache()

    # ---------------------------------------------------------------- dense
    for R in rs:
        rows = [torch.from_numpy(crdts_hip.generate_dense(n, SLOTS, seed=0xDE5E + r).view(np.int64)).cuda()
                for r in range(R)]
        fold_out, acc = torch.empty_like(rows[0]), rows[0].clone()

        def fold():
            eng.dense_fold(rows, SLOTS, out=fold_out, stream=s)

        def chain():
            for k in range(1, R):
                eng.dense_merge(acc, rows[k], SLOTS, "vclock", stream=s)

        with torch.cuda.stream(s):
            fold()
            chain()
        s.synchronize()
        eng.status(s)
        if not torch.equal(fold_out, acc):
            raise SystemExit(f"clock_fold_bench: dense R={R}: the fold differs from the merge chain")
        t = timed({"fold": fold, "chain": chain}, 0xDF01D + R)
        nbytes = 8 * n * SLOTS * (R + 1)
        entry, med = legs(t, nbytes)
        res["dense"][str(R)] = {"fold_bytes": nbytes, "chain_bytes": 8 * n * SLOTS * 3 * (R - 1), "legs": entry}
        ratios("dense", R, t, med)
        del rows, fold_out, acc
        torch.cuda.empty_cache()

    res["claims"] = {f"{tag}_fold_faster_than_chain_R{R}": res["ratios"][f"{tag}_fold_over_chain_R{R}"] < 1.0
                     for tag in ("csr", "dense") for R in rs if R > 2}
    if 2 in rs:
        for tag in ("csr", "dense"):
            res["claims"][f"{tag}_fold_within_merge_spread_R2"] = res["ratios"][f"{tag}_fold_within_merge_spread_R2"]
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
