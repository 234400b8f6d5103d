#!/usr/bin/env python3
"""Timing of the clocks' op path (clock_ops.hip: apply, truncate, subtract,
intersection, value, get — dense rows and CSR runs) beside one merge of the
same rows, in the same process.

Dense shapes: config 1's rows (1M x 16, bench.py's generator arguments) and a
4M x 64 GCounter batch; the PNCounter calls read the same rows as [P|N] rows
of half the actors. CSR shape: a generate_clocks_csr batch with the clock_csr
workload's parameters (1024-actor universe, ~48 actors per clock, 75 % shared
with the other side), --n-csr clocks per side. apply and get take 8 dots per
object, actors drawn over the whole universe (dense) or half from the clock's
own actors (CSR). Every operation is timed with device events after a warm-up,
in rounds that run each operation and crdt_vclock_dense_merge /
crdt_vclock_csr_merge once on the same rows, in an order drawn anew per round,
on preallocated outputs; the in-place dense calls keep running on their
own result (their traffic does not depend on the values). The head of every
result is checked against numpy before any time is printed. Each entry gives
the median / min / max time, objects per second, the ratio to the merge's
median beside the merge's own min-max spread, the bytes the operation must
move and that traffic over the median as a fraction of the 8 TB/s HBM peak.
One JSON line (also written to --out)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))

HBM_PEAK = 8e12  # bytes/s
DOTS = 8
HEAD = 4096  # objects checked against numpy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-csr", type=int, default=1_000_000)
    ap.add_argument("--shapes", default="1000000x16,4000000x64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip

    if not torch.cuda.is_available():
        raise SystemExit("clock_ops_bench: no GPU visible")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(  # noqa: E731
        {8: np.int64, 4: np.int32}[x.dtype.itemsize])).cuda()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731

    def timed(calls):
        """calls: name -> fn(); every round runs each once, in an order drawn
        anew per round (what a call finds in the caches is what some other call
        left there: no call keeps one predecessor); -> name -> [ms]."""
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        order = np.random.default_rng(0x0DE5)
        for r in range(a.warmup + a.rounds):
            for k in order.permutation(list(calls)):
                fn = calls[k]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                s.synchronize()
                eng.status(s)
                if r >= a.warmup:
                    t[k].append(e0.elapsed_time(e1))
        return t

    def entry(ms, n, nbytes, merge_ms, model):
        med = float(np.median(ms))
        mm = float(np.median(merge_ms))
        return {"median_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4),
                "max_ms": round(float(np.max(ms)), 4), "M_objects_per_s": round(n / med / 1e3, 2),
                "over_merge": round(med / mm, 3), "bytes": int(nbytes), "traffic_model": model,
                "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}

    def merge_entry(ms, n, nbytes, model):
        e = entry(ms, n, nbytes, ms, model)
        med = e["median_ms"]
        e["spread_over_median"] = [round(e["min_ms"] / med, 3), round(e["max_ms"] / med, 3)]
        del e["over_merge"]
        return e

    res = {"tool": "clock_ops_bench", "rounds": a.rounds, "warmup": a.warmup, "dots_per_object": DOTS,
           "hbm_peak_TB_per_s": HBM_PEAK / 1e12, "dense": {}, "csr": {}}
    rng = np.random.default_rng(0xC10C)

    # ------------------------------------------------------------------ dense
    for shape in a.shapes.split(","):
        n, A = (int(x) for x in shape.split("x"))
        ha = crdts_hip.generate_dense(n, A, seed=0xC0FFEE01, bits=32, pct_zero=25)
        hb = crdts_hip.generate_dense(n, A, seed=0xC0FFEE01 ^ 0x5EED, bits=32, pct_zero=25)
        da, db = dev(ha), dev(hb)
        h = min(HEAD, n)
        words = n * A
        # correctness of the head, on fresh copies
        for op, f in (("truncate", np.minimum), ("subtract", lambda x, y: np.where(y >= x, np.uint64(0), x)),
                      ("intersection", lambda x, y: np.where(x == y, x, np.uint64(0)))):
            t = da.clone()
            getattr(eng, "dense_" + op)(t, db, A)
            if not (u64(t[:h]) == f(ha[:h], hb[:h])).all():
                raise SystemExit(f"clock_ops_bench: dense {op} {shape} differs from numpy")
        if not (u64(eng.gcounter_value(da, A))[:h] == ha[:h].sum(1, dtype=np.uint64)).all():
            raise SystemExit(f"clock_ops_bench: gcounter value {shape} differs from numpy")
        pv = ha[:h, :A // 2].sum(1, dtype=np.uint64) - ha[:h, A // 2:].sum(1, dtype=np.uint64)
        if not (u64(eng.pncounter_value(da, A // 2))[:h] == pv).all():
            raise SystemExit(f"clock_ops_bench: pncounter value {shape} differs from numpy")
        ends = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(DOTS))
        act = rng.integers(0, A, n * DOTS, dtype=np.uint32)
        ctr = rng.integers(0, 1 << 33, n * DOTS, dtype=np.uint64)
        dr = rng.integers(0, 2, n * DOTS, dtype=np.uint32)
        ops = crdts_hip.ClockOps.from_arrays(ends, act, ctr)
        pops = crdts_hip.ClockOps.from_arrays(ends, act % np.uint32(A // 2), ctr, dr)
        t = da.clone()
        eng.dense_apply(t, ops, A, kind="gcounter")
        exp = ha[:h].copy()
        np.maximum.at(exp, (np.repeat(np.arange(h), DOTS), act[:h * DOTS]), ctr[:h * DOTS])
        if not (u64(t[:h]) == exp).all():
            raise SystemExit(f"clock_ops_bench: dense apply {shape} differs from numpy")
        got = u64(eng.dense_get(da, ops, A))[:h * DOTS]
        if not (got == ha[np.repeat(np.arange(h), DOTS), act[:h * DOTS]]).all():
            raise SystemExit(f"clock_ops_bench: dense get {shape} differs from numpy")
        work = da.clone()
        vout = torch.empty(n, dtype=torch.int64, device="cuda")
        gout = torch.empty(n * DOTS, dtype=torch.int64, device="cuda")
        merge = lambda: eng.dense_merge(work, db, A, "vclock", stream=s)  # noqa: E731
        calls = {"merge": merge}
        for op in ("truncate", "subtract", "intersection"):
            calls[op] = (lambda f: lambda: f(work, db, A, stream=s))(getattr(eng, "dense_" + op))
        calls["gcounter_value"] = lambda: eng.gcounter_value(work, A, out=vout, stream=s)
        calls["pncounter_value"] = lambda: eng.pncounter_value(work, A // 2, out=vout, stream=s)
        calls["apply"] = lambda: eng.dense_apply(work, ops, A, kind="gcounter", stream=s, check_status=False)
        calls["pncounter_apply"] = lambda: eng.dense_apply(work, pops, A // 2, kind="pncounter", stream=s,
                                                           check_status=False)
        calls["get"] = lambda: eng.dense_get(work, ops, A, out=gout, stream=s, check_status=False)
        t = timed(calls)
        nd = n * DOTS
        out = {"merge": merge_entry(t["merge"], n, 24 * words, "24 B per slot: 2 reads + 1 write")}
        for op in ("truncate", "subtract", "intersection"):
            out[op] = entry(t[op], n, 24 * words, t["merge"], "24 B per slot: 2 reads + 1 write")
        for op in ("gcounter_value", "pncounter_value"):
            out[op] = entry(t[op], n, 8 * words + 8 * n, t["merge"], "8 B per slot read + 8 B per object written")
        out["apply"] = entry(t["apply"], n, 8 * n + 20 * nd, t["merge"],
                             "8 B of obj_end per object + per dot 12 B read and an 8-B atomic")
        out["pncounter_apply"] = entry(t["pncounter_apply"], n, 8 * n + 24 * nd, t["merge"],
                                       "8 B of obj_end per object + per dot 16 B read and an 8-B atomic")
        out["get"] = entry(t["get"], n, 8 * n + 20 * nd, t["merge"],
                           "8 B of obj_end per object + per query 4 B actor, 8 B read, 8 B written")
        res["dense"][shape] = out
        del da, db, work, vout, gout, ops, pops, t

    # -------------------------------------------------------------------- CSR
    n = a.n_csr
    hs, ho = crdts_hip.generate_clocks_csr(n, seed=0xC0FFEE09)
    S, O = crdts_hip.ClockBatch.from_host(*hs), crdts_hip.ClockBatch.from_host(*ho)
    off, ln, sact, sctr = hs
    ends = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(DOTS)
    # half of the dots on the clock's own actors, half anywhere in the universe
    lnr, offr = np.repeat(ln.astype(np.int64), DOTS), np.repeat(off.astype(np.int64), DOTS)
    own = sact[np.minimum(offr + rng.integers(0, 1 << 30, n * DOTS) % np.maximum(lnr, 1), sact.size - 1)]
    act = np.where(rng.random(n * DOTS) < 0.5, own, rng.integers(0, 1024, n * DOTS, dtype=np.uint32)).astype(np.uint32)
    ctr = rng.integers(0, 1 << 41, n * DOTS, dtype=np.uint64)
    ops = crdts_hip.ClockOps.from_arrays(ends, act, ctr)
    h = min(HEAD, n)

    def head_clocks(B):
        o, l, x, c = B.to_host()
        return [dict(zip(x[o[i]:o[i] + l[i]].tolist(), c[o[i]:o[i] + l[i]].tolist())) for i in range(h)]

    cs, co = head_clocks(S), head_clocks(O)
    rules = {"truncate": lambda x, y: {k: min(v, y[k]) for k, v in x.items() if k in y},
             "subtract": lambda x, y: {k: v for k, v in x.items() if not y.get(k, 0) >= v},
             "intersection": lambda x, y: {k: v for k, v in x.items() if y.get(k, 0) == v}}
    outs = {}
    for op, rule in rules.items():
        outs[op] = getattr(eng, "clock_csr_" + op)(S, O)
        if head_clocks(outs[op]) != [rule(x, y) for x, y in zip(cs, co)]:
            raise SystemExit(f"clock_ops_bench: csr {op} differs from the dict restatement")
    outs["apply"] = eng.clock_csr_apply(S, ops)
    exp = []
    for i, x in enumerate(cs):
        x = dict(x)
        for k, v in zip(act[i * DOTS:(i + 1) * DOTS].tolist(), ctr[i * DOTS:(i + 1) * DOTS].tolist()):
            if not x.get(k, 0) >= v:
                x[k] = v
        exp.append(dict(sorted(x.items())))
    if head_clocks(outs["apply"]) != exp:
        raise SystemExit("clock_ops_bench: csr apply differs from the dict restatement")
    vout = eng.clock_csr_value(S)
    if u64(vout)[:h].tolist() != [sum(x.values()) & ((1 << 64) - 1) for x in cs]:
        raise SystemExit("clock_ops_bench: csr value differs from the dict restatement")
    gout = eng.clock_csr_get(S, ops)
    if u64(gout)[:h * DOTS].tolist() != [cs[j // DOTS].get(k, 0) for j, k in enumerate(act[:h * DOTS].tolist())]:
        raise SystemExit("clock_ops_bench: csr get differs from the dict restatement")
    mout = eng.clock_csr_merge(S, O)
    calls = {"merge": lambda: eng.clock_csr_merge(S, O, out=mout, stream=s, check_status=False)}
    for op in rules:
        calls[op] = (lambda f, w: lambda: f(S, O, out=w, stream=s, check_status=False))(
            getattr(eng, "clock_csr_" + op), outs[op])
    calls["apply"] = lambda: eng.clock_csr_apply(S, ops, out=outs["apply"], stream=s, check_status=False)
    calls["value"] = lambda: eng.clock_csr_value(S, out=vout, stream=s, check_status=False)
    calls["get"] = lambda: eng.clock_csr_get(S, ops, out=gout, stream=s, check_status=False)
    t = timed(calls)
    es, eo = int(ln.sum()), int(ho[1].sum())
    kept = {k: int(v.len.sum().item()) for k, v in outs.items()}
    em = int(mout.len.sum().item())
    nd = n * DOTS
    c = {"n_obj": n, "entries_self": es, "entries_other": eo,
         "merge": merge_entry(t["merge"], n, 12 * (es + eo + em) + 36 * n,
                              "12 B per entry read per side + 12 B per union entry + 36 B of offsets / lengths per object")}
    for op in rules:
        c[op] = entry(t[op], n, 12 * (es + eo + kept[op]) + 36 * n, t["merge"],
                      "12 B per entry read per side + 12 B per kept entry + 36 B of offsets / lengths per object")
        c[op]["kept_entries"] = kept[op]
    c["apply"] = entry(t["apply"], n, 12 * (es + kept["apply"]) + 12 * nd + 32 * n, t["merge"],
                       "12 B per entry read + 12 B per dot + 12 B per entry written + 32 B of offsets / lengths / "
                       "obj_end per object")
    c["apply"]["out_entries"] = kept["apply"]
    c["value"] = entry(t["value"], n, 8 * es + 20 * n, t["merge"],
                       "8 B per counter read + 12 B of offset / length + 8 B written per object")
    c["get"] = entry(t["get"], n, 20 * n + 12 * nd + 12 * 6 * nd, t["merge"],
                     "20 B of offset / length / obj_end per object + per query 4 B actor, 8 B written and a "
                     "6-probe binary search of 12-B entries (cached after the first query of the object)")
    res["csr"] = c
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
