#!/usr/bin/env python3
"""Timing of the batched Map::truncate of the three Map types
(crdt_map_mvreg_truncate, crdt_map_orswot_truncate, crdt_map_map_truncate)
beside one merge of the same maps, in the same process.

The maps are the populations of the apply bench tools (tools/map_apply_bench.py,
map_orswot_apply_bench.py, map_map_apply_bench.py): their 2,000 generated
objects at A = 16 after the whole op stream, in slabs of the population's own
largest sizes, tiled to --n-obj objects on the device. Object i's truncating
clock T is drawn from its own map clock, each actor independently 0, below its
counter, equal to it or above it (tests/map_truncgen.py, mode `mixed`). Both calls are timed with device events
after a warm-up, alternating, on preallocated outputs; the merge takes the
same rows against partners of the same size (the rows shifted by one object).
The truncate's first and last tile are checked against the Python restatement
before any time is printed. Traffic = the used bytes of the rows read, the
clock rows, and the used bytes of the rows written (the kept state), over the
median time, and as a fraction of the 8 TB/s HBM peak. One JSON line (also
written to --out)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

BASE, A, CLOCK_SEED = 2000, 16, 0x7C
HBM_PEAK = 8e12  # bytes/s


def populations():
    """kind -> states: the apply bench tools' maps after their op streams."""
    import map_opgen
    import map_orswot_opgen as og
    import nested_opgen as ng
    from map_slab import crdts_ref

    mv = []
    for pre, ops in map_opgen.gen_batch(0xA991, BASE, A):
        m = crdts_ref.Map(crdts_ref.MVReg)
        for op in pre + ops:
            map_opgen.apply_op(m, op)
        mv.append(m)
    orw = []
    for pre, ops in og.gen_batch(0x0A57, BASE, A):
        m = og.new_map()
        for op in pre + ops:
            og.apply_op(m, op)
        orw.append(m)
    nested = [ng.replay(s, ops) for s, ops in ng.gen_batch(0x0A55, BASE, A)]
    return {"mvreg": mv, "orswot": orw, "nested": nested}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-obj", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="mvreg,orswot,nested")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import map_truncgen as tg

    if not torch.cuda.is_available():
        raise SystemExit("map_truncate_bench: no GPU visible")
    reps = max(1, a.n_obj // BASE)
    n = reps * BASE
    eng = crdts_hip.Engine(0)
    rep = lambda v: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()  # noqa: E731

    def rebuild(kind, X, arrs, inner=None):
        if kind == "mvreg":
            return crdts_hip.MapSlab(arrs, X.kcap, X.mcap, X.dcap, X.scap)
        if kind == "orswot":
            return crdts_hip.MapOrswotSlab(arrs, X.caps)
        return crdts_hip.MapMapSlab(arrs, X.kcap, X.dcap, X.scap, crdts_hip.MapSlab(inner, *X.inner_caps))

    def mapped(kind, X, fn, fn_inner=None):
        return rebuild(kind, X, {f: fn(v) for f, v in X.a.items()},
                       {f: (fn_inner or fn)(v) for f, v in X.inner.a.items()} if kind == "nested" else None)

    def tile(kind, X, t):
        k = X.kcap if kind == "nested" else 1
        return mapped(kind, X, lambda v: v[t * BASE:(t + 1) * BASE], lambda v: v[t * BASE * k:(t + 1) * BASE * k])

    def same(kind, got, exp):
        g, e = got.canonical(), exp.canonical()
        pairs = [(g.a, e.a)] + ([(g.inner.a, e.inner.a)] if kind == "nested" else [])
        return all(bool((np.asarray(x[f]) == np.asarray(y[f])).all()) for x, y in pairs for f in y)

    res = {"tool": "map_truncate_bench", "n_obj": n, "A": A, "rounds": a.rounds, "clock_mode": "mixed",
           "hbm_peak_TB_per_s": HBM_PEAK / 1e12, "types": {}}
    for kind, states in populations().items():
        if kind not in a.kinds.split(","):
            continue
        caps = tg.KINDS[kind]["caps"](states)  # the population's own largest sizes
        _, clocks = tg.draw(CLOCK_SEED, states, A, modes=("mixed",))
        pack = tg.KINDS[kind]["pack"]
        S = pack(states, A, caps)
        E = pack([tg.truncated(m, T) for m, T in zip(states, clocks)], A, caps)
        k = S.kcap if kind == "nested" else 1
        # the partner of object i: object i - 1 (a nested map's inner maps with it)
        O = mapped(kind, S, lambda v: np.roll(v, 1, axis=0), lambda v: np.roll(v, k, axis=0))
        dS, dO = mapped(kind, S.to("cuda"), rep), mapped(kind, O.to("cuda"), rep)
        rows = rep(torch.from_numpy(tg.clock_rows(clocks, A).view(np.int64)).cuda())
        trunc = {"mvreg": eng.map_mvreg_truncate, "orswot": eng.map_orswot_truncate, "nested": eng.map_map_truncate}[kind]
        merge = {"mvreg": eng.map_mvreg_merge, "orswot": eng.map_orswot_merge, "nested": eng.map_map_merge}[kind]
        out_t = trunc(dS, rows, A)
        out_m = merge(dS, dO, A)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        t_tr, t_mg = [], []
        for r in range(a.warmup + a.rounds):
            for which in ("truncate", "merge"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                if which == "truncate":
                    trunc(dS, rows, A, out=out_t, stream=s, check_status=False)
                else:
                    merge(dS, dO, A, out=out_m, stream=s, check_status=False)
                e1.record(s)
                s.synchronize()
                eng.status(s)
                if r >= a.warmup:
                    (t_tr if which == "truncate" else t_mg).append(e0.elapsed_time(e1))
        for t in (0, reps - 1):  # the first and the last tile against the restatement, before any time is printed
            if not same(kind, tile(kind, out_t, t), E):
                raise SystemExit(f"map_truncate_bench: {kind}: tile {t} differs from the Python restatement")
        # used bytes: the tiles are copies of the base rows
        b_read = reps * (S.used_bytes() + BASE * A * 8)
        b_kept = reps * E.used_bytes()
        b_merge = reps * (S.used_bytes() + O.used_bytes() + tile(kind, out_m, 0).used_bytes())
        mt, mm = float(np.median(t_tr)), float(np.median(t_mg))
        res["types"][kind] = {
            "caps": [list(c) for c in caps] if kind == "nested" else (caps if kind == "orswot" else list(caps)),
            "exact": True,
            "truncate": {"median_ms": round(mt, 4), "min_ms": round(float(np.min(t_tr)), 4),
                         "max_ms": round(float(np.max(t_tr)), 4), "M_maps_per_s": round(n / mt / 1e3, 2),
                         "read_bytes": b_read, "kept_bytes": b_kept,
                         "GB_per_s": round((b_read + b_kept) / mt / 1e6, 2),
                         "fraction_of_hbm_peak": round((b_read + b_kept) / (mt * 1e-3) / HBM_PEAK, 4)},
            "merge": {"median_ms": round(mm, 4), "min_ms": round(float(np.min(t_mg)), 4),
                      "max_ms": round(float(np.max(t_mg)), 4), "M_maps_per_s": round(n / mm / 1e3, 2),
                      "used_bytes": b_merge, "GB_per_s": round(b_merge / mm / 1e6, 2)},
            "truncate_over_merge": round(mt / mm, 3)}
        del dS, dO, out_t, out_m
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
