#!/usr/bin/env python3
"""Timing of the value of Map::get for Map<u64, Orswot> (crdt_map_orswot_get_sizes
/ crdt_map_orswot_get: slab values -> Orswot records) and for the nested map
(crdt_map_map_get: inner maps -> Map<u64, MVReg> slab rows; read.hip), beside
one merge of the same maps and beside crdt_map_mvreg_get, in the same process.

The maps are the map benches' own: tools/map_orswot_apply_bench.py's start
states (tests/map_orswot_opgen.py, 2,000 objects at A = 16, capacities 4),
tools/map_map_apply_bench.py's (tests/nested_opgen.py) and tools/read_bench.py's
Map<u64, MVReg> maps, each tiled to --n-maps. Every present key is queried
once. Every call is timed with device events after a warm-up, in rounds that
run each call once in an order drawn anew per round, on preallocated outputs;
the records are placed once by an exclusive scan (not timed). The first tile's
answers are checked against tests/map_get_ref.py before any time is printed.

Per call: median / min / max ms, queries per second, the algorithmic bytes —
the used slab bytes the call reads (the located values by their counts, the
key rows, the query words) plus the bytes it writes — over the median and as
a fraction of 8 TB/s, the ratio to one merge of the same maps (the partner of
a map is its neighbour), and the ratio to crdt_map_mvreg_get on the Map<u64,
MVReg> maps, whole and per query. One JSON line (also written to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

BASE, A = 2000, 16
HEAD = 256  # maps of the first tile checked against the restatement
HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-maps", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import map_get_ref as G
    import map_opgen
    import map_orswot_opgen as og
    import map_slab
    import nested_opgen as ng
    from crdts_hip._lib import lib
    from map_slab import crdts_ref

    if not torch.cuda.is_available():
        raise SystemExit("map_get_bench: no GPU visible")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    st = eng._stream(s)
    reps = max(1, a.n_maps // BASE)
    n = reps * BASE
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rep = lambda v: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()  # noqa: E731

    def timed(calls):
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        order = np.random.default_rng(0x6E7)
        for r in range(a.warmup + a.rounds):
            for k in order.permutation(list(calls)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                rc = calls[k]()
                e1.record(s)
                s.synchronize()
                if rc not in (None, 0):
                    raise SystemExit(f"map_get_bench: {k} returned {rc}")
                eng.status(s)
                if r >= a.warmup:
                    t[k].append(e0.elapsed_time(e1))
        return t

    def entry(ms, n_q, nbytes, merge_ms):
        med = float(np.median(ms))
        e = {"median_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
             "M_queries_per_s": round(n_q / med / 1e3, 2), "ns_per_query": round(med * 1e6 / n_q, 2),
             "bytes": int(nbytes), "GB_per_s": round(nbytes / med / 1e6, 2),
             "fraction_of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
        if merge_ms is not None:
            e["over_merge"] = round(med / float(np.median(merge_ms)), 3)
        return e

    def every_present_key(a_keys, a_n):
        """One KEY query per present key of the base maps, tiled: (queries, per base map lists, n_q of a tile)."""
        nk = a_n.astype(np.int64)
        keys = np.concatenate([a_keys[i, :k] for i, k in enumerate(nk)]) if nk.sum() else np.zeros(0, np.uint64)
        ends = np.cumsum(nk).astype(np.uint64)
        nq = int(nk.sum())
        q = crdts_hip.ReadQueries.from_arrays(
            np.concatenate([ends + np.uint64(r * nq) for r in range(reps)]), np.zeros(nq * reps, np.uint32),
            np.tile(keys, reps))
        return q, nq

    res = {"tool": "map_get_bench", "n_maps": n, "A": A, "rounds": a.rounds, "warmup": a.warmup,
           "hbm_peak_TB_per_s": HBM_PEAK / 1e12}

    # ------------------------------------------------------------------ Map<u64, MVReg>: the yardstick
    caps_mv = (4, 4, 4, 4)
    M = crdts_hip.MapSlab.alloc(BASE, A, *caps_mv)
    for i, (pre, _) in enumerate(map_opgen.gen_batch(0xA991, BASE, A)):
        m = crdts_ref.Map(crdts_ref.MVReg)
        for op in pre:
            map_opgen.apply_op(m, op)
        map_slab.mvreg_map_to_row(m, M, i, A)
    dM = crdts_hip.MapSlab({f: rep(v) for f, v in M.to("cuda").a.items()}, *caps_mv)
    q_mv, nq_mv = every_present_key(M.a["keys"], M.a["n_keys"])
    g_out = eng.map_mvreg_get(dM, q_mv, A)
    t = timed({"get": lambda: eng.map_mvreg_get(dM, q_mv, A, out=g_out, stream=s, check_status=False) and None})
    mv_ms = float(np.median(t["get"]))
    vals = int(M.a["mv_n"][np.arange(4)[None, :] < M.a["n_keys"][:, None]].sum())
    mv_bytes = reps * ((4 + 8 * 4 + 8) * BASE + 12 * nq_mv + 4 * nq_mv + 8 * (A + 1) * vals +
                       (4 + 8 * (A + 1) * caps_mv[1]) * nq_mv)  # the whole zero-filled output row is written
    res["map_mvreg_get"] = dict(entry(t["get"], nq_mv * reps, mv_bytes, None), n_queries=nq_mv * reps)
    del dM, g_out

    def against_mvreg(e, n_q):
        e["over_map_mvreg_get"] = round(e["median_ms"] / mv_ms, 3)
        e["over_map_mvreg_get_per_query"] = round(e["median_ms"] / n_q / (mv_ms / (nq_mv * reps)), 3)
        return e

    # ------------------------------------------------------------------ Map<u64, Orswot>
    caps = og.caps(4)
    S = crdts_hip.MapOrswotSlab.alloc(BASE, A, **caps)
    for i, (pre, _) in enumerate(og.gen_batch(0x0A57, BASE, A)):
        m = og.new_map()
        for op in pre:
            og.apply_op(m, op)
        map_slab.orswot_map_to_row(m, S, i, A)
    O = crdts_hip.MapOrswotSlab({f: np.roll(v, 1, axis=0) for f, v in S.a.items()}, caps)
    tiled = lambda X: crdts_hip.MapOrswotSlab({f: rep(v) for f, v in X.to("cuda").a.items()}, X.caps)  # noqa: E731
    dS, dO = tiled(S), tiled(O)
    q, nq = every_present_key(S.a["keys"], S.a["n_keys"])
    batch, present = eng.map_orswot_get(dS, q, A)
    exp = [G.orswot_value_record(S, i, k, A) for i in range(HEAD) for k in range(int(S.a["n_keys"][i]))]
    off0 = batch.off[: nq + 1].cpu().tolist() + [batch.bytes]
    head = batch.base[: off0[len(exp)]].cpu().numpy()
    if any(head[o:o + len(e)].tobytes() != e for o, e in zip(off0, exp)) or not bool(present.all()):
        raise SystemExit("map_get_bench: the records differ from tests/map_get_ref.py")
    rec_bytes = off0[nq]  # one tile's records: the next tile starts there
    sizes = torch.empty(q.n_q, dtype=torch.int64, device="cuda")
    pres = torch.empty(q.n_q, dtype=torch.int32, device="cuda")
    cs, cq = dS.cstruct(), q.cqueries()
    out_m = eng.map_orswot_merge(dS, dO, A)
    calls = {
        "sizes": lambda: lib.crdt_map_orswot_get_sizes(eng.ctx, C.byref(cs), C.byref(cq), n, A, p(sizes), p(pres), st),
        "write": lambda: lib.crdt_map_orswot_get(eng.ctx, C.byref(cs), C.byref(cq), n, A, p(batch.base), p(batch.off),
                                                 batch.bytes, st),
        "merge": lambda: eng.map_orswot_merge(dS, dO, A, out=out_m, stream=s, check_status=False) and None}
    t = timed(calls)
    h = S.a
    used = np.arange(4)[None, :] < h["n_keys"][:, None]
    nm, nd = h["vn_mem"][used].astype(np.int64), h["vn_def"][used].astype(np.int64)
    sets = int(h["vdset_n"][used][np.arange(4)[None, :] < h["vn_def"][used][:, None]].sum())
    rows = (4 + 8 * 4 + 8) * BASE + 12 * nq  # n_keys, keys, obj_end per map; kind, key per query
    counted = 8 * nq + 8 * A * int(nm.sum()) + 8 * A * int(nd.sum()) + 4 * int(nd.sum())  # what both calls count
    b_sizes = reps * (rows + counted + 12 * nq)
    b_write = reps * (rows + counted + 8 * nq + 8 * A * nq + 8 * int(nm.sum()) + 4 * int(nd.sum()) + 8 * sets +
                      rec_bytes)
    sub = lambda X: crdts_hip.MapOrswotSlab({f: v[:BASE] for f, v in X.a.items()}, X.caps)  # noqa: E731
    b_merge = reps * (S.used_bytes() + O.used_bytes() + sub(out_m).used_bytes())
    both = [x + y for x, y in zip(t["sizes"], t["write"])]
    res["map_orswot"] = {
        "caps": caps, "n_queries": nq * reps, "record_bytes": rec_bytes * reps, "exact": True,
        "members_per_value": round(float(nm.mean()), 2), "deferred_per_value": round(float(nd.mean()), 3),
        "merge": dict(entry(t["merge"], n, b_merge, None),
                      bytes_model="used bytes of both inputs and the output (MapOrswotSlab.used_bytes)"),
        "get_sizes": against_mvreg(entry(t["sizes"], nq * reps, b_sizes, t["merge"]), nq * reps),
        "get_write": against_mvreg(entry(t["write"], nq * reps, b_write, t["merge"]), nq * reps),
        "get_sizes_plus_write": against_mvreg(entry(both, nq * reps, b_sizes + b_write, t["merge"]), nq * reps)}
    del dS, dO, out_m, batch, calls

    # ------------------------------------------------------------------ the nested map
    _, N, _ = ng.reference(0x0A55, BASE, A)
    mk = lambda X, arrs, inner: crdts_hip.MapMapSlab(arrs, X.kcap, X.dcap, X.scap, crdts_hip.MapSlab(  # noqa: E731
        inner, X.inner.kcap, X.inner.mcap, X.inner.dcap, X.inner.scap))
    P = mk(N, {f: np.roll(v, 1, axis=0) for f, v in N.a.items()},
           {f: np.roll(v, N.kcap, axis=0) for f, v in N.inner.a.items()})

    def tiled_nested(X):
        d = X.to("cuda")
        return mk(X, {f: rep(v) for f, v in d.a.items()}, {f: rep(v) for f, v in d.inner.a.items()})

    dN, dP = tiled_nested(N), tiled_nested(P)
    q, nq = every_present_key(N.a["keys"], N.a["n_keys"])
    rows_out, present = eng.map_map_get(dN, q, A)
    H = crdts_hip.MapSlab({f: v[: int(N.a["n_keys"][:HEAD].sum())] for f, v in rows_out.a.items()},
                          *N.inner_caps).host()
    j = 0
    for i in range(HEAD):
        for k in range(int(N.a["n_keys"][i])):
            if map_slab.mvreg_map_from_row(H, j) != G.inner_map_row(N, i, k):
                raise SystemExit(f"map_get_bench: row {j} differs from tests/map_get_ref.py")
            j += 1
    cn, cq, co = dN.cstruct(), q.cqueries(), rows_out.cstruct()
    out_m = eng.map_map_merge(dN, dP, A)
    calls = {"get": lambda: lib.crdt_map_map_get(eng.ctx, C.byref(cn), C.byref(cq), n, A, C.byref(co), p(present), st),
             "merge": lambda: eng.map_map_merge(dN, dP, A, out=out_m, stream=s, check_status=False) and None}
    t = timed(calls)
    outer_used = np.arange(N.kcap)[None, :] < N.a["n_keys"][:, None]
    inner_used = int(sum(int(m.reshape(m.shape[0], -1)[outer_used.reshape(-1)].sum()) * N.inner.a[f].dtype.itemsize
                         for f, m in N.inner.used_masks().items()))
    b_get = reps * ((4 + 8 * N.kcap + 8) * BASE + 12 * nq + 2 * inner_used + 4 * nq)
    tile0 = mk(out_m, {f: v[:BASE] for f, v in out_m.a.items()},
               {f: v[:BASE * out_m.kcap] for f, v in out_m.inner.a.items()})
    b_merge = reps * (N.used_bytes() + P.used_bytes() + tile0.used_bytes())
    res["map_map"] = {
        "caps": [list(ng.IN_CAPS), list(ng.IN_INNER)], "n_queries": nq * reps, "exact": True,
        "inner_used_bytes_per_query": round(inner_used / nq, 1),
        "merge": dict(entry(t["merge"], n, b_merge, None),
                      bytes_model="used bytes of both inputs and the output (MapMapSlab.used_bytes)"),
        "get": against_mvreg(entry(t["get"], nq * reps, b_get, t["merge"]), nq * reps)}
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
