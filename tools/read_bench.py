#!/usr/bin/env python3
"""Timing of the batched read path (read.hip: crdt_orswot_read*, crdt_map_read*,
crdt_map_mvreg_get) beside one merge of the same objects, in the same process.

(a) The config-3 Orswot batch (generate_orswot, --n-obj objects), four
    `contains` per object — three present members (first, middle, last) and one
    absent — with the rm group only (the contains -> Rm path: the top clock is
    never read); the same with the add group and an actor; and one `value()`
    per object. Beside crdt_orswot_merge of the batch with its other side.
(b) tools/map_apply_bench.py's maps (tests/map_opgen.py's 2,000 objects, A = 16,
    tiled to --n-maps) with eight `get`s per map (its four keys twice, each
    with an actor), through crdt_map_read_sizes / crdt_map_read and through
    crdt_map_mvreg_get. Beside crdt_map_mvreg_merge of the maps with the rows
    shifted by one object.

Every call is timed with device events after a warm-up, in rounds that run
each call once in an order drawn anew per round, on preallocated outputs. The
answers of the first objects are checked against tests/read_ref.py before any
time is printed. Each entry gives the median / min / max time, queries per
second, the ratio to the merge's median, the algorithmic bytes of the call —
object headers and query words, the object's key lines (its key section in
64-B lines, once per object), the mem_dend words and the runs read, the
outputs written — and those bytes over the median. One JSON line (also written
to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

HEAD = 256  # objects checked against the reference
BASE, MAP_A, MAP_CAPS = 2000, 16, (4, 4, 4, 4)
ABSENT = 1 << 40  # config 3's members are below 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-obj", type=int, default=1_000_000)
    ap.add_argument("--n-maps", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import map_opgen
    import map_slab
    import read_ref
    import records
    from crdts_hip._lib import READ_SIZES_FIELDS, ReadOutC, ReadSizesC, lib
    from map_slab import crdts_ref

    if not torch.cuda.is_available():
        raise SystemExit("read_bench: no GPU visible")
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    st = eng._stream(s)

    def timed(calls):
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        order = np.random.default_rng(0x0DE5)
        for r in range(a.warmup + a.rounds):
            for k in order.permutation(list(calls)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                rc = calls[k]()
                e1.record(s)
                s.synchronize()
                if rc not in (None, 0):
                    raise SystemExit(f"read_bench: {k} returned {rc}")
                eng.status(s)
                if r >= a.warmup:
                    t[k].append(e0.elapsed_time(e1))
        return t

    def entry(ms, n_q, nbytes, merge_ms):
        med = float(np.median(ms))
        e = {"median_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
             "bytes": int(nbytes), "GB_per_s": round(nbytes / med / 1e6, 2)}
        if n_q:
            e["M_queries_per_s"] = round(n_q / med / 1e3, 2)
        if merge_ms is not None:
            e["over_merge"] = round(med / float(np.median(merge_ms)), 3)
        return e

    def calls_of(res, q, sizes_fn, write_fn):
        """The two calls of one read on the tensors of its first (checked) run."""
        cq = q.cqueries()
        z = ReadSizesC(*[res[f].data_ptr() if f in res else None for f in READ_SIZES_FIELDS])
        o = ReadOutC()
        for g in ("add", "rm", "list"):
            if g + "_end" in res:
                setattr(o, g + "_end", res[g + "_end"].data_ptr())
                setattr(o, "n_" + g, int(res[g + "_end"][-1].item()))
                for f in (("list_key",) if g == "list" else (g + "_act", g + "_ctr")):
                    setattr(o, f, res[f].data_ptr() if res[f].numel() else None)
        keep = (cq, z, o)
        return (lambda: sizes_fn(C.byref(cq), C.byref(z), st)), (lambda: write_fn(C.byref(cq), C.byref(o), st)), keep

    def head_of(res, k):
        """The per-query tensors cut to the first k queries (the pair arrays stay whole)."""
        return {f: (v if f.endswith(("_act", "_ctr", "_key")) else v[:k]) for f, v in res.items()}

    def total(res, g):
        return int(res[g + "_end"][-1].item()) if g + "_end" in res else 0

    res = {"tool": "read_bench", "rounds": a.rounds, "warmup": a.warmup}

    # ------------------------------------------------------------------ (a) Orswot, config 3
    n, A = a.n_obj, crdts_hip.CONFIG3["n_actors"]
    (lb, lo), (rb, ro) = crdts_hip.generate_orswot(n, threads=16)
    L, R = crdts_hip.OrswotBatch.from_host(lb, lo, A), crdts_hip.OrswotBatch.from_host(rb, ro, A)
    w32, w64 = lb[: lb.size // 8 * 8].view(np.uint32), lb[: lb.size // 8 * 8].view(np.uint64)
    o32, k0 = (lo // 4).astype(np.int64), ((lo + 32 + 8 * A) // 8).astype(np.int64)
    n_mem = w32[o32 + 2].astype(np.int64)
    pick = lambda idx: np.where(n_mem > 0, w64[np.minimum(k0 + idx, w64.size - 1)], np.uint64(ABSENT))  # noqa: E731
    keys = np.stack([pick(0), pick(n_mem // 2), pick(np.maximum(n_mem - 1, 0)),
                     np.full(n, ABSENT, np.uint64)], 1).reshape(-1)
    ends4 = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(4)
    actor4 = (np.arange(4 * n, dtype=np.uint64) % np.uint64(A)).astype(np.uint32)
    RQ = crdts_hip.ReadQueries
    q_rm = RQ.from_arrays(ends4, np.zeros(4 * n, np.uint32), keys)
    q_add = RQ.from_arrays(ends4, np.zeros(4 * n, np.uint32), keys, actor4)
    q_all = RQ.from_arrays(np.arange(1, n + 1, dtype=np.uint64), np.ones(n, np.uint32), np.zeros(n, np.uint64))
    b = L.cbatch()
    sz = lambda q, z, x: lib.crdt_orswot_read_sizes(eng.ctx, C.byref(b), q, A, 0, z, x)  # noqa: E731
    wr = lambda q, o, x: lib.crdt_orswot_read(eng.ctx, C.byref(b), q, A, 0, o, x)  # noqa: E731
    runs = {"contains_rm": (q_rm, ("val", "rm")), "contains_add_rm": (q_add, ("val", "dot", "add", "rm")),
            "value": (q_all, ("val", "list"))}
    h = min(HEAD, n)
    head = []
    for r in records.unpack_batch(lb, lo[:h]):
        d = records.decode(r)
        x = crdts_ref.Orswot()
        x.clock = crdts_ref.VClock(d["clock"])
        x.entries = {m: crdts_ref.VClock(c) for m, c in d["entries"].items()}
        head.append(x)
    first, calls, keep = {}, {}, []
    for name, (q, want) in runs.items():
        first[name] = eng.orswot_read(L, q, want=want)
        per = q.n_q // n
        ka, aa = q.t[2][: per * h].cpu().numpy().view(np.uint64), None if q.t[3] is None else q.t[3][: per * h].cpu().numpy()
        per_obj = [[("all",) if name == "value" else ("key", int(ka[i * per + j]), None if aa is None else int(aa[i * per + j]))
                    for j in range(per)] for i in range(h)]
        got = read_ref.answers(head_of(first[name], per * h), per * h)
        read_ref.assert_answers(got, read_ref.expect(head, per_obj, A), f"read_bench {name}")
        calls[name + "_sizes"], calls[name + "_write"], k = calls_of(first[name], q, sz, wr)
        keep.append(k)
    mout = eng.orswot_merge(L, R)
    calls["merge"] = lambda: eng.orswot_merge(L, R, out=mout, stream=s, check_status=False) and None
    t = timed(calls)
    key_lines = int(((8 * n_mem + 63) // 64 * 64).sum())
    present = int((keys.reshape(n, 4)[:, :3] != np.uint64(ABSENT)).sum())
    hdr = (32 + 8) * n  # header + obj_end
    out = {"n_obj": n, "queries_per_object": 4, "members_mean": round(float(n_mem.mean()), 2),
           "merge": entry(t["merge"], 0, L.compact_bytes() + R.compact_bytes() + mout.compact_bytes(), None)}
    out["merge"]["bytes_model"] = "compact bytes of both inputs and the output (SURVEY.md 8(d))"
    for name, (q, want) in runs.items():
        nq, r0 = q.n_q, first[name]
        # header + obj_end per object, kind + key (+ actor) per query; a contains probes the object's key lines
        # and reads the member's two mem_dend words; value() reads no key before the write call lists them
        common = hdr + nq * (12 + (4 if q.t[3] is not None else 0)) + (key_lines if name != "value" else 0)
        dend = 8 * present if name != "value" else 0
        top = 8 * A * nq if "add" in want else (8 * nq if "dot" in want else 0)  # the dense row, or the actor's word
        pa, pr, lst = total(r0, "add"), total(r0, "rm"), total(r0, "list")
        sizes_out = sum(8 if f in ("val", "dot") else 4 for f in want) * nq
        groups = sum(1 for g in ("add", "rm", "list") if g in want)
        out[name + "_sizes"] = entry(t[name + "_sizes"], nq, common + dend + top + sizes_out, t["merge"])
        # the write call: the same reads, 8 B of *_end per group and query, rm pairs read and written (24 B),
        # add pairs written (12 B; their row is in `top`), listed keys read and written (16 B)
        out[name + "_write"] = entry(t[name + "_write"], nq,
                                     common + dend + top + 8 * groups * nq + 24 * pr + 12 * pa + 16 * lst, t["merge"])
        out[name + "_write"].update(pairs_written=pa + pr, keys_listed=lst)
    res["orswot_config3"] = out
    del L, R, mout, first, calls, keep

    # ------------------------------------------------------------------ (b) Map<u64, MVReg>
    reps = max(1, a.n_maps // BASE)
    n = reps * BASE
    batch = map_opgen.gen_batch(0xA991, BASE, MAP_A)
    S = crdts_hip.MapSlab.alloc(BASE, MAP_A, *MAP_CAPS)
    maps = []
    for i, (pre, _) in enumerate(batch):
        m = crdts_ref.Map(crdts_ref.MVReg)
        for op in pre:
            map_opgen.apply_op(m, op)
        map_slab.mvreg_map_to_row(m, S, i, MAP_A)
        maps.append(m)
    O = crdts_hip.MapSlab({f: np.roll(v, 1, axis=0) for f, v in S.a.items()}, *MAP_CAPS)

    def tiled(X):
        d = X.to("cuda")
        return crdts_hip.MapSlab({f: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous() for f, v in d.a.items()},
                                 X.kcap, X.mcap, X.dcap, X.scap)

    dS, dO = tiled(S), tiled(O)
    G = 8
    per_map = [("key", map_opgen.KEYS[j % 4], j % MAP_A) for j in range(G)]
    q = RQ.from_arrays(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(G), np.zeros(G * n, np.uint32),
                       np.tile(np.array([k for _, k, _ in per_map], np.uint64), n),
                       np.tile(np.array([x for _, _, x in per_map], np.uint32), n))
    want = ("val", "slot", "dot", "add", "rm")
    r0 = eng.map_read(dS, q, MAP_A, want=want)
    got = read_ref.answers(head_of(r0, G * h), G * h)
    read_ref.assert_answers(got, read_ref.expect(maps[:h], [per_map] * h, MAP_A, read_ref.map_query), "read_bench map")
    v = dS.read_view()
    msz = lambda qq, z, x: lib.crdt_map_read_sizes(eng.ctx, C.byref(v), qq, n, MAP_A, z, x)  # noqa: E731
    mwr = lambda qq, o, x: lib.crdt_map_read(eng.ctx, C.byref(v), qq, n, MAP_A, o, x)  # noqa: E731
    c_sizes, c_write, keep = calls_of(r0, q, msz, mwr)
    g_out = eng.map_mvreg_get(dS, q, MAP_A)
    gn = g_out[0][: G * h].cpu().numpy()
    exp_n = [len(read_ref.mvreg_get(m, x)) for m in maps[:h] for x in per_map]
    if gn.tolist() != exp_n:
        raise SystemExit("read_bench: map_mvreg_get differs from the reference")
    m_out = eng.map_mvreg_merge(dS, dO, MAP_A)
    calls = {"map_read_sizes": c_sizes, "map_read_write": c_write,
             "map_mvreg_get": lambda: eng.map_mvreg_get(dS, q, MAP_A, out=g_out, stream=s, check_status=False) and None,
             "merge": lambda: eng.map_mvreg_merge(dS, dO, MAP_A, out=m_out, stream=s, check_status=False) and None}
    t = timed(calls)
    nq = q.n_q
    hits = int(r0["val"].sum().item())
    row = (8 * MAP_A + 4 + 8 * MAP_CAPS[0] + 8) * n  # map clock, n_keys, keys, obj_end
    common = row + 16 * nq
    sizes_b = common + 8 * MAP_A * hits + 28 * nq
    pairs = total(r0, "add") + total(r0, "rm")
    write_b = common + 8 * MAP_A * hits + 16 * nq + 12 * pairs  # entry rows, two *_end words, the pairs written
    vals = int(g_out[0].sum().item())
    get_b = (4 + 8 * MAP_CAPS[0] + 8) * n + 12 * nq + 4 * hits + 8 * (MAP_A + 1) * vals + \
        (4 + 8 * (MAP_A + 1) * MAP_CAPS[1]) * nq
    sub = lambda X, k: crdts_hip.MapSlab({f: x[:k] for f, x in X.a.items()}, X.kcap, X.mcap, X.dcap, X.scap)  # noqa: E731
    b_merge = reps * (S.used_bytes() + O.used_bytes() + sub(m_out, BASE).used_bytes())
    res["map_mvreg"] = {"n_maps": n, "A": MAP_A, "caps": list(MAP_CAPS), "gets_per_map": G, "present": hits,
                        "merge": entry(t["merge"], 0, b_merge, None),
                        "map_read_sizes": entry(t["map_read_sizes"], nq, sizes_b, t["merge"]),
                        "map_read_write": entry(t["map_read_write"], nq, write_b, t["merge"]),
                        "map_mvreg_get": entry(t["map_mvreg_get"], nq, get_b, t["merge"])}
    res["map_mvreg"]["merge"]["bytes_model"] = "used bytes of both inputs and the output (MapSlab.used_bytes)"
    res["map_mvreg"]["map_read_write"]["pairs_written"] = pairs
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    del keep


if __name__ == "__main__":
    main()
