#!/usr/bin/env python3
"""Timing of the bincode codec of Map<u64, Orswot> and of the nested map
Map<u64, Map<u64, MVReg>> (crdt_map_orswot_from_bincode / _bincode_sizes /
_to_bincode and the crdt_map_map_* three) beside one merge of the same maps,
in the same process — the method of tools/map_bincode_bench.py.

The maps are tools/map_orswot_apply_bench.py's and tools/map_map_apply_bench.py's
populations after their op streams (2,000 generated objects each at A = 16),
tiled to --n-maps maps, in slabs of the states' own largest counts. Blobs are
the format restatement's (tests/nested_bincode_ref.py: u8 actors, u64 keys,
members, inner keys and values; every unordered container shuffled), packed
back to back with 0-5 junk bytes between them. Ingest is one launch; egest is
the sizes launch and the write launch, timed separately on blobs placed once
by an exclusive scan (the scan is not timed). Every call is timed with device
events around its launch after a warm-up, alternating, on preallocated
outputs; the merge takes the same slab against itself shifted by one object.
The ingested slab's and the written blobs' first and last tiles are checked
against the restatement before any time is printed. Bytes moved = blob bytes +
used slab bytes (used_bytes()), over the median time and as a fraction of
8 TB/s. One JSON line (also written to --out)."""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

A, BASE = 16, 2000
HBM_PEAK = 8e12  # bytes/s


def pack(blobs, rng):
    """-> (bytes, offsets, lengths): back to back with 0-5 junk bytes between the blobs."""
    buf, off = bytearray(), []
    for b in blobs:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(6)))
        off.append(len(buf))
        buf += b
    return bytes(buf), off, [len(b) for b in blobs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-maps", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import map_orswot_opgen as og
    import map_slab
    import map_truncgen
    import nested_bincode_ref as NB
    import nested_opgen as ng

    if not torch.cuda.is_available():
        raise SystemExit("nested_bincode_bench: no GPU visible")
    C, lib = crdts_hip.C, crdts_hip.lib
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    st = eng._stream(s)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda:0")  # noqa: E731
    reps = max(1, a.n_maps // BASE)
    n = reps * BASE

    def timed(calls):
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
        return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                    "max_ms": round(float(np.max(v)), 4)} for k, v in times.items()}

    def rates(t, nbytes):
        ms = t["median_ms"]
        return dict(t, M_maps_per_s=round(n / ms / 1e3, 3), bytes_moved=nbytes, GB_per_s=round(nbytes / ms / 1e6, 2),
                    fraction_of_8TBps=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4))

    def blobs_of(out, off, lens, lo, hi):
        o, ln = off[lo:hi].cpu().numpy(), lens[lo:hi].cpu().numpy()
        h = out[int(o[0]):int(o[-1] + ln[-1])].cpu().numpy()  # the tile's bytes only
        return [h[x - o[0]:x - o[0] + y].tobytes() for x, y in zip(o, ln)]

    rep = lambda v: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()  # noqa: E731
    res = {"tool": "nested_bincode_bench", "A": A, "rounds": a.rounds, "warmup": a.warmup,
           "hbm_peak_TB_per_s": HBM_PEAK / 1e12}

    def run(kind, states, w, enc):
        orswot = kind == "map_orswot"
        caps = map_truncgen.KINDS["orswot" if orswot else "nested"]["caps"](states)
        if orswot:
            E = crdts_hip.MapOrswotSlab.alloc(BASE, A, **caps)
            for i, m in enumerate(states):
                map_slab.orswot_map_to_row(m, E, i, A, zero=False)
            mk = lambda arrs, inner=None: crdts_hip.MapOrswotSlab(arrs, caps)  # noqa: E731
            new = lambda cnt: crdts_hip.MapOrswotSlab.alloc(cnt, A, device="cuda:0", **caps)  # noqa: E731
        else:
            E = ng.pack(states, A, *caps)
            mk = lambda arrs, inner: crdts_hip.MapMapSlab(arrs, *caps[0], crdts_hip.MapSlab(inner, *caps[1]))  # noqa: E731
            new = lambda cnt: crdts_hip.MapMapSlab.alloc(cnt, A, *caps[0], caps[1], device="cuda:0")  # noqa: E731
        d = E.to("cuda:0")
        # tiles of the nested map's inner rows: BASE * kcap rows per tile, so a whole-array repeat keeps i * kcap + k
        dE = mk({f: rep(v) for f, v in d.a.items()}, None if orswot else {f: rep(v) for f, v in d.inner.a.items()})
        kc = 1 if orswot else caps[0][0]
        dO = mk({f: torch.roll(v, 1, 0) for f, v in dE.a.items()},
                None if orswot else {f: torch.roll(v, kc, 0) for f, v in dE.inner.a.items()})
        rng = random.Random(0xB1C)
        buf, off, ln = pack([enc(m, *w, rng=rng) for m in states], random.Random(0xB1D))
        canon = [enc(m, *w) for m in states]
        t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda:0").repeat(reps)
        bo = (i64(off)[None, :] + len(buf) * torch.arange(reps, device="cuda:0")[:, None]).reshape(-1).contiguous()
        bl = i64(ln).repeat(reps)
        blob_bytes = sum(ln) * reps
        out_i = new(n)
        name = "map_orswot" if orswot else "map_map"
        merge = eng.map_orswot_merge if orswot else eng.map_map_merge
        out_m = merge(dE, dO, A)
        r_i, r_e = out_i.cstruct(), dE.cstruct()
        sizes = torch.empty(n, dtype=torch.int64, device="cuda:0")
        lens = (eng.map_orswot_to_bincode if orswot else eng.map_map_to_bincode)(dE, A, *w)[2]
        ends = torch.cumsum(lens, 0)
        eout, eoff = torch.empty(int(ends[-1].item()), dtype=torch.uint8, device="cuda:0"), (ends - lens).contiguous()
        f_in, f_sz, f_wr = (getattr(lib, f"crdt_{name}_{x}") for x in ("from_bincode", "bincode_sizes", "to_bincode"))
        calls = {
            "ingest": lambda: crdts_hip.check(f_in(eng.ctx, p(t), int(t.numel()), p(bo), p(bl), n, *w, A, C.byref(r_i),
                                                   st), "from_bincode"),
            "egest_sizes": lambda: crdts_hip.check(f_sz(eng.ctx, C.byref(r_e), n, A, *w, p(sizes), st), "bincode_sizes"),
            "egest_write": lambda: crdts_hip.check(f_wr(eng.ctx, C.byref(r_e), n, A, *w, p(eout), p(eoff),
                                                        int(eout.numel()), st), "to_bincode"),
            "merge": lambda: merge(dE, dO, A, out=out_m, stream=s, check_status=False),
        }
        tm = timed(calls)
        Ec = E.canonical()
        for lo in (0, n - BASE):  # the first and the last tile, before any time is printed
            tile = mk({f: v[lo:lo + BASE] for f, v in out_i.a.items()},
                      None if orswot else {f: v[lo * kc:(lo + BASE) * kc] for f, v in out_i.inner.a.items()}).canonical()
            same = all(bool((tile.a[f] == Ec.a[f]).all()) for f in Ec.a)
            if not orswot:
                same = same and all(bool((tile.inner.a[f] == Ec.inner.a[f]).all()) for f in Ec.inner.a)
            if not same:
                raise SystemExit(f"nested_bincode_bench: ingested {name} maps at {lo} differ from the restatement")
            if blobs_of(eout, eoff, lens, lo, lo + BASE) != canon or not torch.equal(sizes, lens):
                raise SystemExit(f"nested_bincode_bench: written {name} blobs at {lo} differ from the restatement")
        used = reps * E.used_bytes()
        eg_bytes = reps * sum(map(len, canon)) + used
        eg = {"median_ms": round(tm["egest_sizes"]["median_ms"] + tm["egest_write"]["median_ms"], 4)}
        res[name] = {
            "n_obj": n, "caps": caps if orswot else [list(caps[0]), list(caps[1])], "widths": list(w), "exact": True,
            "blob_bytes": blob_bytes, "used_slab_bytes": used,
            "ingest": rates(tm["ingest"], blob_bytes + used),
            "egest": dict(rates(eg, eg_bytes), sizes=tm["egest_sizes"], write=tm["egest_write"]),
            "merge": dict(tm["merge"], M_maps_per_s=round(n / tm["merge"]["median_ms"] / 1e3, 3)),
            "ingest_over_merge": round(tm["ingest"]["median_ms"] / tm["merge"]["median_ms"], 3),
            "egest_over_merge": round(eg["median_ms"] / tm["merge"]["median_ms"], 3)}

    states = []
    for pre, ops in og.gen_batch(0x0A57, BASE, A):
        m = og.new_map()
        for op in pre + ops:
            og.apply_op(m, op)
        states.append(m)
    run("map_orswot", states, (1, 8, 8), NB.encode_map_orswot)
    torch.cuda.empty_cache()
    run("map_map", [ng.replay(s0, ops) for s0, ops in ng.gen_batch(0x0A55, BASE, A)], (1, 8, 8, 8), NB.encode_map_map)
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
