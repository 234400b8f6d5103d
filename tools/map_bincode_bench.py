#!/usr/bin/env python3
"""Timing of the bincode codec of Map<u64, MVReg> and of the stand-alone MVReg
(crdt_map_mvreg_from_bincode / _bincode_sizes / _to_bincode and the
crdt_mvreg_* three) beside one merge of the same objects, in the same process.

The maps are tools/map_apply_bench.py's population (2,000 generated objects at
A = 16 after the whole op stream, as tools/map_truncate_bench.py takes them),
tiled to --n-maps maps; the registers are tools/mvreg_apply_bench.py's initial
registers (4,000 at A = 16, cap 4), tiled to --n-regs. Blobs are the format
restatement's (tests/map_bincode_ref.py: u8 actors, u64 keys and values; the
maps' deferred clocks shuffled), packed back to back with 0-5 junk bytes
between them. Ingest is one launch; egest is the sizes launch and the write
launch, timed separately on blobs placed once by an exclusive scan (the scan
is not timed). Every call is timed with device events around its launch after
a warm-up, alternating, on preallocated outputs; the merge takes the same
slab against itself shifted by one object. The ingested slab's and the written
blobs' first and last tiles are checked against the restatement before any
time is printed. Bytes moved = blob bytes + used slab bytes (MapSlab.used_bytes;
registers: the used slots and counts; the register ingest also writes its
whole zero-filled block, reported separately), over the median time and as a
fraction of 8 TB/s. One JSON line (also written to --out)."""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-crdt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

A, WA, WK, WV = 16, 1, 8, 8
MAP_BASE, REG_BASE, REG_CAP = 2000, 4000, 4
HBM_PEAK = 8e12  # bytes/s
ORSWOT_CODEC = {"ingest_M_obj_per_s": 466, "egest_M_obj_per_s": 736,
                "note": "the Orswot codec, DESIGN.md §0: other objects, a reference point and not a gate"}


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
    ap.add_argument("--n-regs", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import crdts_hip
    import map_bincode_ref as MB
    import map_opgen
    import map_slab
    import mvreg_opgen as mo
    from map_slab import crdts_ref

    if not torch.cuda.is_available():
        raise SystemExit("map_bincode_bench: no GPU visible")
    C, lib = crdts_hip.C, crdts_hip.lib
    eng = crdts_hip.Engine(0)
    s = torch.cuda.Stream()
    st = eng._stream(s)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda:0")  # noqa: E731

    def tiled_blobs(blobs, reps, seed):
        """The base blobs `reps` times over: (buffer, offsets, lengths) on the device."""
        buf, off, ln = pack(blobs, random.Random(seed))
        t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda:0").repeat(reps)
        o = (i64(off)[None, :] + len(buf) * torch.arange(reps, device="cuda:0")[:, None]).reshape(-1).contiguous()
        return t, o, i64(ln).repeat(reps), sum(ln) * reps

    def timed(calls, rounds, warmup):
        times = {k: [] for k in calls}
        torch.cuda.synchronize()
        for r in range(warmup + rounds):
            for which, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                call()
                e1.record(s)
                s.synchronize()
                eng.status(s)
                if r >= warmup:
                    times[which].append(e0.elapsed_time(e1))
        return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                    "max_ms": round(float(np.max(v)), 4)} for k, v in times.items()}

    def rates(t, n, nbytes):
        ms = t["median_ms"]
        return dict(t, M_obj_per_s=round(n / ms / 1e3, 2), bytes_moved=nbytes, GB_per_s=round(nbytes / ms / 1e6, 2),
                    fraction_of_8TBps=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4))

    def placed(lens):
        ends = torch.cumsum(lens, 0)
        return torch.empty(int(ends[-1].item()), dtype=torch.uint8, device="cuda:0"), (ends - lens).contiguous()

    def blobs_of(out, off, lens, lo, hi):
        o, n = off[lo:hi].cpu().numpy(), lens[lo:hi].cpu().numpy()
        h = out[int(o[0]):int(o[-1] + n[-1])].cpu().numpy()  # the tile's bytes only
        return [h[x - o[0]:x - o[0] + y].tobytes() for x, y in zip(o, n)]

    res = {"tool": "map_bincode_bench", "A": A, "widths": {"actor": WA, "key": WK, "val": WV}, "rounds": a.rounds,
           "hbm_peak_TB_per_s": HBM_PEAK / 1e12, "orswot_codec_reference_point": ORSWOT_CODEC}

    # ------------------------------------------------------------ Map<u64, MVReg>
    states = []
    for pre, ops in map_opgen.gen_batch(0xA991, MAP_BASE, A):
        m = crdts_ref.Map(crdts_ref.MVReg)
        for op in pre + ops:
            map_opgen.apply_op(m, op)
        states.append(m)
    caps = (max(max(len(m.entries) for m in states), 1),
            max(max([len(e[1].vals) for m in states for e in m.entries.values()] + [1]), 1),
            max(max(len(m.deferred) for m in states), 1),
            max(max([len(k) for m in states for k in m.deferred.values()] + [1]), 1))
    reps = max(1, a.n_maps // MAP_BASE)
    n = reps * MAP_BASE
    E = crdts_hip.MapSlab.alloc(MAP_BASE, A, *caps)
    for i, m in enumerate(states):
        map_slab.mvreg_map_to_row(m, E, i, A, zero=False)
    rng = random.Random(0xB1C)
    t, bo, bl, blob_bytes = tiled_blobs([MB.encode_map_mvreg(m, WA, WK, WV, rng=rng) for m in states], reps, 0xB1D)
    canon = [MB.encode_map_mvreg(m, WA, WK, WV) for m in states]
    rep = lambda v: v.repeat((reps,) + (1,) * (v.dim() - 1)).contiguous()  # noqa: E731
    dE = crdts_hip.MapSlab({f: rep(v) for f, v in E.to("cuda:0").a.items()}, *caps)
    dO = crdts_hip.MapSlab({f: torch.roll(v, 1, 0) for f, v in dE.a.items()}, *caps)
    out_i = crdts_hip.MapSlab.alloc(n, A, *caps, device="cuda:0")
    out_m = eng.map_mvreg_merge(dE, dO, A)
    r_i, r_e = out_i.cstruct(), dE.cstruct()
    sizes = torch.empty(n, dtype=torch.int64, device="cuda:0")
    lens = eng.map_mvreg_to_bincode(dE, A, WA, WK, WV)[2]
    eout, eoff = placed(lens)
    calls = {
        "ingest": lambda: crdts_hip.check(lib.crdt_map_mvreg_from_bincode(
            eng.ctx, p(t), int(t.numel()), p(bo), p(bl), n, WA, WK, WV, A, C.byref(r_i), st), "from_bincode"),
        "egest_sizes": lambda: crdts_hip.check(lib.crdt_map_mvreg_bincode_sizes(
            eng.ctx, C.byref(r_e), n, A, WA, WK, WV, p(sizes), st), "bincode_sizes"),
        "egest_write": lambda: crdts_hip.check(lib.crdt_map_mvreg_to_bincode(
            eng.ctx, C.byref(r_e), n, A, WA, WK, WV, p(eout), p(eoff), int(eout.numel()), st), "to_bincode"),
        "merge": lambda: eng.map_mvreg_merge(dE, dO, A, out=out_m, stream=s, check_status=False),
    }
    tm = timed(calls, a.rounds, a.warmup)
    for lo in (0, n - MAP_BASE):  # the first and the last tile, before any time is printed
        tile = crdts_hip.MapSlab({f: v[lo:lo + MAP_BASE] for f, v in out_i.a.items()}, *caps).canonical()
        if not all(bool((tile.a[f] == E.a[f]).all()) for f in E.a):
            raise SystemExit(f"map_bincode_bench: ingested maps at {lo} differ from the restatement")
        if blobs_of(eout, eoff, lens, lo, lo + MAP_BASE) != canon or not torch.equal(sizes, lens):
            raise SystemExit(f"map_bincode_bench: written map blobs at {lo} differ from the restatement")
    used = reps * E.used_bytes()
    eg_bytes = reps * sum(map(len, canon)) + used
    eg = {"median_ms": round(tm["egest_sizes"]["median_ms"] + tm["egest_write"]["median_ms"], 4)}
    res["map_mvreg"] = {
        "n_obj": n, "caps": list(caps), "exact": True, "blob_bytes": blob_bytes, "used_slab_bytes": used,
        "ingest": rates(tm["ingest"], n, blob_bytes + used),
        "egest": dict(rates(eg, n, eg_bytes), sizes=tm["egest_sizes"], write=tm["egest_write"]),
        "merge": dict(tm["merge"], M_obj_per_s=round(n / tm["merge"]["median_ms"] / 1e3, 2)),
        "ingest_over_merge": round(tm["ingest"]["median_ms"] / tm["merge"]["median_ms"], 3),
        "egest_over_merge": round(eg["median_ms"] / tm["merge"]["median_ms"], 3)}
    del dE, dO, out_i, out_m, eout, t

    # ------------------------------------------------------------ the stand-alone MVReg
    regs = mo.gen_batch(0xBE5C, REG_BASE, A, REG_CAP, 3, 4, 4)["regs0"]
    reps = max(1, a.n_regs // REG_BASE)
    n = reps * REG_BASE
    S = mo.slab(regs, REG_CAP, A)
    blobs = [MB.encode_mvreg(r, WA, WV) for r in regs]
    t, bo, bl, blob_bytes = tiled_blobs(blobs, reps, 0xB1E)

    def dev(x):
        x = torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.int64)).to("cuda:0")
        return x.repeat((reps,) + (1,) * (x.dim() - 1)).contiguous()

    def alloc(cap):
        return (torch.empty(n, dtype=torch.int32, device="cuda:0"),
                torch.empty((n, cap, A), dtype=torch.int64, device="cuda:0"),
                torch.empty((n, cap), dtype=torch.int64, device="cuda:0"))

    dS = tuple(dev(x) for x in S)
    dO = tuple(torch.roll(x, 1, 0) for x in dS)
    out_i, out_m = alloc(REG_CAP), alloc(2 * REG_CAP)
    sizes = torch.empty(n, dtype=torch.int64, device="cuda:0")
    lens = eng.mvreg_to_bincode(dS, A, WA, WV)[2]
    eout, eoff = placed(lens)
    calls = {
        "ingest": lambda: crdts_hip.check(lib.crdt_mvreg_from_bincode(
            eng.ctx, p(t), int(t.numel()), p(bo), p(bl), n, WA, WV, A, p(out_i[0]), p(out_i[1]), p(out_i[2]), REG_CAP,
            st), "mvreg_from_bincode"),
        "egest_sizes": lambda: crdts_hip.check(lib.crdt_mvreg_bincode_sizes(
            eng.ctx, p(dS[0]), p(dS[1]), p(dS[2]), REG_CAP, n, A, WA, WV, p(sizes), st), "mvreg_bincode_sizes"),
        "egest_write": lambda: crdts_hip.check(lib.crdt_mvreg_to_bincode(
            eng.ctx, p(dS[0]), p(dS[1]), p(dS[2]), REG_CAP, n, A, WA, WV, p(eout), p(eoff), int(eout.numel()), st),
            "mvreg_to_bincode"),
        "merge": lambda: eng.mvreg_merge(dS, dO, A, out=out_m, stream=s, check_status=False),
    }
    tm = timed(calls, a.rounds, a.warmup)
    for lo in (0, n - REG_BASE):
        for g, e in zip(out_i, S):
            if not bool((g[lo:lo + REG_BASE].cpu().numpy().view(e.dtype) == e).all()):
                raise SystemExit(f"map_bincode_bench: ingested registers at {lo} differ from the restatement")
        if blobs_of(eout, eoff, lens, lo, lo + REG_BASE) != blobs or not torch.equal(sizes, lens):
            raise SystemExit(f"map_bincode_bench: written register blobs at {lo} differ from the restatement")
    used = reps * (int(S[0].sum()) * (8 * A + 8) + 4 * REG_BASE)
    eg = {"median_ms": round(tm["egest_sizes"]["median_ms"] + tm["egest_write"]["median_ms"], 4)}
    res["mvreg"] = {
        "n_obj": n, "cap": REG_CAP, "exact": True, "blob_bytes": blob_bytes, "used_slab_bytes": used,
        "zero_filled_block_bytes": n * (REG_CAP * (8 * A + 8) + 4),
        "ingest": rates(tm["ingest"], n, blob_bytes + used),
        "egest": dict(rates(eg, n, blob_bytes + used), sizes=tm["egest_sizes"], write=tm["egest_write"]),
        "merge": dict(tm["merge"], M_obj_per_s=round(n / tm["merge"]["median_ms"] / 1e3, 2)),
        "ingest_over_merge": round(tm["ingest"]["median_ms"] / tm["merge"]["median_ms"], 3),
        "egest_over_merge": round(eg["median_ms"] / tm["merge"]["median_ms"], 3)}
    res["build"] = crdts_hip.build_record()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
