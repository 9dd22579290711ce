"""`dist -N 5 -D 1.0` at BASELINE configs[4] (100,000 references of 76 hashes x 1,000 queries of ~45,776, 24-bit): rk_dist_topn
against rk_dist_rows + rk_topn_rows in warm steady state -- wall time and the context's device memory -- and rk_dist_topn's
stages (rk_ctx_last_ms RK_MS_TOPN_*: counting kernel, selection kernel, candidate sort + download, host finish) with its
candidate count per row.  Writes one JSON document.

    python tools/topn_timing.py [--reps 10] [--old-reps 3] [--no-old] [--out profiles/topn_configs4.json]

Kernel times under a profiler: rocprofv3 --kernel-trace --stats -d DIR -- python tools/topn_timing.py --no-old --reps 5"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabbitkssd_amd import capi, synth  # noqa: E402

N, D, K = 5, 1.0, 20


def raw_topn(ctx, idx, qs, metric):
    L = capi.lib()
    opts = capi.DistOpts(0, metric, K, 0, D, 0, 1)
    hits, n = C.c_void_p(), C.c_uint64()
    t0 = time.perf_counter()
    ctx.check(L.rk_dist_topn(ctx._h, idx._h, qs._h, C.byref(opts), C.c_uint64(N), C.byref(hits), C.byref(n)))
    t = time.perf_counter() - t0
    out = np.frombuffer(C.string_at(hits.value, n.value * capi.HIT_DTYPE.itemsize), dtype=capi.HIT_DTYPE).copy()
    L.rk_free_host(hits)
    return t, out


def raw_old(ctx, idx, qs, metric):
    L = capi.lib()
    opts = capi.DistOpts(0, metric, K, 0, D, 0, 1)
    hits, n = C.c_void_p(), C.c_uint64()
    t0 = time.perf_counter()
    ctx.check(L.rk_dist_rows(ctx._h, idx._h, qs._h, C.byref(opts), C.byref(hits), C.byref(n), None))
    t1 = time.perf_counter()
    n_all = n.value
    hp = C.cast(hits, C.c_void_p)
    if L.rk_topn_rows(hp, C.byref(n), C.c_uint64(N)):
        raise RuntimeError("rk_topn_rows")
    t = time.perf_counter() - t0
    out = np.frombuffer(C.string_at(hits.value, n.value * capi.HIT_DTYPE.itemsize), dtype=capi.HIT_DTYPE).copy()
    L.rk_free_host(hits)
    return t, t1 - t0, n_all, out


def setup(ctx, rh, roff, qh, qoff):
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), 24)
    qs = ctx.sketches_from_host(qh, qoff)
    return idx, qs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--old-reps", type=int, default=3)
    ap.add_argument("--no-old", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t0 = time.perf_counter()
    _, rh, roff = synth.clade_sketches(100000, 76, 24, seed=31)
    _, qh, qoff = synth.clade_sketches(1000, 45776, 24, seed=32)
    res = {"shape": "configs[4]: 100,000 refs x 76 hashes, 1,000 queries x 45,776 hashes, 24-bit; dist -N 5 -D 1.0, metric 0",
           "generate_s": round(time.perf_counter() - t0, 2)}

    ctx = capi.Context(0)
    idx, qs = setup(ctx, rh, roff, qh, qoff)
    ctx.trim()   # (pool bytes from here on: the live index + queries, then what the calls add)
    before = ctx.pool_stats()
    for _ in range(2):
        _, new = raw_topn(ctx, idx, qs, 0)
    walls = [raw_topn(ctx, idx, qs, 0)[0] * 1e3 for _ in range(args.reps)]
    after = ctx.pool_stats()
    ctx.set_timing(True)
    stages = {k: [] for k in ("counts_ms", "select_ms", "sort_download_ms", "host_finish_ms", "candidates")}
    for _ in range(max(3, args.reps // 2)):
        raw_topn(ctx, idx, qs, 0)
        for i, k in enumerate(stages):
            stages[k].append(ctx.last_ms(1 + i))
    ctx.set_timing(False)
    res["topn"] = {
        "wall_ms_median": round(float(np.median(walls)), 3), "wall_ms_min": round(float(np.min(walls)), 3), "reps": len(walls),
        "pool_bytes_index_and_queries": before[0], "pool_bytes_peak": after[0], "pool_bytes_of_the_call": after[0] - before[0],
        "stages_median": {k: round(float(np.median(v)), 3) for k, v in stages.items()},
        "candidates_per_row": round(float(np.median(stages["candidates"])) / 1000.0, 1),
        "records": int(len(new)),
    }
    s1 = ctx.pool_stats()
    raw_topn(ctx, idx, qs, 0)
    s2 = ctx.pool_stats()
    res["topn"]["steady_state_driver_allocs"] = s2[2] - s1[2]
    print(json.dumps(res["topn"]), flush=True)
    idx.close()
    qs.close()
    ctx.close()

    if not args.no_old:
        ctx = capi.Context(0)
        idx, qs = setup(ctx, rh, roff, qh, qoff)
        ctx.trim()
        before = ctx.pool_stats()
        _, _, n_all, old = raw_old(ctx, idx, qs, 0)
        runs = [raw_old(ctx, idx, qs, 0) for _ in range(args.old_reps)]
        after = ctx.pool_stats()
        walls_old = [r[0] * 1e3 for r in runs]
        res["old"] = {
            "wall_ms_median": round(float(np.median(walls_old)), 3), "wall_ms_min": round(float(np.min(walls_old)), 3),
            "dist_rows_ms_median": round(float(np.median([r[1] * 1e3 for r in runs])), 3), "reps": len(runs),
            "pool_bytes_index_and_queries": before[0], "pool_bytes_peak": after[0], "pool_bytes_of_the_call": after[0] - before[0],
            "records_before_topn": int(n_all),
            "host_bytes_of_records": int(n_all) * capi.HIT_DTYPE.itemsize,
        }
        res["identical_records"] = bool(old.tobytes() == new.tobytes())
        res["speedup_wall"] = round(res["old"]["wall_ms_median"] / res["topn"]["wall_ms_median"], 1)
        res["device_bytes_ratio"] = round(res["old"]["pool_bytes_of_the_call"] / res["topn"]["pool_bytes_of_the_call"], 1)
        print(json.dumps(res["old"]), flush=True)
        ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
