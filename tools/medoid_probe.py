#!/usr/bin/env python3
"""Developer probe: rk_medoid_rows (labels: rk_cluster_rows at half of -D) with and without the two record arrays, against what a user
has without it -- rk_dist_rows plus a numpy grouping of the downloaded hit records (degrees, sums and the two extreme records per
genome) --, against the same call with RK_MEDOID_DEVICE=0 (rk_dist_rows + rk_medoid_hits inside the call) and against rk_dbscan_rows
(min_pts 5) on the same index, the nearest existing call.  Over the collections of tools/dbscan_probe.py at -D 0.05: 10,000 and 50,000
genomes in clades of 10, a species of 1,000 strains per clade, and the star of 3,000 leaves (-D 0.03).  Per collection: wall time of
every leg (synchronous calls; 2 warm-up calls, then the median and the spread of 9 timed ones), sums sweep through gather kernel by HIP
events (RK_MS_MEDOID), the call's stats, the bytes each leg moves to the host, and whether the legs agree.
    python3 tools/medoid_probe.py [out.json] [collections: 10k,50k,species,star]        (default profiles/medoid_probe.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rabbitkssd_amd import capi, synth  # noqa: E402

BITS, KMER, MAX_DIST, M, MIN_PTS = 28, 20, 0.05, 1220, 5
RK_MS_MEDOID = 11
NONE = capi.MEDOID_NONE


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, summary(ms)


def numpy_grouping(hits, n, labels):
    """degrees, sums and the two extreme records per genome from a downloaded hit list: one sort of the 2 * hits (genome, record)
    incidences by (genome, inside, ratio key, neighbour), then run starts"""
    labels = np.asarray(labels, dtype=np.uint32)
    row, col = hits["row"], hits["col"]
    inside = (labels[row] == labels[col]) & (labels[row] != NONE)
    u = hits["size0"].astype(np.uint64) + hits["size1"].astype(np.uint64) - hits["common"].astype(np.uint64)
    q = (hits["common"].astype(np.uint64) << np.uint64(32)) // np.maximum(u, np.uint64(1))
    ends = np.concatenate([row, col]).astype(np.int64)
    other = np.concatenate([col, row]).astype(np.int64)
    ins2, q2 = np.concatenate([inside, inside]), np.concatenate([q, q])
    in_deg = np.bincount(ends[ins2], minlength=n).astype(np.uint32)
    out_deg = np.bincount(ends[~ins2], minlength=n).astype(np.uint32)
    central = np.zeros(n, dtype=np.uint64)
    order = np.argsort(ends[ins2], kind="stable")
    if len(order):
        e_sorted = ends[ins2][order]
        starts = np.flatnonzero(np.concatenate([[True], e_sorted[1:] != e_sorted[:-1]]))
        central[e_sorted[starts]] = np.add.reduceat(q2[ins2][order], starts)
    rec = np.concatenate([np.arange(len(hits)), np.arange(len(hits))])
    far = np.full(n, -1, dtype=np.int64)
    near = np.full(n, -1, dtype=np.int64)
    for mask, key, dest in ((ins2, q2, far), (~ins2, ~q2, near)):   # (q orders as the ratio does up to 2^-32: a probe, not the rule)
        idx = np.flatnonzero(mask)
        if len(idx):
            o = idx[np.lexsort((other[idx], key[idx], ends[idx]))]
            first = np.flatnonzero(np.concatenate([[True], ends[o][1:] != ends[o][:-1]]))
            dest[ends[o][first]] = rec[o][first]
    return in_deg, out_deg, central, far, near


def probe(ctx, name, index, n, max_dist, reps):
    labels, _ = ctx.cluster_rows(index, 0, KMER, max_dist / 2)
    call = lambda **kw: ctx.medoid_rows(index, 0, KMER, max_dist, labels, **kw)   # noqa: E731
    device, t_device = timed(call, reps)
    bare, t_bare = timed(lambda: call(records=False), reps)
    ctx.set_timing(True)
    call()
    sweeps_ms = ctx.last_ms(RK_MS_MEDOID)
    call(records=False)
    sums_ms = ctx.last_ms(RK_MS_MEDOID)
    ctx.set_timing(False)

    def with_env(key, value, fn):
        def run():
            os.environ[key] = value
            try:
                return fn()
            finally:
                del os.environ[key]
        return run
    host, t_host = timed(with_env("RK_MEDOID_DEVICE", "0", call), reps)

    def user():
        hits = ctx.dist_rows(index, None, 1, 0, KMER, max_dist)[0]
        return numpy_grouping(hits, n, labels), len(hits)
    (grouped, n_hits), t_user = timed(user, reps)
    (_, _, _, _, dst), t_dbscan = timed(lambda: ctx.dbscan_rows(index, 0, KMER, max_dist, MIN_PTS), reps)
    st = device[5]
    equal = all(np.array_equal(a, b) for a, b in zip(device[:5], host[:5]))
    equal = equal and all(np.array_equal(a, b) for a, b in zip(device[:3], bare[:3])) and all(np.array_equal(a, b) for a, b in zip(device[:3], grouped[:3]))
    res = {"collection": name, "genomes": n, "max_dist": max_dist, "labels": "rk_cluster_rows at %g" % (max_dist / 2), "clusters": int(len(np.unique(labels))),
           "kernel": ctx.dist_kernel_name(index, None, 1, 0, KMER, max_dist), "hits": n_hits, "medoid_rows": t_device, "medoid_rows_no_records": t_bare,
           "sums_to_gather_ms": round(sweeps_ms, 4), "sums_alone_ms": round(sums_ms, 4),
           "medoid_rows_host_leg": t_host, "dist_rows_plus_numpy": t_user,
           "dbscan_rows": t_dbscan, "ratio_numpy_over_medoid_rows": round(t_user["median_ms"] / t_device["median_ms"], 3),
           "ratio_host_leg_over_medoid_rows": round(t_host["median_ms"] / t_device["median_ms"], 3),
           "ratio_medoid_rows_over_dbscan_rows": round(t_device["median_ms"] / t_dbscan["median_ms"], 3), "stats": st,
           "bytes_to_host_medoid_rows": 96 * n + 32 + 28 * st["borderline"], "bytes_to_host_no_records": 16 * n + 32 + 28 * st["borderline"],
           "bytes_to_device_labels": 4 * n, "bytes_to_host_baseline": 40 * n_hits + 8, "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    return res


def star(leaves):
    """a hub of 100 hashes and `leaves` sketches that keep 60 of them: hub-leaf d = 0.0255, leaf-leaf ~0.05 (tests/test_gpu_medoid.py)"""
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 24, size=47 * leaves))
    rng.shuffle(pool)
    hub, spare = pool[:100], pool[100:]
    parts = [np.sort(hub)] + [np.sort(np.concatenate([rng.choice(hub, size=60, replace=False), spare[40 * j: 40 * j + 40]])) for j in range(leaves)]
    parts = [parts[i] for i in np.random.default_rng(12).permutation(len(parts))]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts).astype(np.uint32), off


def main(out_path=None, which="10k,50k,species,star"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "medoid_probe.json")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 10), ("50k", 50000, 10), ("species", 10000, 1000)):
        if name not in which.split(","):
            continue
        names, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=strains)
        index = ctx.index_build(ctx.sketches_from_host(h, off), BITS)
        results.append(probe(ctx, "clade_%d_strains_%d" % (n, strains), index, len(names), MAX_DIST, 9))
        del index
        ctx.trim()
    if "star" in which.split(","):
        h, off = star(3000)
        index = ctx.index_build(ctx.sketches_from_host(h, off), 24)
        results.append(probe(ctx, "star_3000_leaves", index, len(off) - 1, 0.03, 9))
        del index
    res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "collections": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r.get("results_equal", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
