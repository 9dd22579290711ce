#!/usr/bin/env python3
"""Developer probe: rk_dbscan_rows (min_pts = 5) against the same call with RK_DBSCAN_DEVICE=0 (rk_dist_rows + rk_dbscan_hits inside the
call: every hit record crosses PCIe and the rule runs on the host) and against rk_cluster_rows on the same index (the nearest existing
call: one sweep over the records where this one makes four), over the bench's collections at -D 0.05: the 10,000- and 50,000-genome
clade collections, a species of 1,000 strains per clade, and the star of 3,000 leaves (-D 0.03: every record lands on deg[hub], and the
hub's leaves all meet in one best_w / best_nb minimum each).  Per collection: wall time of every leg (synchronous calls; 2 warm-up
calls, then the median and the spread of the timed ones), hook kernel through label kernel by HIP events (RK_MS_DBSCAN), the call's
stats, the bytes each leg moves to the host, and whether the two dbscan legs agree.
    python3 tools/dbscan_probe.py [out.json] [collections: 10k,50k,species,star]        (default profiles/dbscan_probe.json)"""
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
RK_MS_DBSCAN = 9


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": reps}


def probe(ctx, name, index, n, max_dist, reps):
    device, t_device = timed(lambda: ctx.dbscan_rows(index, 0, KMER, max_dist, MIN_PTS), reps)
    ctx.set_timing(True)
    ctx.dbscan_rows(index, 0, KMER, max_dist, MIN_PTS)
    hook_ms = ctx.last_ms(RK_MS_DBSCAN)
    ctx.set_timing(False)
    os.environ["RK_DBSCAN_DEVICE"] = "0"
    try:
        host, t_host = timed(lambda: ctx.dbscan_rows(index, 0, KMER, max_dist, MIN_PTS), reps)
    finally:
        del os.environ["RK_DBSCAN_DEVICE"]
    (_, cst), t_cluster = timed(lambda: ctx.cluster_rows(index, 0, KMER, max_dist), reps)
    st = device[4]
    equal = all(np.array_equal(a, b) for a, b in zip(device[:4], host[:4]))
    res = {"collection": name, "genomes": n, "min_pts": MIN_PTS, "max_dist": max_dist, "kernel": ctx.dist_kernel_name(index, None, 1, 0, KMER, max_dist),
           "hits": int(host[4]["edges"]), "dbscan_rows": t_device, "hook_to_labels_ms": round(hook_ms, 4), "dbscan_rows_host_leg": t_host,
           "cluster_rows": t_cluster,
           "ratio_host_leg_over_dbscan_rows": round(t_host["median_ms"] / t_device["median_ms"], 3),
           "ratio_dbscan_rows_over_cluster_rows": round(t_device["median_ms"] / t_cluster["median_ms"], 3),
           "stats": st, "cluster_stats": cst, "bytes_to_host_dbscan_rows": 13 * n + 64 + 20 * st["borderline"], "bytes_to_host_host_leg": 40 * int(host[4]["edges"]) + 8,
           "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    return res


def star(leaves):
    """a hub of 100 hashes and `leaves` sketches that keep 60 of them: hub-leaf d = 0.0255, leaf-leaf ~0.05 (tests/test_gpu_dbscan.py)"""
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
    out_path = out_path or os.path.join(ROOT, "profiles", "dbscan_probe.json")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 10), ("50k", 50000, 10), ("species", 10000, 1000)):
        if name not in which.split(","):
            continue
        names, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=strains)
        index = ctx.index_build(ctx.sketches_from_host(h, off), BITS)
        results.append(probe(ctx, "clade_%d_strains_%d" % (n, strains), index, len(names), MAX_DIST, 9 if name != "species" else 5))
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
