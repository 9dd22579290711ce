#!/usr/bin/env python3
"""Developer probe: rk_knn_rows (k = 10) against what a user does without it -- rk_dist_rows plus a grouping of the hits on the host,
written here with numpy (every hit under both of its genomes, lexsort by genome, distance and neighbour, the first k of each group) --
and against rk_dist_rows + rk_knn_hits (the same grouping in C, exact ratios), over the bench's collections at -D 0.05: the 10,000-
and 50,000-genome clade collections, a species of 1,000 strains per clade, and the star of 3,000 leaves (-D 0.03: its hub is ONE
wave streaming 3,000 entries).  Per collection: wall time of every path (synchronous calls; 2 warm-up calls, then the median and the
spread of the timed ones), degree pass through selection kernel by HIP events (RK_MS_KNN_SELECT), the join alone (rk_dist_rows_dev
into a device buffer, the floor of any path), the call's stats, the bytes each path moves to the host, and whether the paths agree.
    python3 tools/knn_probe.py [out.json] [collections: 10k,50k,species,star]        (default profiles/knn_probe.json)"""
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

BITS, KMER, MAX_DIST, M, K = 28, 20, 0.05, 1220, 10
RK_MS_KNN_SELECT = 8


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": reps}


def group_numpy(hits, n, k):
    """(off, record numbers): per genome the k nearest hits by (dist, neighbour) -- floating-point distances, not exact ratios"""
    m = len(hits)
    genome = np.concatenate([hits["row"], hits["col"]]).astype(np.int64)
    other = np.concatenate([hits["col"], hits["row"]]).astype(np.int64)
    dist = np.concatenate([hits["dist"], hits["dist"]])
    order = np.lexsort((other, dist, genome))
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(genome, minlength=n), out=start[1:])
    g = genome[order]
    keep = np.arange(2 * m) - start[g] < k
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(g[keep], minlength=n), out=off[1:])
    return off, order[keep] % max(m, 1)


def probe(ctx, name, index, n, max_dist, reps):
    (off, nbrs, st), t_knn = timed(lambda: ctx.knn_rows(index, 0, KMER, max_dist, K), reps)
    ctx.set_timing(True)
    ctx.knn_rows(index, 0, KMER, max_dist, K)
    select_ms = ctx.last_ms(RK_MS_KNN_SELECT)
    ctx.set_timing(False)
    (hits, _), t_rows = timed(lambda: ctx.dist_rows(index, None, 1, 0, KMER, max_dist), reps)
    (h_off, h_nbrs), t_hits = timed(lambda: capi.knn_hits(hits, n, K, 0), reps, warm=1)
    (np_off, np_rec), t_numpy = timed(lambda: group_numpy(hits, n, K), reps, warm=1)
    equal = np.array_equal(off, h_off) and len(nbrs) == len(h_nbrs) and all(np.array_equal(nbrs[f], h_nbrs[f]) for f in capi.HIT_DTYPE.names if f != "pad")
    numpy_equal = np.array_equal(off, np_off) and all(np.array_equal(nbrs[f], hits[np_rec][f]) for f in ("row", "col"))
    # the join alone into a device buffer: what any path pays first
    cap = max(1 << 16, int(st["edges"]) + 1024)
    buf = torch.empty(cap * capi.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def join():
        cnt.zero_()
        ctx.dist_rows_dev(index, 1, 0, KMER, max_dist, buf.data_ptr(), cap, cnt.data_ptr())
        torch.cuda.synchronize()
    _, t_join = timed(join, reps)
    res = {"collection": name, "genomes": n, "k": K, "max_dist": max_dist, "kernel": ctx.dist_kernel_name(index, None, 1, 0, KMER, max_dist),
           "hits": int(len(hits)), "neighbours": int(len(nbrs)), "knn_rows": t_knn, "degree_to_select_ms": round(select_ms, 4), "join_alone": t_join,
           "dist_rows": t_rows, "knn_hits": t_hits, "numpy_grouping": t_numpy,
           "ratio_dist_rows_plus_numpy_over_knn_rows": round((t_rows["median_ms"] + t_numpy["median_ms"]) / t_knn["median_ms"], 3),
           "ratio_dist_rows_plus_knn_hits_over_knn_rows": round((t_rows["median_ms"] + t_hits["median_ms"]) / t_knn["median_ms"], 3),
           "ratio_knn_rows_over_join_alone": round(t_knn["median_ms"] / t_join["median_ms"], 3),
           "stats": st, "bytes_to_host_knn_rows": 4 * (n + 1) + 40 * int(len(nbrs)) + 32 + 20 * st["borderline"], "bytes_to_host_dist_rows": 40 * int(len(hits)) + 8,
           "results_equal": bool(equal), "numpy_grouping_equal": bool(numpy_equal)}
    print(json.dumps(res), flush=True)
    del buf, cnt
    return res


def star(leaves):
    """a hub of 100 hashes and `leaves` sketches that keep 60 of them: hub-leaf d = 0.0255, leaf-leaf ~0.05 (tests/test_gpu_knn.py)"""
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
    out_path = out_path or os.path.join(ROOT, "profiles", "knn_probe.json")
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
