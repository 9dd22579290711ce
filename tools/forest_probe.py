#!/usr/bin/env python3
"""Developer probe: rk_forest_rows against rk_dist_rows + a Kruskal on the host, over the bench's collections at -D 0.05: the
10,000- and 50,000-genome clade collections, a species of 1,000 strains per clade, and (memory allowing) the 500,000-genome scale
collection.  Per collection: wall time of both paths (synchronous calls; 2 warm-up calls, then the median and the spread of the
timed ones), the call's stats (rounds among them), the bytes each path moves to the host, and whether both paths give the same
edges.  The host Kruskal orders by the exact ratio common / u (integer cross-multiplication through a 62-bit key, as the device
does), then row, then col.
    python3 tools/forest_probe.py [out.json] [collections: 10k,50k,species,500k]        (default profiles/forest_probe.json)"""
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

BITS, KMER, MAX_DIST, M = 28, 20, 0.05, 1220


def host_kruskal(hits, n, metric):
    """the forest of a hit list on the host: a lexsort by (exact ratio descending, row, col) and a union-find"""
    c = hits["common"].astype(object)
    u = (hits["size0"].astype(np.int64) + hits["size1"] - hits["common"]) if metric == 0 else np.minimum(hits["size0"], hits["size1"]).astype(np.int64)
    key = np.array([(int(ci) << 62) // int(ui) for ci, ui in zip(c, u)], dtype=np.uint64)   # distinct ratios, distinct keys (u < 2^31)
    order = np.lexsort((hits["col"], hits["row"], ~key))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    keep = []
    rows, cols = hits["row"].tolist(), hits["col"].tolist()
    for e in order.tolist():
        a, b = find(rows[e]), find(cols[e])
        if a != b:
            parent[max(a, b)] = min(a, b)
            keep.append(e)
    return hits[np.array(keep, dtype=np.int64)] if keep else hits[:0]


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": reps}


def probe(ctx, name, index, n, reps):
    (edges, st), t_forest = timed(lambda: ctx.forest_rows(index, 0, KMER, MAX_DIST), reps)
    (hits, _), t_rows = timed(lambda: ctx.dist_rows(index, None, 1, 0, KMER, MAX_DIST), reps)
    t0 = time.perf_counter()
    want = host_kruskal(hits, n, 0)
    kruskal_ms = (time.perf_counter() - t0) * 1e3
    equal = len(want) == len(edges) and all(np.array_equal(edges[f], want[f]) for f in capi.HIT_DTYPE.names if f != "pad")
    res = {"collection": name, "genomes": n, "kernel": ctx.dist_kernel_name(index, None, 1, 0, KMER, MAX_DIST), "hits": int(len(hits)),
           "forest_edges": int(len(edges)), "forest_rows": t_forest, "dist_rows": t_rows, "host_kruskal_python_ms": round(kruskal_ms, 3),
           "ratio_dist_rows_over_forest_rows": round(t_rows["median_ms"] / t_forest["median_ms"], 3),
           "stats": st, "bytes_to_host_forest_rows": 40 * int(len(edges)) + 32 + 8 * st["rounds"] + 20 * st["borderline"],
           "bytes_to_host_dist_rows": 40 * int(len(hits)) + 8, "edges_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    return res


def main(out_path=None, which="10k,50k,species,500k"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "forest_probe.json")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 10), ("50k", 50000, 10), ("species", 10000, 1000)):
        if name not in which.split(","):
            continue
        names, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=strains)
        index = ctx.index_build(ctx.sketches_from_host(h, off), BITS)
        results.append(probe(ctx, "clade_%d_strains_%d" % (n, strains), index, len(names), 9))
        del index
        ctx.trim()
    if "500k" in which.split(","):
        try:
            n = 500000
            h, off, _ = synth.scale_collection_torch(n)
            torch.cuda.synchronize()
            index = ctx.index_build(ctx.sketches_from_dev(h.data_ptr(), off.data_ptr(), n), BITS)
            del h, off
            results.append(probe(ctx, "scale_500000", index, n, 3))
            del index
        except (capi.RkError, RuntimeError, MemoryError) as e:   # device or host memory
            results.append({"collection": "scale_500000", "skipped": str(e)[:300]})
            print(json.dumps(results[-1]), flush=True)
    res = {"max_dist": MAX_DIST, "hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "collections": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r.get("edges_equal", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
