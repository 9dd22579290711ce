#!/usr/bin/env python3
"""Developer probe: rk_cluster_rows against rk_dist_rows + a union-find on the host, over the bench's collections at -D 0.05:
the 10,000- and 50,000-genome clade collections, a species of 1,000 strains per clade, and (memory allowing) the 500,000-genome
scale collection.  Per collection: wall time of both paths (synchronous calls; 2 warm-up calls, then the median and the spread of
the timed ones), the hook kernel alone (HIP events, RK_MS_CLUSTER_HOOK), the call's stats, the bytes each path moves to the host,
and that both paths give the same labels.
    python3 tools/cluster_probe.py [out.json] [collections: 10k,50k,species,500k]        (default profiles/cluster_probe.json)"""
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
RK_MS_CLUSTER_HOOK = 6


def components(row, col, n):
    """labels (smallest member) of the graph's components: scipy where it is installed, else min-label propagation in numpy"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _, comp = connected_components(coo_matrix((np.ones(len(row), dtype=np.int8), (row, col)), shape=(n, n)), directed=False)
        first = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(first, comp, np.arange(n))
        return first[comp].astype(np.uint32)
    except ImportError:
        lab = np.arange(n, dtype=np.int64)
        while True:
            m = np.minimum(lab[row], lab[col])
            new = lab.copy()
            np.minimum.at(new, row, m)
            np.minimum.at(new, col, m)
            new = new[new]
            if np.array_equal(new, lab):
                return lab.astype(np.uint32)
            lab = new


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
    ctx.set_timing(True)
    (labels, st), t_cluster = timed(lambda: ctx.cluster_rows(index, 0, KMER, MAX_DIST), reps)
    hook_ms = ctx.last_ms(RK_MS_CLUSTER_HOOK)
    ctx.set_timing(False)
    (labels2, st2), t_plain = timed(lambda: ctx.cluster_rows(index, 0, KMER, MAX_DIST), reps)   # without the events
    (hits, _), t_rows = timed(lambda: ctx.dist_rows(index, None, 1, 0, KMER, MAX_DIST), reps)
    t0 = time.perf_counter()
    want = components(hits["row"].astype(np.int64), hits["col"].astype(np.int64), n)
    uf_ms = (time.perf_counter() - t0) * 1e3
    res = {"collection": name, "genomes": n, "kernel": ctx.dist_kernel_name(index, None, 1, 0, KMER, MAX_DIST), "hits": int(len(hits)),
           "cluster_rows": t_plain, "cluster_rows_timing_on": t_cluster, "hook_kernel_ms": round(hook_ms, 5),
           "dist_rows": t_rows, "host_union_find_ms": round(uf_ms, 3),
           "ratio_dist_rows_over_cluster_rows": round(t_rows["median_ms"] / t_plain["median_ms"], 3),
           "stats": st2, "bytes_to_host_cluster_rows": 4 * n + 32 + 20 * st2["borderline"], "bytes_to_host_dist_rows": 40 * int(len(hits)) + 8,
           "labels_equal": bool(np.array_equal(labels2, want) and np.array_equal(labels, want))}
    print(json.dumps(res), flush=True)
    return res


def main(out_path=None, which="10k,50k,species,500k"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "cluster_probe.json")
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
    return 0 if all(r.get("labels_equal", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
