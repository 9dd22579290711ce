#!/usr/bin/env python3
"""Developer probe: rk_mreach_rows (min_pts = 5) against the same call with RK_MREACH_DEVICE=0 (rk_dist_rows + rk_mreach_hits inside the
call: every hit record crosses PCIe and the rule runs on the host), against rk_forest_rows on the same index (the same rounds over the
plain weights, without the core records) and against rk_knn_rows with k = 4 (the same adjacency and selection, all four records kept),
over the collections of tools/dbscan_probe.py: the 10,000- and 50,000-genome clade collections, a species of 1,000 strains per clade,
and the star of 3,000 leaves (-D 0.03).  Per collection: wall time of every leg (synchronous calls; 2 warm-up calls, then the median and
the spread of 9 timed ones), degree pass through the last round by HIP events (RK_MS_MREACH), the call's stats, the bytes each leg moves
to the host, and whether the two mreach legs agree.
    python3 tools/mreach_probe.py [out.json] [collections: 10k,50k,species,star]        (default profiles/mreach_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rabbitkssd_amd import capi, synth  # noqa: E402
from dbscan_probe import BITS, KMER, M, MAX_DIST, MIN_PTS, star, timed  # noqa: E402

RK_MS_MREACH = 10
REPS = 9


def probe(ctx, name, index, n, max_dist):
    device, t_device = timed(lambda: ctx.mreach_rows(index, 0, KMER, max_dist, MIN_PTS), REPS)
    ctx.set_timing(True)
    ctx.mreach_rows(index, 0, KMER, max_dist, MIN_PTS)
    rounds_ms = ctx.last_ms(RK_MS_MREACH)
    ctx.set_timing(False)
    os.environ["RK_MREACH_DEVICE"] = "0"
    try:
        host, t_host = timed(lambda: ctx.mreach_rows(index, 0, KMER, max_dist, MIN_PTS), REPS)
    finally:
        del os.environ["RK_MREACH_DEVICE"]
    (_, fst), t_forest = timed(lambda: ctx.forest_rows(index, 0, KMER, max_dist), REPS)
    (_, _, kst), t_knn = timed(lambda: ctx.knn_rows(index, 0, KMER, max_dist, MIN_PTS - 1), REPS)
    st = device[3]
    equal = np.array_equal(device[0], host[0]) and np.array_equal(device[1], host[1]) and device[2].tobytes() == host[2].tobytes()
    res = {"collection": name, "genomes": n, "min_pts": MIN_PTS, "max_dist": max_dist, "kernel": ctx.dist_kernel_name(index, None, 1, 0, KMER, max_dist),
           "hits": int(host[3]["edges"]), "mreach_rows": t_device, "degree_to_last_round_ms": round(rounds_ms, 4), "mreach_rows_host_leg": t_host,
           "forest_rows": t_forest, "knn_rows_k4": t_knn,
           "ratio_host_leg_over_mreach_rows": round(t_host["median_ms"] / t_device["median_ms"], 3),
           "ratio_mreach_rows_over_forest_rows": round(t_device["median_ms"] / t_forest["median_ms"], 3),
           "ratio_mreach_rows_over_knn_rows": round(t_device["median_ms"] / t_knn["median_ms"], 3),
           "stats": st, "forest_stats": fst, "knn_stats": kst, "edges": len(device[2]),
           "bytes_to_host_mreach_rows": 40 * len(device[2]) + 40 * n + 8 * st["rounds"] + 20 * st["borderline"],
           "bytes_to_host_host_leg": 40 * int(host[3]["edges"]) + 8, "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    return res


def main(out_path=None, which="10k,50k,species,star"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "mreach_probe.json")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 10), ("50k", 50000, 10), ("species", 10000, 1000)):
        if name not in which.split(","):
            continue
        names, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=strains)
        index = ctx.index_build(ctx.sketches_from_host(h, off), BITS)
        results.append(probe(ctx, "clade_%d_strains_%d" % (n, strains), index, len(names), MAX_DIST))
        del index
        ctx.trim()
    if "star" in which.split(","):
        h, off = star(3000)
        index = ctx.index_build(ctx.sketches_from_host(h, off), 24)
        results.append(probe(ctx, "star_3000_leaves", index, len(off) - 1, 0.03))
        del index
    res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "reps": REPS, "collections": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r.get("results_equal", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
