#!/usr/bin/env python3
"""Developer probe: rk_greedy_rows against rk_dist_rows + rk_greedy_hits (the sequential rule on the host, in C), over the bench's
collections at -D 0.05: the 10,000- and 50,000-genome clade collections, a species of 1,000 strains per clade, and (memory
allowing) the 500,000-genome scale collection.  Per collection: wall time of both paths (synchronous calls; 2 warm-up calls, then
the median and the spread of the timed ones), the call's stats (rounds among them), the time of all rounds by HIP events
(RK_MS_GREEDY_ROUNDS), the bytes each path moves between host and device, and whether both paths give the same representatives and
links.
    python3 tools/greedy_probe.py [out.json] [collections: 10k,50k,species,500k]        (default profiles/greedy_probe.json)"""
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
RK_MS_GREEDY_ROUNDS = 7


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
    (rep, links, st), t_greedy = timed(lambda: ctx.greedy_rows(index, 0, KMER, MAX_DIST), reps)
    L = capi.lib()
    L.rk_ctx_set_timing(ctx._h, 1)
    ctx.greedy_rows(index, 0, KMER, MAX_DIST)
    rounds_ms = float(L.rk_ctx_last_ms(ctx._h, RK_MS_GREEDY_ROUNDS))
    L.rk_ctx_set_timing(ctx._h, 0)
    (hits, _), t_rows = timed(lambda: ctx.dist_rows(index, None, 1, 0, KMER, MAX_DIST), reps)
    (want_rep, want_links), t_host = timed(lambda: capi.greedy_hits(hits, n, 0), reps, warm=1)
    equal = np.array_equal(rep, want_rep) and len(links) == len(want_links) and all(
        np.array_equal(links[f], want_links[f]) for f in capi.HIT_DTYPE.names if f != "pad")
    batches = st["rounds"] if st["rounds"] <= 4 else 4 + (min(st["rounds"], 16) - 4 + 3) // 4 + (max(st["rounds"], 16) - 16 + 7) // 8
    res = {"collection": name, "genomes": n, "kernel": ctx.dist_kernel_name(index, None, 1, 0, KMER, MAX_DIST), "hits": int(len(hits)),
           "representatives": st["n_reps"], "greedy_rows": t_greedy, "rounds_ms": round(rounds_ms, 4), "dist_rows": t_rows, "greedy_hits": t_host,
           "ratio_host_path_over_greedy_rows": round((t_rows["median_ms"] + t_host["median_ms"]) / t_greedy["median_ms"], 3),
           "stats": st, "bytes_greedy_rows": 8 * n + 44 * n + 32 + 64 * batches + 28 * st["borderline"] + 8 * st["borderline_kept"],
           "bytes_dist_rows": 40 * int(len(hits)) + 8, "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    return res


def main(out_path=None, which="10k,50k,species,500k"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "greedy_probe.json")
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
    return 0 if all(r.get("results_equal", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
