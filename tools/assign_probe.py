#!/usr/bin/env python3
"""Developer probe: rk_assign_rows (reference labels: rk_cluster_rows at half of -D; queries: 1,000 strains of the collection with a tenth
of their hashes replaced) with and without the two record arrays, against what a user has without it -- rk_dist_rows with explicit
queries plus a numpy grouping of the downloaded hit records (the three counts, the label, the nearest and the runner-up record per query)
--, against the same call with RK_ASSIGN_DEVICE=0 (rk_dist_rows + rk_assign_hits inside the call) and, for scale, against rk_dist_topn at
N = 1 on the same index and queries (the nearest existing call; it knows no labels).  Over the collections of tools/medoid_probe.py at
-D 0.05: 10,000 and 50,000 genomes in clades of 10, a species of 1,000 strains per clade, and the hub case: one query within -D 0.03 of
3,000 references of two clusters.  Per collection: wall time of every leg (synchronous calls; 2 warm-up calls, then the median and the
spread of 9 timed ones), first sweep through gather kernel by HIP events (RK_MS_ASSIGN), the call's stats, the bytes each leg moves to
the host, and whether the legs agree.
    python3 tools/assign_probe.py [out.json] [collections: 10k,50k,species,hub]        (default profiles/assign_probe.json)"""
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

BITS, KMER, MAX_DIST, M, QUERIES = 28, 20, 0.05, 1220, 1000
RK_MS_ASSIGN = 12
NONE = capi.ASSIGN_NONE


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


def csr(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts).astype(np.uint32), off


def perturbed(h, off, picks, seed, bits, fresh=0.1):
    rng = np.random.default_rng(seed)
    parts = []
    for g in picks:
        mine = h[int(off[g]): int(off[g + 1])].copy()
        swap = rng.random(len(mine)) < fresh
        mine[swap] = rng.integers(0, 1 << bits, size=int(swap.sum()), dtype=np.uint64).astype(h.dtype)
        parts.append(np.unique(mine))
    return csr(parts)


def numpy_grouping(hits, n_query, labels):
    """label, the three counts and the numbers of the nearest and the runner-up record per query from a downloaded hit list: one sort of
    the labelled records by (query, ratio key, reference), then run starts -- twice"""
    labels = np.asarray(labels, dtype=np.uint32)
    row, col = hits["row"].astype(np.int64), hits["col"].astype(np.int64)
    lab = labels[col]
    u = hits["size0"].astype(np.uint64) + hits["size1"].astype(np.uint64) - hits["common"].astype(np.uint64)
    far = ~((hits["common"].astype(np.uint64) << np.uint64(32)) // np.maximum(u, np.uint64(1)))   # (orders as the ratio does up to 2^-32: a probe, not the rule)
    n_within = np.bincount(row, minlength=n_query).astype(np.uint32)
    n_labelled = np.bincount(row[lab != NONE], minlength=n_query).astype(np.uint32)

    def firsts(mask):
        best = np.full(n_query, -1, dtype=np.int64)
        idx = np.flatnonzero(mask)
        if len(idx):
            o = idx[np.lexsort((col[idx], far[idx], row[idx]))]
            first = np.flatnonzero(np.concatenate([[True], row[o][1:] != row[o][:-1]]))
            best[row[o][first]] = o[first]
        return best
    nearest = firsts(lab != NONE)
    label = np.where(nearest >= 0, lab[np.maximum(nearest, 0)] if len(hits) else NONE, NONE).astype(np.uint32)
    same = (lab == label[row]) & (lab != NONE)
    n_same = np.bincount(row[same], minlength=n_query).astype(np.uint32)
    runner_up = firsts((lab != NONE) & ~same)
    return label, n_within, n_labelled, n_same, nearest, runner_up


def probe(ctx, name, index, n, queries, nq, max_dist, reps, labels=None):
    if labels is None:
        labels, _ = ctx.cluster_rows(index, 0, KMER, max_dist / 2)
    call = lambda **kw: ctx.assign_rows(index, queries, 0, KMER, max_dist, labels, **kw)   # noqa: E731
    device, t_device = timed(call, reps)
    bare, t_bare = timed(lambda: call(records=False), reps)
    ctx.set_timing(True)
    call()
    sweeps_ms = ctx.last_ms(RK_MS_ASSIGN)
    call(records=False)
    counts_ms = ctx.last_ms(RK_MS_ASSIGN)
    ctx.set_timing(False)

    def with_env(key, value, fn):
        def run():
            os.environ[key] = value
            try:
                return fn()
            finally:
                del os.environ[key]
        return run
    host, t_host = timed(with_env("RK_ASSIGN_DEVICE", "0", call), reps)
    # the wave-level combine of the two sweeps off (RK_ASSIGN_COMBINE=0), the two forms alternating call by call
    plain_call = with_env("RK_ASSIGN_COMBINE", "0", call)
    for _ in range(2):
        call()
        plain_call()
    ms = {"on": [], "off": [], "on_events": [], "off_events": []}
    ctx.set_timing(True)
    for _ in range(reps):
        for key, fn in (("on", call), ("off", plain_call)):
            t0 = time.perf_counter()
            plain = fn()
            ms[key].append((time.perf_counter() - t0) * 1e3)
            ms[key + "_events"].append(ctx.last_ms(RK_MS_ASSIGN))
    ctx.set_timing(False)
    combine = {k: summary(v) for k, v in ms.items()}
    combine["equal"] = bool(all(np.array_equal(a, b) for a, b in zip(device[:6], plain[:6])))

    def user():
        hits = ctx.dist_rows(index, queries, 0, 0, KMER, max_dist)[0]
        return numpy_grouping(hits, nq, labels), hits
    (grouped, hits), t_user = timed(user, reps)
    top1, t_topn = timed(lambda: ctx.dist_topn(index, queries, 0, KMER, max_dist, 1), reps)
    st = device[6]
    equal = all(np.array_equal(a, b) for a, b in zip(device[:6], host[:6]))
    equal = equal and all(np.array_equal(a, b) for a, b in zip(device[:4], bare[:4])) and all(np.array_equal(a, b) for a, b in zip(device[:4], grouped[:4]))
    for mine, theirs in ((device[4], grouped[4]), (device[5], grouped[5])):   # (which queries have the record; the record itself may differ where two keys tie in 32 bits)
        equal = equal and np.array_equal(mine["row"] != NONE, theirs >= 0)
    res = {"collection": name, "references": n, "queries": nq, "max_dist": max_dist, "clusters": int(len(np.unique(labels))),
           "kernel": ctx.dist_kernel_name(index, queries, 0, 0, KMER, max_dist), "hits": int(len(hits)), "assign_rows": t_device, "assign_rows_no_records": t_bare,
           "first_to_gather_ms": round(sweeps_ms, 4), "three_sweeps_ms": round(counts_ms, 4), "assign_rows_host_leg": t_host, "dist_rows_plus_numpy": t_user,
           "combine_on_off_alternating": combine, "dist_topn_1": t_topn, "topn_records": int(len(top1)), "ratio_numpy_over_assign_rows": round(t_user["median_ms"] / t_device["median_ms"], 3),
           "ratio_host_leg_over_assign_rows": round(t_host["median_ms"] / t_device["median_ms"], 3),
           "ratio_assign_rows_over_dist_topn_1": round(t_device["median_ms"] / t_topn["median_ms"], 3), "stats": st,
           "bytes_to_host_assign_rows": 96 * nq + 32 + 28 * st["borderline"], "bytes_to_host_no_records": 16 * nq + 32 + 28 * st["borderline"],
           "bytes_to_device_labels": 4 * n, "bytes_to_host_baseline": 40 * int(len(hits)) + 8, "results_equal": bool(equal and combine["equal"])}
    print(json.dumps(res), flush=True)
    return res


def hub(leaves):
    """references: `leaves` sketches that keep 60 of a hub's 100 hashes, alternately of two clusters; queries: the hub (within -D 0.03 of
    every reference: d = 0.0255, all ratios equal) and one unrelated sketch (tests/test_gpu_assign.py)"""
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 24, size=47 * leaves))
    rng.shuffle(pool)
    centre, spare = pool[:100], pool[100:]
    parts = [np.sort(np.concatenate([rng.choice(centre, size=60, replace=False), spare[40 * j: 40 * j + 40]])) for j in range(leaves)]
    return csr(parts), csr([np.sort(centre), np.sort(spare[40 * leaves: 40 * leaves + 100])]), [1 - (v % 2) for v in range(leaves)]


def main(out_path=None, which="10k,50k,species,hub"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "assign_probe.json")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 10), ("50k", 50000, 10), ("species", 10000, 1000)):
        if name not in which.split(","):
            continue
        names, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=strains)
        index = ctx.index_build(ctx.sketches_from_host(h, off), BITS)
        qh, qoff = perturbed(h, off, range(0, n, n // QUERIES), 7, BITS)
        queries = ctx.sketches_from_host(qh, qoff)
        results.append(probe(ctx, "clade_%d_strains_%d" % (n, strains), index, len(names), queries, len(qoff) - 1, MAX_DIST, 9))
        del index, queries
        ctx.trim()
    if "hub" in which.split(","):
        (h, off), (qh, qoff), labels = hub(3000)
        index = ctx.index_build(ctx.sketches_from_host(h, off), 24)
        results.append(probe(ctx, "hub_of_3000_references", index, len(off) - 1, ctx.sketches_from_host(qh, qoff), 2, 0.03, 9, labels=labels))
        del index
    res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "collections": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r.get("results_equal", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
