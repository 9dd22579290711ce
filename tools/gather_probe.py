#!/usr/bin/env python3
"""Developer probe: rk_gather_rows (min_new 1, no limit) against the same call with RK_GATHER_DEVICE=0 (export + rk_gather_lists inside
the call) and against what a user has without it -- a numpy loop over rk_dist_rows: per round the dense common counts of the queries'
remaining hashes, an argmax per row, the picked reference's hashes taken out of the query on the host, the remaining queries uploaded
again.  Workloads: 100 queries that are each the union of 5 (50) strains drawn from different clades of 10,000 (50,000) genomes in clades
of 10, plus 20 % unrelated hashes; one query that is the union of a species of 1,000 strains; one query that shares one private hash with
each of 3,000 references.  Per workload and leg: wall time (synchronous calls; warm-up calls, then the median and the spread of the timed
ones), the rounds, the launches and the read-backs, the call's timed span by HIP events (RK_MS_GATHER) and its share of the wall time,
and whether the legs agree.  The two choices that were made by measurement are measured here: the cover walk split by the length of the
list (RK_GATHER_LANE_MAX = 8, 16, 32, 64) against every list by one lane (RK_GATHER_SPLIT=0), and the rounds between two reads of the live-row counter
(RK_GATHER_SYNC_EVERY = 1, 2, 4, 8, 16).
    python3 tools/gather_probe.py [out.json] [workloads: 10k,50k,species,private]        (default profiles/gather_probe.json)"""
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

BITS, KMER, M = 28, 20, 1220


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


def with_env(fn, **env):
    def call():
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            return fn()
        finally:
            for k in env:
                del os.environ[k]
    return call


def csr(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0)).astype(np.uint32), off


def numpy_rounds(ctx, index, h, off, queries):
    """(query, ref, fresh) of every pick and the rounds taken, with rk_dist_rows' dense common counts and numpy alone"""
    live = {q: s for q, s in enumerate(queries) if len(s)}
    picks = {q: [] for q in range(len(queries))}
    rounds = 0
    while live:
        order = sorted(live)
        qh, qoff = csr([live[q] for q in order])
        dense = ctx.dist_rows(index, ctx.sketches_from_host(qh, qoff), 0, 0, KMER, 0.0, want_dense=True)[1]
        best = dense.argmax(axis=1)   # (the first maximum: the smaller index)
        rounds += 1
        for row, q in enumerate(order):
            r, fresh = int(best[row]), int(dense[row, best[row]])
            if fresh < 1:
                del live[q]
                continue
            picks[q].append((q, r, fresh))
            left = np.setdiff1d(live[q], h[int(off[r]):int(off[r + 1])], assume_unique=True)
            if len(left):
                live[q] = left
            else:
                del live[q]
    return [p for q in range(len(queries)) for p in picks[q]], rounds


def probe(ctx, name, h, off, bits, queries, reps, numpy_leg=True):
    n = len(off) - 1
    index = ctx.index_build(ctx.sketches_from_host(h, off), bits)
    qh, qoff = csr(queries)
    qs = ctx.sketches_from_host(qh, qoff)

    def call():
        return ctx.gather_rows(index, qs)

    def spanned(fn):
        ctx.set_timing(True)
        fn()
        ms = ctx.last_ms(capi.MS_GATHER)
        ctx.set_timing(False)
        return round(ms, 4)
    device, t_device = timed(call, reps)
    span_ms = spanned(call)
    host, t_host = timed(with_env(call, RK_GATHER_DEVICE=0), 3, warm=1)
    st = device[5]
    equal = all(np.array_equal(a, b) for a, b in zip(device[:5], host[:5])) and st["path"] == 1 and host[5]["path"] == 2
    res = {"workload": name, "references": n, "queries": len(queries), "query_hashes": int(qoff[-1]), "picks": st["picks"], "gather_rows": t_device,
           "timed_span_ms": span_ms, "device_share_of_wall": round(span_ms / t_device["median_ms"], 3), "rounds": st["rounds"],
           "launched_rounds": st["launched_rounds"], "launches": st["launches"], "read_backs": st["read_backs"], "stats": st,
           "gather_rows_host_leg": t_host, "host_leg_rounds": host[5]["rounds"], "host_leg_launches": 0,
           "ratio_host_leg_over_device": round(t_host["median_ms"] / t_device["median_ms"], 3),
           "bytes_to_host_call": 32 * st["picks"] + 12 * len(queries) + 8 * (len(queries) + 1), "bytes_to_host_host_leg": 4 * index.total + 8 * index.distinct + int(qh.nbytes)}
    if numpy_leg:
        (user, user_rounds), t_user = timed(lambda: numpy_rounds(ctx, index, h, off, queries), 1, warm=0)
        mine = [(int(p["query"]), int(p["ref"]), int(p["fresh"])) for p in device[1]]
        equal = equal and user == mine
        res.update({"numpy_loop_over_dist_rows": t_user, "numpy_loop_rounds": user_rounds, "numpy_loop_launches": "one rk_dist_rows call and one upload per round",
                    "ratio_numpy_over_device": round(t_user["median_ms"] / t_device["median_ms"], 3)})
    # the two choices made by measurement, both alternatives
    res["cover_walk"] = {}
    for lane_max in (8, 16, 32, 64, 0):   # 0: no split, every list by the lane that found the winner
        alt_call = with_env(call, RK_GATHER_LANE_MAX=lane_max) if lane_max else with_env(call, RK_GATHER_SPLIT=0)
        alt, t_alt = timed(alt_call, reps)
        equal = equal and all(np.array_equal(a, b) for a, b in zip(device[:5], alt[:5]))
        res["cover_walk"]["lane_max_%d" % lane_max if lane_max else "every_list_by_one_lane"] = dict(
            t_alt, timed_span_ms=spanned(alt_call), lane_lists=alt[5]["lane_lists"], wave_lists=alt[5]["wave_lists"], block_lists=alt[5]["block_lists"])
    res["sync_every"] = {}
    for every in (1, 2, 4, 8, 16):
        got, t = timed(with_env(call, RK_GATHER_SYNC_EVERY=every), reps)
        equal = equal and all(np.array_equal(a, b) for a, b in zip(device[:5], got[:5]))
        res["sync_every"][str(every)] = dict(t, launched_rounds=got[5]["launched_rounds"], read_backs=got[5]["read_backs"], launches=got[5]["launches"])
    res["results_equal"] = bool(equal)
    print(json.dumps(res), flush=True)
    del index, qs
    ctx.trim()
    return res


def strain_unions(h, off, n_queries, strains, per_clade, bits, seed):
    """queries that are each the union of `strains` genomes drawn from different clades, plus 20 % unrelated hashes"""
    rng = np.random.default_rng(seed)
    n = len(off) - 1
    out = []
    for _ in range(n_queries):
        clades = rng.choice(n // per_clade, size=strains, replace=False)
        members = clades * per_clade + rng.integers(0, per_clade, size=strains)
        union = np.unique(np.concatenate([h[int(off[g]):int(off[g + 1])] for g in members]))
        foreign = rng.integers(0, 1 << bits, size=len(union) // 5, dtype=np.uint64).astype(np.uint32)
        out.append(np.unique(np.concatenate([union, foreign])))
    return out


def private_hashes(n):
    """n references of 100 hashes each and the query that holds one private hash of each"""
    pool = np.random.default_rng(3).permutation(1 << 24)[: 100 * n].astype(np.uint32)
    parts = [np.sort(pool[100 * v: 100 * v + 100]) for v in range(n)]
    h, off = csr(parts)
    return h, off, [np.sort(pool[::100])]


def main(out_path=None, which="10k,50k,species,private"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "gather_probe.json")
    which = which.split(",")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 5), ("50k", 50000, 50)):
        if name in which:
            _, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=10)
            results.append(probe(ctx, "100_unions_of_%d_strains_of_%d_genomes" % (strains, n), h, off, BITS, strain_unions(h, off, 100, strains, 10, BITS, 7), 7))
    if "species" in which:
        _, h, off = synth.clade_sketches(10000, M, BITS, kmer_size=KMER, strains_per_clade=1000)
        species = np.unique(h[: int(off[1000])])
        results.append(probe(ctx, "union_of_a_species_of_1000_strains", h, off, BITS, [species], 5))
    if "private" in which:
        h, off, queries = private_hashes(3000)
        results.append(probe(ctx, "one_private_hash_with_each_of_3000_references", h, off, 24, queries, 5))
    res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "workloads": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r["results_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
