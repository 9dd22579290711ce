#!/usr/bin/env python3
"""Developer probe: rk_lca_rows against the same call with RK_LCA_DEVICE=0 (export + look-up + rk_lca_lists inside the call) and against
a numpy route a caller could write without it: export_lists, the LCA of every list by np.minimum / np.maximum.reduceat over preorder ids
and a vectorised climb, np.searchsorted for the query hashes, np.unique over row << 32 | taxon.  Workloads: 1,000 perturbed strains
against 10,000 / 50,000 genomes in clades of 10 under a three-level taxonomy (clade -> group of 10 clades -> root); against 10 species
of 1,000 strains, each under one node; 1,000 queries of 100,000 hashes (a tenth of them hashes of the collection) against the 10,000
genomes.  Per workload and leg: wall time (synchronous calls, download included; warm-up calls -- two of the device leg, one of each
baseline --, then the median and the spread of the timed ones: 9 or 7 of the device leg, 3 of each baseline), the call's timed span by HIP events (RK_MS_LCA), the span of the same call over ONE EMPTY query -- the list pass alone,
which depends on the index and the taxonomy only -- and the difference, the query pass; and whether the legs agree.
    python3 tools/lca_probe.py [out.json] [workloads: 10k,50k,species,big]        (default profiles/lca_probe.json)
A VARIANT is the same measurement of another build of the library, or under a developer switch, recorded beside the workloads of an
existing out.json under "variants"[label]: the constants of rk_lca.hip are compile-time, so a variant of them is a copy of the unit
with the constexpr edited, compiled and linked with the other objects of rabbitkssd_amd/build into a library of its own.
    python3 tools/lca_probe.py out.json 10k,50k,species lane16=/path/to/librabbitkssd_lane16.so
    RK_LCA_CAP=20000000 python3 tools/lca_probe.py out.json big cap20M=            (no path: the library as built)
A variant times the device leg as above and each baseline once, for the comparison of the results alone."""
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

BITS, KMER, M, QUERIES = 28, 20, 1220, 1000
NONE = capi.LCA_NONE


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


def three_levels(n, strains):
    """(parent, taxa): node 0 the root, then the groups of 10 clades, then the clades; genome v carries its clade"""
    clades = n // strains
    groups = -(-clades // 10)
    parent = [0] + [0] * groups + [1 + c // 10 for c in range(clades)]
    return np.array(parent, dtype=np.uint32), np.array([1 + groups + v // strains for v in range(n)], dtype=np.uint32)


def preorder(parent):
    """(pre, ppar, last, node_of) as numpy arrays: an iterative walk, children by ascending id"""
    T = len(parent)
    kids = [[] for _ in range(T)]
    root = 0
    for t in range(T):
        if parent[t] == t:
            root = t
        else:
            kids[parent[t]].append(t)
    pre, ppar, last, node_of = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64)
    n, stack = 0, [(root, 0)]
    node_of[0] = root
    n = 1
    while stack:
        t, k = stack.pop()
        if k < len(kids[t]):
            stack.append((t, k + 1))
            c = kids[t][k]
            pre[c], node_of[n], ppar[n] = n, c, pre[t]
            n += 1
            stack.append((c, 0))
        else:
            last[pre[t]] = n - 1
    return pre, ppar, last, node_of


def numpy_route(index, qs, taxa, parent):
    """(off, taxon, direct, matched, unlabelled) without the library's LCA: what a caller writes today"""
    postings, hashes, counts = index.export_lists()
    qh, qoff = qs.download()
    pre, ppar, last, node_of = preorder(parent.tolist())
    big = np.iinfo(np.int64).max
    g = np.where(taxa[postings] == NONE, -1, pre[np.minimum(taxa[postings], len(parent) - 1)])
    starts = np.concatenate([[0], np.cumsum(counts[:-1], dtype=np.int64)])
    mn = np.minimum.reduceat(np.where(g < 0, big, g), starts)
    mx = np.maximum.reduceat(g, starts)
    at = np.where(mx < 0, 0, mn)
    while True:
        up = last[at] < mx
        if not up.any():
            break
        at = np.where(up, ppar[at], at)
    list_taxon = np.where(mx < 0, 1 << 31, node_of[at]).astype(np.uint64)
    where = np.searchsorted(hashes, qh)
    hit = (where < len(hashes)) & (hashes[np.minimum(where, len(hashes) - 1)] == qh)
    rows = np.repeat(np.arange(len(qoff) - 1, dtype=np.uint64), np.diff(qoff).astype(np.int64))
    keys, direct = np.unique((rows[hit] << np.uint64(32)) | list_taxon[where[hit]], return_counts=True)
    labelled = (keys & np.uint64(0xFFFFFFFF)) < (1 << 31)
    q = len(qoff) - 1
    matched = np.bincount(rows[hit].astype(np.int64), minlength=q)
    unl = np.bincount((keys[~labelled] >> np.uint64(32)).astype(np.int64), weights=direct[~labelled], minlength=q).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount((keys[labelled] >> np.uint64(32)).astype(np.int64), minlength=q))])
    return off, (keys[labelled] & np.uint64(0xFFFFFFFF)).astype(np.uint32), direct[labelled], matched, unl


def probe(ctx, name, index, queries, taxa, parent, reps, slow_reps=3, slow_warm=1):
    empty = ctx.sketches_from_host(np.zeros(0, dtype=np.uint32), np.zeros(2, dtype=np.uint64))

    def call():
        return ctx.lca_rows(index, queries, taxa, parent)

    def host():
        os.environ["RK_LCA_DEVICE"] = "0"
        try:
            return call()
        finally:
            del os.environ["RK_LCA_DEVICE"]

    got, t_device = timed(call, reps)
    ctx.set_timing(True)
    spans, list_spans = [], []
    for _ in range(5):
        call()
        spans.append(ctx.last_ms(capi.MS_LCA))
        ctx.lca_rows(index, empty, taxa, parent)
        list_spans.append(ctx.last_ms(capi.MS_LCA))
    ctx.set_timing(False)
    span, list_span = statistics.median(spans), statistics.median(list_spans)
    hgot, t_host = timed(host, slow_reps, warm=slow_warm)
    ngot, t_numpy = timed(lambda: numpy_route(index, queries, taxa, parent), slow_reps, warm=slow_warm)
    off, recs, matched, unl, st = got
    equal = st["path"] == 1 and hgot[4]["path"] == 2 and all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], hgot[:4]))
    equal = equal and np.array_equal(off, ngot[0]) and np.array_equal(recs["taxon"], ngot[1]) and np.array_equal(recs["direct"], ngot[2])
    equal = equal and np.array_equal(matched, ngot[3]) and np.array_equal(unl, ngot[4])
    q = queries.count
    res = {"workload": name, "references": index.genomes, "nodes": int(len(parent)), "queries": q, "stats": st, "lca_rows": t_device,
           "timed_span_ms": round(span, 4), "list_pass_ms": round(list_span, 4), "query_pass_ms": round(span - list_span, 4),
           "device_share_of_wall": round(span / t_device["median_ms"], 3), "bytes_up": 16 * int(len(parent)) + 4 * index.genomes,
           "bytes_to_host": 8 * (q + 1) + 8 * q + 8 * st["records"] + 32, "lca_rows_host_leg": t_host,
           "ratio_host_leg_over_device": round(t_host["median_ms"] / t_device["median_ms"], 2), "numpy_route": t_numpy,
           "ratio_numpy_over_device": round(t_numpy["median_ms"] / t_device["median_ms"], 2), "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    return res


def main(out_path=None, which="10k,50k,species,big", variant=None):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "lca_probe.json")
    which = which.split(",")
    slow = {}
    if variant is not None:
        label, _, lib_path = variant.partition("=")
        if lib_path:
            capi.LIB_PATH = os.path.abspath(lib_path)   # (before the first call loads the library)
        slow = {"slow_reps": 1, "slow_warm": 0}
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 10), ("50k", 50000, 10), ("species", 10000, 1000)):
        if name not in which and not (name == "10k" and "big" in which):
            continue
        names, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=strains)
        index = ctx.index_build(ctx.sketches_from_host(h, off), BITS)
        parent, taxa = three_levels(n, strains)
        if name in which:
            qh, qoff = perturbed(h, off, range(0, n, n // QUERIES), 7, BITS)
            results.append(probe(ctx, "clade_%d_strains_%d" % (n, strains), index, ctx.sketches_from_host(qh, qoff), taxa, parent, 9, **slow))
        if name == "10k" and "big" in which:
            rng = np.random.default_rng(11)
            pool = np.unique(h)
            parts = [np.unique(np.concatenate([rng.integers(0, 1 << BITS, size=90000, dtype=np.uint64).astype(np.uint32), pool[rng.integers(0, len(pool), size=10000)]]))
                     for _ in range(1000)]
            qh, qoff = csr(parts)
            results.append(probe(ctx, "1000_queries_of_100000_against_10000_genomes", index, ctx.sketches_from_host(qh, qoff), taxa, parent, 7, **slow))
        del index
        ctx.trim()
    if variant is not None:
        res = json.load(open(out_path))
        keep = ("workload", "stats", "lca_rows", "timed_span_ms", "list_pass_ms", "query_pass_ms", "results_equal")
        res.setdefault("variants", {})[label] = {"switches": {k: v for k, v in os.environ.items() if k.startswith("RK_LCA_")},
                                                 "workloads": [{k: r[k] for k in keep} for r in results]}
    else:
        res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "workloads": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r["results_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
