#!/usr/bin/env python3
"""Developer probe: rk_screen_rows (min_common 1, every candidate) against the same call with RK_SCREEN_DEVICE=0 (export +
rk_screen_lists inside the call), against what a user has without it -- a numpy route over Index.export_lists: a searchsorted per query,
the matched lists gathered, a bincount for common, the row's candidates ranked once (lexsort), the minimum rank per list
(np.minimum.reduceat), a bincount for won -- and, for context only, against rk_gather_rows, which answers a different question on the
same inputs.  The workloads are those of tools/gather_probe.py, unchanged, so that the two commands can be read side by side.  Per
workload and leg: wall time (synchronous calls; 2 warm-up calls, then the median and the spread of 7), the call's timed span by HIP
events (RK_MS_SCREEN; the same protocol: the median and the spread of 7 spans) and its share of the wall time, the launches and read-backs, and whether the legs agree: all legs are compared
for equality before anything is timed.  The choice that was made by measurement is measured here: equal (row, winner) of a wave combined
before the add against every add lane by lane (RK_SCREEN_COMBINE=0).
The numpy route ranks by the float64 quotient common / size: with sizes below 2^20 two different quotients differ by more than 2^-40
and equal ones divide to the same double, so its order is the exact one on these workloads (the library compares 64-bit products).
    python3 tools/screen_probe.py [out.json] [workloads: 10k,50k,species,private]        (default profiles/screen_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gather_probe import BITS, KMER, M, csr, private_hashes, strain_unions, summary, timed, with_env  # noqa: E402
from rabbitkssd_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 7


def numpy_route(index, ref_sizes, queries):
    """(off, recs, matched, n_cand, claimed) from the exported lists with numpy alone"""
    postings, hashes, counts = index.export_lists()
    pos = np.zeros(len(counts) + 1, dtype=np.int64)
    pos[1:] = np.cumsum(counts)
    n = len(ref_sizes)
    off, recs = [0], []
    matched, n_cand, claimed = [], [], []
    for q, s in enumerate(queries):
        at = np.searchsorted(hashes, s)
        hit = at < len(hashes)
        hit[hit] = hashes[at[hit]] == s[hit]
        u = at[hit]   # (a list of a built index holds at least one posting)
        lens = counts[u].astype(np.int64)
        starts = np.zeros(len(u) + 1, dtype=np.int64)
        starts[1:] = np.cumsum(lens)
        flat = np.repeat(pos[u] - starts[:-1], lens) + np.arange(starts[-1])
        refs = postings[flat]
        common = np.bincount(refs, minlength=n)
        cands = np.flatnonzero(common >= 1)
        order = cands[np.lexsort((cands, -ref_sizes[cands].astype(np.int64), -(common[cands] / ref_sizes[cands])))]
        rank = np.full(n, n, dtype=np.int64)
        rank[order] = np.arange(len(order))
        won = np.zeros(n, dtype=np.int64)
        if len(u):
            best = np.minimum.reduceat(rank[refs], starts[:-1])
            won = np.bincount(order[best[best < n]], minlength=n)
        matched.append(len(u))
        n_cand.append(len(cands))
        claimed.append(int(won.sum()))
        recs += [(q, int(r), int(common[r]), int(won[r]), int(ref_sizes[r]), len(s)) for r in cands]
        off.append(len(recs))
    return off, recs, matched, n_cand, claimed


def as_lists(got):
    off, recs, matched, n_cand, claimed = got[:5]
    return off.tolist(), [tuple(int(r[f]) for f in capi.SCREEN_REC_DTYPE.names) for r in recs], matched.tolist(), n_cand.tolist(), claimed.tolist()


def probe(ctx, name, h, off, bits, queries):
    n = len(off) - 1
    index = ctx.index_build(ctx.sketches_from_host(h, off), bits)
    ref_sizes = np.diff(off).astype(np.uint32)   # (the sketches of these workloads are sets)
    qh, qoff = csr(queries)
    qs = ctx.sketches_from_host(qh, qoff)

    def call():
        return ctx.screen_rows(index, qs)

    def spanned(fn):
        """the timed span under the same protocol as the wall times: WARM calls, then the median and the spread of REPS spans"""
        ctx.set_timing(True)
        ms = []
        for k in range(WARM + REPS):
            fn()
            if k >= WARM:
                ms.append(ctx.last_ms(capi.MS_SCREEN))
        ctx.set_timing(False)
        return summary(ms)
    plain_call, host_call = with_env(call, RK_SCREEN_COMBINE=0), with_env(call, RK_SCREEN_DEVICE=0)
    # all legs agree before anything is timed
    device, plain, host = call(), plain_call(), host_call()
    user = numpy_route(index, ref_sizes, queries)
    equal = all(np.array_equal(a, b) for a, b in zip(device[:5], plain[:5])) and all(np.array_equal(a, b) for a, b in zip(device[:5], host[:5]))
    equal = equal and as_lists(device) == tuple(user) and device[5]["path"] == 1 and plain[5]["path"] == 1 and host[5]["path"] == 2
    st = device[5]
    _, t_device = timed(call, REPS, WARM)
    span = spanned(call)
    span_ms = span["median_ms"]
    _, t_plain = timed(plain_call, REPS, WARM)
    span_plain = spanned(plain_call)
    _, t_host = timed(host_call, REPS, WARM)
    _, t_user = timed(lambda: numpy_route(index, ref_sizes, queries), REPS, WARM)
    gathered, t_gather = timed(lambda: ctx.gather_rows(index, qs), 3, 1)   # (context only: 1 warm-up call, 3 timed)
    res = {"workload": name, "references": n, "queries": len(queries), "query_hashes": int(qoff[-1]), "records": st["records"], "screen_rows": t_device,
           "timed_span_ms": span_ms, "timed_span": span, "device_share_of_wall": round(span_ms / t_device["median_ms"], 3), "launches": st["launches"], "read_backs": st["read_backs"],
           "stats": st, "screen_rows_plain_adds": dict(t_plain, timed_span_ms=span_plain["median_ms"], timed_span=span_plain, adds=plain[5]["adds"]), "adds_combined": st["adds"],
           "screen_rows_host_leg": t_host, "ratio_host_leg_over_device": round(t_host["median_ms"] / t_device["median_ms"], 3),
           "numpy_over_export_lists": t_user, "ratio_numpy_over_device": round(t_user["median_ms"] / t_device["median_ms"], 3),
           "gather_rows_for_context": dict(t_gather, picks=gathered[5]["picks"], rounds=gathered[5]["rounds"], launches=gathered[5]["launches"]),
           "ratio_gather_over_screen": round(t_gather["median_ms"] / t_device["median_ms"], 3),
           "bytes_to_host_call": 24 * st["records"] + 12 * len(queries) + 8 * (len(queries) + 1), "bytes_to_host_host_leg": 4 * index.total + 8 * index.distinct + int(qh.nbytes),
           "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    del index, qs
    ctx.trim()
    return res


def main(out_path=None, which="10k,50k,species,private"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "screen_probe.json")
    which = which.split(",")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 5), ("50k", 50000, 50)):
        if name in which:
            _, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=10)
            results.append(probe(ctx, "100_unions_of_%d_strains_of_%d_genomes" % (strains, n), h, off, BITS, strain_unions(h, off, 100, strains, 10, BITS, 7)))
    if "species" in which:
        _, h, off = synth.clade_sketches(10000, M, BITS, kmer_size=KMER, strains_per_clade=1000)
        species = np.unique(h[: int(off[1000])])
        results.append(probe(ctx, "union_of_a_species_of_1000_strains", h, off, BITS, [species]))
    if "private" in which:
        h, off, queries = private_hashes(3000)
        results.append(probe(ctx, "one_private_hash_with_each_of_3000_references", h, off, 24, queries))
    res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "protocol": "%d warm-up calls, the median of %d" % (WARM, REPS),
           "workloads": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r["results_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
