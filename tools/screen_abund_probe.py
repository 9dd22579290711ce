#!/usr/bin/env python3
"""Developer probe: what abundances cost.  rk_screen_abund_rows (min_common 1, every candidate) on the four workloads of
tools/screen_probe.py, with seeded geometric counts (most of them 1 to 10, with a tail), against rk_screen_rows on the same sketches, against
the same call with RK_SCREEN_DEVICE=0 (export + rk_screen_abund_lists inside the call) and against what a user has without it: the numpy
route of tools/screen_probe.py with the counts carried along (a lexsort by reference and count for the medians).  Then
rk_sketches_mask_counts against rk_sketches_mask on the workloads of tools/mask_probe.py.  Per workload and leg: wall time of synchronous
calls, download included (2 warm-up calls, then the median and the spread of 7), the timed span of the device leg likewise, the value
passes and the segments per select class; all legs are compared for equality before anything is timed.
    python3 tools/screen_abund_probe.py [out.json] [workloads: 10k,50k,species,private,mask]        (default profiles/screen_abund_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gather_probe import BITS, KMER, M, csr, private_hashes, strain_unions, summary, timed, with_env  # noqa: E402
from mask_probe import ascending_sketches  # noqa: E402
from rabbitkssd_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 7


def geometric_counts(n, seed):
    """most counts 1 to 10, with a tail"""
    rng = np.random.default_rng(seed)
    c = rng.geometric(0.35, size=n).astype(np.uint64)
    c[rng.random(n) < 0.03] *= 1000
    return c.astype(np.uint32)


def lower_medians(refs, vals, cands, sizes):
    """per candidate the element of rank (size - 1) // 2 among its values; refs / vals parallel, sizes[cand] values each (0: median 0)"""
    order = np.lexsort((vals, refs))
    start = np.searchsorted(refs[order], cands)
    at = np.minimum(start + (np.maximum(sizes, 1) - 1) // 2, max(len(order) - 1, 0))
    return np.where(sizes > 0, vals[order][at] if len(order) else 0, 0)


def numpy_route(index, ref_sizes, queries, counts):
    """(recs as tuples, abund as tuples, occ) from the exported lists with numpy alone"""
    postings, hashes, lens_all = index.export_lists()
    pos = np.zeros(len(lens_all) + 1, dtype=np.int64)
    pos[1:] = np.cumsum(lens_all)
    n = len(ref_sizes)
    recs, abund, occ = [], [], []
    for q, (s, c) in enumerate(zip(queries, counts)):
        at = np.searchsorted(hashes, s)
        hit = at < len(hashes)
        hit[hit] = hashes[at[hit]] == s[hit]
        u, cu = at[hit], c[hit].astype(np.int64)
        lens = lens_all[u].astype(np.int64)
        starts = np.zeros(len(u) + 1, dtype=np.int64)
        starts[1:] = np.cumsum(lens)
        flat = np.repeat(pos[u] - starts[:-1], lens) + np.arange(starts[-1])
        refs = postings[flat].astype(np.int64)
        vals = np.repeat(cu, lens)
        common = np.bincount(refs, minlength=n)
        cands = np.flatnonzero(common >= 1)
        order = cands[np.lexsort((cands, -ref_sizes[cands].astype(np.int64), -(common[cands] / ref_sizes[cands])))]
        rank = np.full(n, n, dtype=np.int64)
        rank[order] = np.arange(len(order))
        won = np.zeros(n, dtype=np.int64)
        occ_common, occ_won = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        mine = np.zeros(len(refs), dtype=bool)
        if len(u):
            best = np.minimum.reduceat(rank[refs], starts[:-1])   # (every matched list of a built index has a holder, and every holder is a candidate)
            winner = order[best]
            won = np.bincount(winner, minlength=n)
            np.add.at(occ_common, refs, vals)
            np.add.at(occ_won, winner, cu)
            mine = refs == np.repeat(winner, lens)
        med_common = lower_medians(refs, vals, cands, common[cands])
        med_won = lower_medians(refs[mine], vals[mine], cands, won[cands])
        recs += [(q, int(r), int(common[r]), int(won[r]), int(ref_sizes[r]), len(s)) for r in cands]
        abund += [(int(occ_common[r]), int(occ_won[r]), int(a), int(b)) for r, a, b in zip(cands, med_common, med_won)]
        occ.append([int(c.sum(dtype=np.uint64)), int(cu.sum()), int(cu.sum())])
    return recs, abund, occ


def screen_probe(ctx, name, h, off, bits, queries):
    n = len(off) - 1
    index = ctx.index_build(ctx.sketches_from_host(h, off), bits)
    ref_sizes = np.diff(off).astype(np.uint32)
    qh, qoff = csr(queries)
    qc = geometric_counts(len(qh), 19)
    counts = [qc[int(qoff[i]):int(qoff[i + 1])] for i in range(len(queries))]
    qs = ctx.sketches_from_host_counts(qh, qc, qoff)

    def call():
        return ctx.screen_abund_rows(index, qs)

    def plain_call():
        return ctx.screen_rows(index, qs)

    def spanned(fn, which):
        ctx.set_timing(True)
        ms = []
        for k in range(WARM + REPS):
            fn()
            if k >= WARM:
                ms.append(ctx.last_ms(which))
        ctx.set_timing(False)
        return summary(ms)
    host_call = with_env(call, RK_SCREEN_DEVICE=0)
    device, plain, host = call(), plain_call(), host_call()
    recs, abund, occ = numpy_route(index, ref_sizes, queries, counts)
    equal = all(np.array_equal(a, b) for a, b in zip(device[:7], host[:7])) and device[7]["path"] == 1 and host[7]["path"] == 2
    equal = equal and all(np.array_equal(a, b) for a, b in zip((device[0], device[1]) + device[3:6], plain[:5]))
    equal = equal and [tuple(int(r[f]) for f in capi.SCREEN_REC_DTYPE.names) for r in device[1]] == recs
    equal = equal and [tuple(int(a[f]) for f in capi.SCREEN_ABUND_DTYPE.names) for a in device[2]] == abund and device[6].tolist() == occ
    st = device[7]
    _, t_device = timed(call, REPS, WARM)
    span = spanned(call, capi.MS_SCREEN_ABUND)
    _, t_plain = timed(plain_call, REPS, WARM)
    span_plain = spanned(plain_call, capi.MS_SCREEN)
    _, t_host = timed(host_call, REPS, WARM)
    _, t_user = timed(lambda: numpy_route(index, ref_sizes, queries, counts), 3, 1)
    res = {"workload": name, "references": n, "queries": len(queries), "query_hashes": int(qoff[-1]), "records": st["records"], "values": st["values"],
           "value_passes": st["value_passes"], "segments_rank_wave_block": [st["rank_segs"], st["wave_segs"], st["block_segs"]], "stats": st,
           "screen_abund_rows": t_device, "timed_span": span, "screen_rows_same_tree": t_plain, "timed_span_screen_rows": span_plain,
           "ratio_abund_over_plain": round(t_device["median_ms"] / t_plain["median_ms"], 3), "screen_abund_rows_host_leg": t_host,
           "ratio_host_leg_over_device": round(t_host["median_ms"] / t_device["median_ms"], 3), "numpy_over_export_lists": t_user,
           "ratio_numpy_over_device": round(t_user["median_ms"] / t_device["median_ms"], 3), "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    del index, qs
    ctx.trim()
    return res


def mask_probe(ctx, name, rh, roff, bits, qh, qoff):
    wide = qh.dtype == np.uint64
    index = ctx.index_build((ctx.sketches_from_host64 if wide else ctx.sketches_from_host)(rh, roff), bits)
    qc = geometric_counts(len(qh), 23)
    qs = ctx.sketches_from_host_counts(qh, qc, qoff, wide=wide)
    (sk, st), t_counts = timed(lambda: ctx.sketches_mask_counts(qs, index, 0, 0), REPS, WARM)
    (pk, pst), t_plain = timed(lambda: ctx.sketches_mask(qs, index, 0, 0), REPS, WARM)
    (hk, hst), t_host = timed(with_env(lambda: ctx.sketches_mask_counts(qs, index, 0, 0), RK_MASK_DEVICE=0), 1, 0)
    keep = ~np.isin(qh, np.unique(rh))
    equal = all(np.array_equal(a, b) for a, b in zip(sk.download(), pk.download())) and np.array_equal(sk.download_counts(), qc[keep]) and st == pst
    equal = equal and np.array_equal(hk.download_counts(), qc[keep]) and hst["path"] == 2
    res = {"workload": name, "query_hashes": st["hashes"], "kept": st["kept"], "sketches_mask_counts": t_counts, "sketches_mask_same_tree": t_plain,
           "ratio_counts_over_plain": round(t_counts["median_ms"] / t_plain["median_ms"], 3), "sketches_mask_counts_host_leg": t_host, "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    del index, qs, sk, pk, hk
    ctx.trim()
    return res


def main(out_path=None, which="10k,50k,species,private,mask"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "screen_abund_probe.json")
    which = which.split(",")
    ctx = capi.Context(0)
    results, masks = [], []
    for name, n, strains in (("10k", 10000, 5), ("50k", 50000, 50)):
        if name in which:
            _, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=10)
            results.append(screen_probe(ctx, "100_unions_of_%d_strains_of_%d_genomes" % (strains, n), h, off, BITS, strain_unions(h, off, 100, strains, 10, BITS, 7)))
    if "species" in which:
        _, h, off = synth.clade_sketches(10000, M, BITS, kmer_size=KMER, strains_per_clade=1000)
        results.append(screen_probe(ctx, "union_of_a_species_of_1000_strains", h, off, BITS, [np.unique(h[: int(off[1000])])]))
    if "private" in which:
        h, off, queries = private_hashes(3000)
        results.append(screen_probe(ctx, "one_private_hash_with_each_of_3000_references", h, off, 24, queries))
    if "mask" in which:
        rng = np.random.default_rng(4)
        big = ascending_sketches(1000, 100000, BITS, 11, np.uint32)
        own = rng.integers(0, 1 << BITS, size=380000, dtype=np.uint64).astype(np.uint32)
        rh = np.unique(np.concatenate([big[0][:: max(1, len(big[0]) // 365000)][:365000], own]))[:730000]
        masks.append(mask_probe(ctx, "a_1000_queries_of_100000_against_one_reference_of_730000", rh, np.array([0, len(rh)], dtype=np.uint64), BITS, big[0], big[1]))
        clades = synth.clade_sketches(10000, M, BITS, kmer_size=KMER, strains_per_clade=10)
        masks.append(mask_probe(ctx, "b_1000_queries_of_100000_against_10000_genomes", clades[1], clades[2], BITS, big[0], big[1]))
        # ten tiny queries: every other hash one of the collection's, every other one its own
        own = ascending_sketches(10, 500, BITS, 12, np.uint32)[0]
        pool = np.unique(clades[1])
        theirs = pool[:: len(pool) // 5000][:5000]
        parts = [np.unique(np.concatenate([own[i * 500:(i + 1) * 500], theirs[i * 500:(i + 1) * 500]])) for i in range(10)]
        toff = np.zeros(11, dtype=np.uint64)
        toff[1:] = np.cumsum([len(p) for p in parts])
        masks.append(mask_probe(ctx, "c_10_queries_of_1000_against_10000_genomes", clades[1], clades[2], BITS, np.concatenate(parts), toff))
        big = clades = None
        qh, qoff = ascending_sketches(1000, 100000, 36, 13, np.uint64)
        own = rng.integers(0, 1 << 36, size=380000, dtype=np.uint64)
        rh = np.unique(np.concatenate([qh[:: max(1, len(qh) // 365000)][:365000], own]))[:730000]
        masks.append(mask_probe(ctx, "a64_1000_queries_of_100000_against_one_reference_of_730000_64_bit", rh, np.array([0, len(rh)], dtype=np.uint64), 36, qh, qoff))
    res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "protocol": "%d warm-up calls, the median of %d" % (WARM, REPS),
           "workloads": results, "mask_workloads": masks}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r["results_equal"] for r in results + masks) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
