#!/usr/bin/env python3
"""Developer probe: rk_sketches_mask {0, 0} against the same call with RK_MASK_DEVICE=0 (download + export + rk_mask_lists + upload inside
the call) and against what a caller does without it: download the query hashes, np.isin against the references' hashes, upload what is
left.  Workloads: (a) 1,000 query sketches of 100,000 hashes against one reference of 730,000 hashes (a human genome at L3), half of
which the queries hold; (b) the same queries against the 10,000-genome clade collection of synth; (c) 10 queries of 1,000 hashes
against (b); (a64) is (a) in the 64-bit layout.  Per workload and leg: wall time (synchronous calls; warm-up calls, then the median and
the spread of the timed ones), the call's timed span by HIP events (RK_MS_MASK) and its share of the wall time, the bytes the kernels
must read and write at the least (computed from the shapes: two passes over the hashes, the keep words twice, the survivors, the
offsets; the probes of the look-up depend on the data and are not counted) and the rate that gives over the timed span, and whether the
legs agree.
    python3 tools/mask_probe.py [out.json] [workloads: a,b,c,a64]        (default profiles/mask_probe.json)"""
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
        out = None   # (the result of the call before: its device memory goes back to the pool first)
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


def ascending_sketches(n, size, bits, seed, dtype):
    """n set sketches of `size` hashes each, ascending, spread over 2^bits: cumulative sums of random steps"""
    rng = np.random.default_rng(seed)
    step = max(2, int(1.6 * (1 << bits) / size))   # the last hash lies near 0.8 * 2^bits
    h = np.cumsum(rng.integers(1, step, size=(n, size), dtype=np.uint64), axis=1, dtype=np.uint64)
    assert int(h.max()) < (1 << bits)
    off = np.arange(n + 1, dtype=np.uint64) * size
    return h.reshape(-1).astype(dtype), off


def probe(ctx, name, rh, roff, bits, qh, qoff, reps, slow_reps=1):
    wide = qh.dtype == np.uint64
    from_host = ctx.sketches_from_host64 if wide else ctx.sketches_from_host
    index = ctx.index_build(from_host(rh, roff), bits)
    qs = from_host(qh, qoff)
    held = np.unique(rh)

    def call():
        return ctx.sketches_mask(qs, index, 0, 0)

    def caller_today():
        h, off = qs.download()
        keep = ~np.isin(h, held)
        before = np.concatenate([[0], np.cumsum(keep, dtype=np.uint64)])
        return from_host(h[keep], before[off.astype(np.int64)])

    (sk, st), t_device = timed(call, reps)
    ctx.set_timing(True)
    call()
    span_ms = round(ctx.last_ms(capi.MS_MASK), 4)
    ctx.set_timing(False)
    device = sk.download()
    (hsk, hst), t_host = timed(with_env(call, RK_MASK_DEVICE=0), slow_reps, warm=0)
    host = hsk.download()
    del hsk
    usk, t_user = timed(caller_today, slow_reps, warm=0)
    user = usk.download()
    del usk
    equal = st["path"] == 1 and hst["path"] == 2 and all(np.array_equal(a, b) for a, b in zip(device, host)) and all(np.array_equal(a, b) for a, b in zip(device, user))
    w = qh.itemsize
    n = len(qoff) - 1
    least = 2 * st["hashes"] * w + 2 * st["tiles"] * (st["tile_hashes"] // 8) + st["kept"] * w + 8 * st["tiles"] + 16 * (n + 1)
    res = {"workload": name, "hash_bytes": w, "references": len(roff) - 1, "reference_hashes": int(roff[-1]), "distinct_indexed": index.distinct,
           "queries": n, "query_hashes": st["hashes"], "kept": st["kept"], "matched": st["matched"], "emptied": st["emptied"], "stats": st,
           "sketches_mask": t_device, "timed_span_ms": span_ms, "device_share_of_wall": round(span_ms / t_device["median_ms"], 3),
           "kernel_bytes_at_least": least, "rate_over_span_GB_s": round(least / (span_ms * 1e-3) / 1e9, 1) if span_ms else None,
           "bytes_to_host_call": 8 * (n + 1) + 24, "sketches_mask_host_leg": t_host, "bytes_across_host_leg": (st["hashes"] + st["kept"]) * w + 4 * index.total + (w + 4) * index.distinct,
           "ratio_host_leg_over_device": round(t_host["median_ms"] / t_device["median_ms"], 2), "download_isin_upload": t_user,
           "bytes_across_download_isin_upload": (st["hashes"] + st["kept"]) * w, "ratio_isin_over_device": round(t_user["median_ms"] / t_device["median_ms"], 2),
           "results_equal": bool(equal)}
    print(json.dumps(res), flush=True)
    del index, qs, sk
    ctx.trim()
    return res


def main(out_path=None, which="a,b,c,a64"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "mask_probe.json")
    which = which.split(",")
    ctx = capi.Context(0)
    results = []
    big = ascending_sketches(1000, 100000, BITS, 11, np.uint32) if {"a", "b"} & set(which) else None
    rng = np.random.default_rng(4)

    def human(qh, bits, dtype):
        """one reference of 730,000 hashes: half of them hashes the queries hold, half of them its own"""
        own = rng.integers(0, 1 << bits, size=380000, dtype=np.uint64).astype(dtype)
        h = np.unique(np.concatenate([qh[:: max(1, len(qh) // 365000)][:365000], own]))[:730000]
        return h, np.array([0, len(h)], dtype=np.uint64)
    if "a" in which:
        rh, roff = human(big[0], BITS, np.uint32)
        results.append(probe(ctx, "a_1000_queries_of_100000_against_one_reference_of_730000", rh, roff, BITS, big[0], big[1], 7))
    clades = synth.clade_sketches(10000, M, BITS, kmer_size=KMER, strains_per_clade=10) if {"b", "c"} & set(which) else None
    if "b" in which:
        results.append(probe(ctx, "b_1000_queries_of_100000_against_10000_genomes", clades[1], clades[2], BITS, big[0], big[1], 7))
    if "c" in which:
        # ten tiny queries: every other hash one of the collection's, every other one its own
        own = ascending_sketches(10, 500, BITS, 12, np.uint32)[0]
        pool = np.unique(clades[1])
        theirs = pool[:: len(pool) // 5000][:5000]
        parts = [np.unique(np.concatenate([own[i * 500:(i + 1) * 500], theirs[i * 500:(i + 1) * 500]])) for i in range(10)]
        toff = np.zeros(11, dtype=np.uint64)
        toff[1:] = np.cumsum([len(p) for p in parts])
        results.append(probe(ctx, "c_10_queries_of_1000_against_10000_genomes", clades[1], clades[2], BITS, np.concatenate(parts), toff, 21, slow_reps=5))
    big = clades = None
    if "a64" in which:
        qh, qoff = ascending_sketches(1000, 100000, 36, 13, np.uint64)
        rh, roff = human(qh, 36, np.uint64)
        results.append(probe(ctx, "a64_1000_queries_of_100000_against_one_reference_of_730000_64_bit", rh, roff, 36, qh, qoff, 7))
    res = {"hash_bits": BITS, "device": torch.cuda.get_device_name(0), "workloads": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r["results_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
