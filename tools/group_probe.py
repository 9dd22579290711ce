#!/usr/bin/env python3
"""Developer probe: rk_group_sketches (labels: rk_cluster_rows at half of -D 0.05; rules pan and core) against the same call with
RK_GROUP_DEVICE=0 (export + rk_group_lists + rk_sketches_from_host inside the call) and against what a user has without it -- a numpy
grouping over the sketches on the host: np.unique over label << 32 | hash with counts.  Over the four shapes the neighbouring probes use:
10,000 and 50,000 genomes in clades of 10, a species of 1,000 strains per clade, a star of 3,000 leaves around one hub.  Per shape and
rule: wall time of every leg (synchronous calls; 2 warm-up calls, then the median and the spread of the timed ones), the first list kernel
through the gather of the hashes by HIP events (RK_MS_GROUP), the call's stats (the lists of every length class, the spilled ones), the
bytes each leg moves, and whether the legs agree.
    python3 tools/group_probe.py [out.json] [shapes: 10k,50k,species,star]        (default profiles/group_probe.json)"""
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


def numpy_grouping(h, off, labels, core):
    """(hashes, off) of the group sketches from the sketches on the host (sets of 32-bit hashes): one np.unique over label << 32 | hash"""
    labels = np.asarray(labels, dtype=np.uint64)
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
    lab = labels[owner]
    keep = lab != capi.GROUP_NONE
    keys, counts = np.unique((lab[keep] << np.uint64(32)) | h[keep].astype(np.uint64), return_counts=True)
    used, sizes = np.unique(labels[labels != capi.GROUP_NONE], return_counts=True)
    if core:
        keys = keys[counts == sizes[np.searchsorted(used, keys >> np.uint64(32))]]
    goff = np.concatenate([[0], np.searchsorted(keys >> np.uint64(32), used, side="right")]).astype(np.uint64)
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), goff


def probe(ctx, name, h, off, bits, reps):
    n = len(off) - 1
    index = ctx.index_build(ctx.sketches_from_host(h, off), bits)
    labels, _ = ctx.cluster_rows(index, 0, KMER, MAX_DIST / 2)
    out = []
    for rule in ("pan", "core"):
        def call():
            sk, gl, gs, st = ctx.group_sketches(index, labels, rule)
            return sk.download(), gl, gs, st

        def host_call():
            os.environ["RK_GROUP_DEVICE"] = "0"
            try:
                return call()
            finally:
                del os.environ["RK_GROUP_DEVICE"]
        device, t_device = timed(call, reps)
        ctx.set_timing(True)
        call()
        kernels_ms = ctx.last_ms(capi.MS_GROUP)
        ctx.set_timing(False)
        host, t_host = timed(host_call, 3, warm=1)
        user, t_user = timed(lambda: numpy_grouping(h, off, labels, rule == "core"), 3, warm=1)
        st = device[3]
        equal = all(np.array_equal(a, b) for a, b in zip(device[0] + device[1:3], host[0] + host[1:3]))
        equal = equal and np.array_equal(device[0][0], user[0]) and np.array_equal(device[0][1], user[1]) and host[3]["path"] == 2 and st["path"] == 1
        res = {"shape": name, "genomes": n, "rule": rule, "groups": st["groups"], "group_sketches": t_device, "first_list_kernel_to_gather_ms": round(kernels_ms, 4),
               "group_sketches_host_leg": t_host, "numpy_unique_over_sketches": t_user, "ratio_host_leg_over_device": round(t_host["median_ms"] / t_device["median_ms"], 3),
               "ratio_numpy_over_device": round(t_user["median_ms"] / t_device["median_ms"], 3), "stats": st,
               "bytes_to_device": 4 * n + 4 * st["groups"], "bytes_to_host_call": 8 * (st["groups"] + 1) + 48,
               "bytes_to_host_download": int(device[0][0].nbytes), "bytes_to_host_host_leg": 4 * st["postings"] + 8 * st["lists"], "results_equal": bool(equal)}
        print(json.dumps(res), flush=True)
        out.append(res)
    del index
    ctx.trim()
    return out


def star(leaves):
    """`leaves` sketches that keep 80 of a hub's 100 hashes and 20 of their own (d = 0.011 to the hub: one cluster at 0.025), and the hub"""
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 24, size=27 * leaves))
    rng.shuffle(pool)
    centre, spare = pool[:100], pool[100:]
    parts = [np.sort(np.concatenate([rng.choice(centre, size=80, replace=False), spare[20 * j: 20 * j + 20]])) for j in range(leaves)] + [np.sort(centre)]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts).astype(np.uint32), off


def main(out_path=None, which="10k,50k,species,star"):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "group_probe.json")
    ctx = capi.Context(0)
    results = []
    for name, n, strains in (("10k", 10000, 10), ("50k", 50000, 10), ("species", 10000, 1000)):
        if name not in which.split(","):
            continue
        _, h, off = synth.clade_sketches(n, M, BITS, kmer_size=KMER, strains_per_clade=strains)
        results += probe(ctx, "clade_%d_strains_%d" % (n, strains), h, off, BITS, 9)
    if "star" in which.split(","):
        h, off = star(3000)
        results += probe(ctx, "star_of_3000_leaves", h, off, 24, 9)
    res = {"hash_bits": BITS, "hashes_per_genome": M, "device": torch.cuda.get_device_name(0), "shapes": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r["results_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
