#!/usr/bin/env python3
"""Developer probe: what counting costs the sketch pass.  rk_sketch_packed_dev_ex against rk_sketch_packed_dev_counts on sequence
resident in HBM, L3K10:
  lds    1,000 genomes of 5 Mb (uniform ACGT): every genome is deduplicated in LDS (k_dedup), min_count 1
  big1   one read set of 240 Mb -- a 24 Mb genome ten times over, so every hash occurs ten times --: its candidate region is beyond
         the LDS sort, the device-wide path (dedup_big), min_count 1: the uncounted call takes sort + unique, the counted one the
         run-length route
  big2   the same at min_count 2: both take the run-length route, the counted one selects the counts as well
Per workload and leg: warm-up calls, then the median, min and max of the wall time of REPS synchronous calls (each call ends with
its read-back), the scan kernel's share by HIP events (RK_MS_SKETCH_KERNEL), the record of the call (rk_sketch_last_plan), and
whether the counted call's hashes and offsets are the uncounted call's, its counts sum to the candidates (lds) or are all 10 (big).

The uncounted legs run on any tree that has the library built, the parent commit's included (--tree DIR: the package is imported
from there; the counted legs are skipped where the symbols are missing).  --parent FILE merges such a run: per workload the
uncounted medians of both trees and whether this tree's median lies within the parent's own min-max spread or below it.
    python3 tools/abund_probe.py [--tree DIR] [--parent parent.json] [--out out.json] [--reps 9]     (default profiles/abund_probe.json)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--genomes", type=int, default=1000)
    args = ap.parse_args()
    assert args.reps >= 7
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from rabbitkssd_amd import capi, synth

    L = capi.lib()
    has_counts = hasattr(L, "rk_sketch_packed_dev_counts")
    ctx = capi.Context(0)
    flt = ctx.filter(capi.params_init(10, 6, 3), synth.shuf_table(10, 6, 3))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")

    def call(fn_name, packed, gbeg, gend, min_count):
        h = C.c_void_p()
        fn = getattr(L, fn_name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        ctx.check(fn(ctx._h, flt._h, C.c_void_p(packed.data_ptr()), C.c_uint64(packed.numel()), gbeg.ctypes.data_as(C.c_void_p),
                     gend.ctypes.data_as(C.c_void_p), C.c_uint32(len(gbeg)), C.c_uint32(min_count), None, C.byref(h)))
        return capi.Sketches(ctx, h)

    def leg(fn_name, packed, gbeg, gend, min_count):
        ctx.set_timing(True)
        for _ in range(2):
            sk = call(fn_name, packed, gbeg, gend, min_count)
        ms, scan = [], []
        for _ in range(args.reps):
            sk = None   # (the result of the call before: its device memory goes back to the pool first)
            t0 = time.perf_counter()
            sk = call(fn_name, packed, gbeg, gend, min_count)
            ms.append((time.perf_counter() - t0) * 1e3)
            scan.append(ctx.last_ms(0))
        ctx.set_timing(False)
        plan = ctx.sketch_last_plan()
        res = dict(summary(ms), scan_kernel_median_ms=round(statistics.median(scan), 4), attempts=plan["attempts"], n_big=plan["n_big"],
                   max_candidates=plan["max_candidates"], hashes=int(sk.total))
        return sk, res

    def workload(name, packed, gbeg, gend, min_count, counts_check):
        usk, unc = leg("rk_sketch_packed_dev_ex", packed, gbeg, gend, min_count)
        res = {"workload": name, "genomes": len(gbeg), "bases": int((gend - gbeg).sum()), "min_count": min_count, "uncounted": unc}
        if has_counts:
            uh, uoff = usk.download()
            usk = None
            csk, cnt = leg("rk_sketch_packed_dev_counts", packed, gbeg, gend, min_count)
            ch, coff = csk.download()
            c = csk.download_counts()
            res["counted"] = cnt
            res["counted_over_uncounted"] = round(cnt["median_ms"] / unc["median_ms"], 4)
            res["counted_minus_uncounted_ms"] = round(cnt["median_ms"] - unc["median_ms"], 4)
            res["results_equal"] = bool(uh.tobytes() == ch.tobytes() and uoff.tobytes() == coff.tobytes() and counts_check(c))
            res["occurrences"] = int(c.astype(np.uint64).sum())
            res["largest_count"] = int(c.max()) if len(c) else 0
        print(json.dumps(res), flush=True)
        ctx.trim()
        return res

    results = []
    # ---- lds: the flagship sketch workload of bench.py
    n, length = args.genomes, 5_000_000
    stride = (length + 1023) // 1024 * 1024
    packed = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    view = packed.view(n, stride)
    for i in range(n):
        view[i, :length] = lut[torch.randint(0, 4, (length,), generator=gen, device="cuda")]
    gbeg = np.arange(n, dtype=np.uint64) * stride
    gend = gbeg + np.uint64(length)
    torch.cuda.synchronize()
    results.append(workload("lds_%d_genomes_of_5Mb" % n, packed, gbeg, gend, 1, lambda c: len(c) > 0 and int(c.min()) >= 1))
    del packed, view
    # ---- big: one read set, the device-wide path
    unit, copies = 24_000_000, 10
    genome = lut[torch.randint(0, 4, (unit,), generator=gen, device="cuda")]
    total = (unit + 1) * copies - 1          # the copies are records of their own: one 0x00 between two of them
    packed = torch.zeros((total + 1023) // 1024 * 1024, dtype=torch.uint8, device="cuda")
    for k in range(copies):
        packed[k * (unit + 1):k * (unit + 1) + unit] = genome
    gbeg, gend = np.zeros(1, dtype=np.uint64), np.array([total], dtype=np.uint64)
    torch.cuda.synchronize()
    for min_count in (1, 2):
        results.append(workload("big%d_one_read_set_of_240Mb_min_count_%d" % (min_count, min_count), packed, gbeg, gend, min_count,
                                lambda c: len(c) > 0 and int(c.min()) == copies and int(c.max()) == copies))
    del packed
    res = {"device": torch.cuda.get_device_name(0), "tree": "this" if os.path.abspath(args.tree) == ROOT else "other", "has_counted_calls": has_counts,
           "reps": args.reps, "workloads": results}
    if args.parent:
        parent = json.load(open(args.parent))
        res["parent"] = {"has_counted_calls": parent["has_counted_calls"], "workloads": [{k: w[k] for k in ("workload", "uncounted")} for w in parent["workloads"]]}
        cmp = []
        for mine, theirs in zip(results, parent["workloads"]):
            assert mine["workload"] == theirs["workload"]
            m, p = mine["uncounted"], theirs["uncounted"]
            cmp.append({"workload": mine["workload"], "this_median_ms": m["median_ms"], "parent_median_ms": p["median_ms"], "parent_min_ms": p["min_ms"],
                        "parent_max_ms": p["max_ms"], "ratio_this_over_parent": round(m["median_ms"] / p["median_ms"], 4),
                        "margin": "the parent's own min-max spread over its %d timed calls" % p["reps"],
                        "uncounted_no_slower_than_parent": bool(m["median_ms"] <= p["max_ms"])})
        res["uncounted_against_parent"] = cmp
    out = args.out or os.path.join(ROOT, "profiles", "abund_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    return 0 if all(r.get("results_equal", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
