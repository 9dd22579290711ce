#!/usr/bin/env python3
"""Developer probe: the sharded build from PER-RANK sketches over the scale collection, one GPU playing S ranks and S shards.
Per rank (contiguous genome ranges): the signature and the split into keys (count + pack).  Per shard: the build from the keys
that would arrive (the all-to-all emulated by concatenation) against rk_index_build_shard over the whole collection -- time, the
pool bytes each build takes from the driver (after rk_ctx_trim: its peak), and that order, postings and tile records agree.  Then
the record exchange (concatenation), the joins, and the hit count against the one-GPU build.
    python3 tools/shard_keys_probe.py [n_genomes] [S] [out.json]        (default profiles/shard_keys_500k.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rabbitkssd_amd import capi, synth  # noqa: E402

BITS, KMER, MAX_DIST = 28, 20, 0.05


def timed(fn, reps=2):
    """(last result, ms of the last of `reps` runs): the first run loads the code objects"""
    out, ms = None, 0.0
    for _ in range(reps):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    return out, ms


def pool_growth(ctx, fn):
    ctx.trim()
    before = ctx.pool_stats()[0]
    out = fn()
    torch.cuda.synchronize()
    return out, ctx.pool_stats()[0] - before


def hits_of(ctx, index):
    cap = 1 << 25
    hits = torch.empty(cap * 48, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.dist_rows_dev(index, 1, 0, KMER, MAX_DIST, hits.data_ptr(), cap, cnt.data_ptr())
    torch.cuda.synchronize()
    n = int(cnt.item())
    assert n <= cap, "hit buffer too small"
    return n


def main(n=500000, S=8, out_path=None):
    os.environ.setdefault("RK_POOL_LIMIT_MB", "196608")
    out_path = out_path or os.path.join(ROOT, "profiles", "shard_keys_%dk.json" % (n // 1000))
    ctx = capi.Context(0)
    h, off, _ = synth.scale_collection_torch(n)
    torch.cuda.synchronize()
    off_h = off.cpu().numpy()
    bounds = [n * r // S for r in range(S + 1)]
    ranks, sigs, sends, counts = [], [], [], []
    for r in range(S):
        a, b = bounds[r], bounds[r + 1]
        loff = (off[a:b + 1] - off[a]).contiguous()
        torch.cuda.synchronize()
        loc = ctx.sketches_from_dev(h.data_ptr() + 4 * int(off_h[a]), loff.data_ptr(), b - a)
        sig = torch.empty((b - a) * 17, dtype=torch.int32, device="cuda")
        _, ms_sig = timed(lambda: ctx.sketches_signature(loc, sig.data_ptr()))
        cnt, ms_count = timed(lambda: ctx.sketches_shard_keys(loc, a, n, BITS, S))
        buf = torch.empty(max(1, sum(cnt)), dtype=torch.int64, device="cuda")
        _, ms_pack = timed(lambda: ctx.sketches_shard_pack(loc, a, n, BITS, S, buf.data_ptr()))
        ranks.append({"rank": r, "genomes": b - a, "postings": int(off_h[b] - off_h[a]), "signature_ms": round(ms_sig, 4),
                      "split_count_ms": round(ms_count, 4), "split_pack_ms": round(ms_pack, 4), "split_ms": round(ms_count + ms_pack, 4),
                      "key_bytes": 8 * sum(cnt), "read_write_bytes": 4 * int(off_h[b] - off_h[a]) * 2 + 8 * sum(cnt)})
        print("rank %d: %d genomes, signature %.3f ms, split %.3f + %.3f ms" % (r, b - a, ms_sig, ms_count, ms_pack), flush=True)
        sigs.append(sig)
        sends.append(buf)
        counts.append(cnt)
        del loc
    sig_all = torch.cat(sigs)
    del sigs
    torch.cuda.synchronize()
    whole = ctx.sketches_from_dev(h.data_ptr(), off.data_ptr(), n)
    shards, parts, refs = [], [], []
    for d in range(S):
        recv = torch.cat([sends[r][sum(counts[r][:d]):sum(counts[r][:d + 1])] for r in range(S)])
        n_keys = sum(counts[r][d] for r in range(S))
        torch.cuda.synchronize()
        part, ms_keys = timed(lambda: ctx.index_build_shard_keys(recv.data_ptr(), n_keys, sig_all.data_ptr(), n, BITS, d, S))
        del part
        part, pool_keys = pool_growth(ctx, lambda: ctx.index_build_shard_keys(recv.data_ptr(), n_keys, sig_all.data_ptr(), n, BITS, d, S))
        ref, ms_sk = timed(lambda: ctx.index_build_shard(whole, BITS, d, S))
        del ref
        ref, pool_sk = pool_growth(ctx, lambda: ctx.index_build_shard(whole, BITS, d, S))
        same = part.total == ref.total == n_keys and np.array_equal(part.order, ref.order) and part.shard_records(S) == ref.shard_records(S)
        same = same and records_of(part, S) == records_of(ref, S)
        shards.append({"shard": d, "keys": n_keys, "key_build_ms": round(ms_keys, 4), "sketch_build_ms": round(ms_sk, 4),
                       "key_build_pool_bytes": pool_keys, "sketch_build_pool_bytes": pool_sk, "same_as_sketch_build": bool(same)})
        print("shard %d: %d keys, key build %.3f ms (%.2f GB), sketch build %.3f ms (%.2f GB), same %s"
              % (d, n_keys, ms_keys, pool_keys / 1e9, ms_sk, pool_sk / 1e9, same), flush=True)
        del recv
        parts.append(part)
        refs.append(ref)
    del sends
    n_hits_sk = joined_hits(ctx, refs, S)
    del refs
    n_hits = joined_hits(ctx, parts, S)
    del parts
    one = ctx.index_build(whole, BITS)
    n_one = hits_of(ctx, one)
    del one
    res = {"genomes": n, "shards": S, "hash_bits": BITS, "max_dist": MAX_DIST, "postings": int(off_h[-1]),
           "signature_all_gather_bytes": 68 * n, "ranks": ranks, "shards_detail": shards,
           "slowest_key_build_ms": max(s["key_build_ms"] for s in shards), "slowest_sketch_build_ms": max(s["sketch_build_ms"] for s in shards),
           "slowest_split_ms": max(r["split_ms"] for r in ranks), "slowest_signature_ms": max(r["signature_ms"] for r in ranks),
           "pool_ratio_max": max(s["key_build_pool_bytes"] / s["sketch_build_pool_bytes"] for s in shards),
           "hits_sharded_from_keys": n_hits, "hits_sharded_from_sketches": n_hits_sk, "hits_one_gpu": n_one, "hits_equal": n_hits == n_one == n_hits_sk,
           "all_shards_same": all(s["same_as_sketch_build"] for s in shards),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps({k: v for k, v in res.items() if k not in ("ranks", "shards_detail")}), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    del whole
    ctx.close()
    return 0 if res["hits_equal"] and res["all_shards_same"] else 1


def records_of(part, S):
    """the shard's tile records per destination, sorted (12 bytes each)"""
    cnt = part.shard_records(S)
    b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
    part.shard_pack(b.data_ptr())
    torch.cuda.synchronize()
    rec = b[: sum(cnt) * 12].view(torch.int32).view(-1, 3).cpu().numpy()
    out, at = [], 0
    for c in cnt:
        r = rec[at:at + c]
        out.append(r[np.lexsort(r.T[::-1])].tobytes())
        at += c
    return out


def joined_hits(ctx, parts, S):
    """the record exchange (concatenation), the joins, the hits of all shards"""
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    n_hits = 0
    for d in range(S):
        recv = torch.cat([bufs[r][12 * sum(sent[r][:d]): 12 * sum(sent[r][:d + 1])] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()   # (the library works on its own stream: the concatenation must be complete)
        j = ctx.index_join_shard(parts[d], recv.data_ptr(), sum(sent[r][d] for r in range(S)))
        n_hits += hits_of(ctx, j)
        del j, recv
    return n_hits


if __name__ == "__main__":
    args = sys.argv[1:]
    sys.exit(main(*[int(x) for x in args[:2]], *(args[2:3])))
