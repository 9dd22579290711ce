"""Multi-GPU plumbing of the distance path: query rows are independent, so the N x N (or
Q x R) matrix is sharded by rows, block-cyclically: blocks of ROW_BLOCK consecutive rows are
dealt round-robin to the ranks (block b -> rank b mod world).  Neighbouring genomes of a
sorted collection are close relatives that share posting lists, so a block keeps them on one
GPU (and lets the kernel walk them in pairs), while the round-robin still balances the
triangle.  The reference index is sent to every rank with ONE broadcast and per-rank hits are
only concatenated -- there is no reduction.  Backend-agnostic: "nccl" (= RCCL over xGMI) on
GPUs, "gloo" in the CPU tests."""
import math

import numpy as np


ROW_BLOCK = 32  # rk_dist_opts.row_block used by the multi-GPU callers (whole 32-genome blocks: the tile kernel counts a tile once)


def rank_rows(n_rows, rank, world, row_block=ROW_BLOCK):
    """row_first/row_step of this rank (what rk_dist_opts takes, together with row_block)
    and the row indices it owns."""
    rows = np.arange(n_rows, dtype=np.int64)
    return rank, world, rows[(rows // row_block) % world == rank]


def rank_pairs(n_genomes, rank, world, row_block=ROW_BLOCK):
    """all-vs-all pairs (j > i) whose row i belongs to this rank."""
    rows = rank_rows(n_genomes, rank, world, row_block)[2]
    return int(((n_genomes - 1) - rows).sum())


def weak_scaling_genomes(base_genomes, world):
    """dataset size that keeps the pairs per GPU at the 1-GPU level: N(N-1)/2 ~ world * P1."""
    return int(round(base_genomes * math.sqrt(world)))


def broadcast_blob(blob, src, device, dist):
    """Broadcast a 1-D uint8 torch tensor from `src` (other ranks pass None): size first,
    then the payload in one collective.  Returns the tensor on every rank.  A collective that
    fails or times out (the process group's timeout: see init_timeout) is reported with the rank
    and the byte count instead of a bare backend error."""
    import torch
    rank = dist.get_rank()
    # (the byte count of the message is fixed on the host BEFORE anything can fail: the handler must not touch the device)
    n_known = "%d bytes" % blob.numel() if rank == src else "size not yet received"
    size = torch.tensor([blob.numel() if rank == src else 0], dtype=torch.int64, device=device)
    try:
        dist.broadcast(size, src)
        n = int(size.item())
        n_known = "%d bytes" % n
        if rank != src:
            blob = torch.empty(n, dtype=torch.uint8, device=device)
        dist.broadcast(blob, src)
        if device.type == "cuda":
            torch.cuda.synchronize(device)   # RCCL errors surface at the synchronisation
    except Exception as e:  # noqa: BLE001 -- every backend raises its own type
        raise RuntimeError("rank %d/%d: index broadcast from rank %d (%s) failed: %s"
                           % (rank, dist.get_world_size(), src, n_known, e)) from e
    return blob


def init_timeout():
    """timeout for torch.distributed.init_process_group: a rank that never arrives (a dead GPU, a missing xGMI link) must end
    the job with an error after two minutes, not hang it"""
    import datetime
    return datetime.timedelta(seconds=120)


def gather_hits(local_hits, dist, dst=0):
    """Concatenate per-rank structured hit arrays on `dst`, sorted by (row, col)."""
    world = dist.get_world_size()
    parts = [None] * world
    dist.all_gather_object(parts, local_hits.tobytes())
    if dist.get_rank() != dst:
        return None
    merged = np.concatenate([np.frombuffer(p, dtype=local_hits.dtype) for p in parts])
    return merged[np.lexsort((merged["col"], merged["row"]))]


# ---- sharded build (round 5): hash ranges build, rows join, ONE all-to-all of 12-byte tile records in between ------------
REC_BYTES = 12


def exchange_records(send, send_counts, dist, device, rec_bytes=REC_BYTES):
    """all-to-all of tile records: `send` = this rank's records contiguous by destination (uint8 tensor, rec_bytes each: REC_BYTES
    for tile records, capi.KEY_BYTES for the keys of a build from per-rank sketches), send_counts[d] = records for rank d.  Returns (recv uint8 tensor on `device`, records received).  RCCL: one
    all_to_all_single on device memory; gloo (CPU rehearsal): the same collective on host copies, or -- where the backend has no
    all-to-all -- one broadcast per source rank."""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    counts = torch.tensor(send_counts, dtype=torch.int64)
    table = [torch.zeros(world, dtype=torch.int64) for _ in range(world)]
    if dist.get_backend() == "nccl":
        table = [t.to(device) for t in table]
        dist.all_gather(table, counts.to(device))
        table = [t.cpu() for t in table]
    else:
        dist.all_gather(table, counts)
    recv_counts = [int(table[r][rank]) for r in range(world)]
    n_recv = sum(recv_counts)
    in_split = [int(c) * rec_bytes for c in send_counts]
    out_split = [c * rec_bytes for c in recv_counts]
    if dist.get_backend() == "nccl":
        recv = torch.empty(max(1, n_recv * rec_bytes), dtype=torch.uint8, device=device)
        dist.all_to_all_single(recv[: n_recv * rec_bytes], send[: sum(in_split)], out_split, in_split)
        return recv, n_recv
    host = send[: sum(in_split)].cpu()
    recv = torch.empty(n_recv * rec_bytes, dtype=torch.uint8)
    try:
        dist.all_to_all_single(recv, host, out_split, in_split)
    except Exception:  # noqa: BLE001 -- a backend without all-to-all: every rank's buffer travels whole, each takes its slice
        at = 0
        for r in range(world):
            n_r = int(table[r].sum()) * rec_bytes
            buf = host if r == rank else torch.empty(n_r, dtype=torch.uint8)
            dist.broadcast(buf, r)
            lo = int(table[r][:rank].sum()) * rec_bytes
            recv[at:at + out_split[r]] = buf[lo:lo + out_split[r]]
            at += out_split[r]
    out = torch.empty(max(1, n_recv * rec_bytes), dtype=torch.uint8, device=device)
    out[: n_recv * rec_bytes] = recv.to(device)
    return out, n_recv


def sharded_join_index(ctx, sketches, hash_bits, dist, device, stream=0):
    """this rank's join-only index of a sharded all-vs-all: build the lists of its hash range, exchange the tile records, sort what
    arrives (rk_index_build_shard -> rk_index_shard_records / _pack -> all-to-all -> rk_index_join_shard).  Returns
    (join index, part index, seconds spent [build, exchange, join build], records sent, records received)."""
    import time
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    t0 = time.perf_counter()
    part = ctx.index_build_shard(sketches, hash_bits, rank, world)
    counts = part.shard_records(world)
    send = torch.empty(max(1, sum(counts) * REC_BYTES), dtype=torch.uint8, device=device)
    part.shard_pack(send.data_ptr(), stream)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    recv, n_recv = exchange_records(send, counts, dist, device)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    join = ctx.index_join_shard(part, recv.data_ptr(), n_recv)
    t3 = time.perf_counter()
    return join, part, (t1 - t0, t2 - t1, t3 - t2), sum(counts), n_recv


# ---- sharded build from PER-RANK sketches: rank r holds only the sketches of its own genomes (a sketcher that ran on N ranks) --------
SIG_WORDS = 17   # capi.SIG_WORDS: u32 per genome of a signature
KEY_BYTES = 8    # capi.KEY_BYTES


def agree(ok, err, what, dist, device):
    """status agreement before the next collective: every rank says whether its local step `what` worked; if any failed, EVERY rank
    raises a RuntimeError that names the failing rank(s) and their errors -- no rank goes on into a collective the others never reach"""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
    if dist.get_backend() == "nccl":
        flag = flag.to(device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) == 1:
        return
    msgs = [None] * world
    dist.all_gather_object(msgs, None if ok else "%s: %s" % (what, err))
    failed = [(r, m) for r, m in enumerate(msgs) if m is not None]
    raise RuntimeError("rank %d/%d: %s failed on rank(s) %s -- %s" % (rank, world, what, ", ".join(str(r) for r, _ in failed),
                                                                  "; ".join("rank %d: %s" % (r, m) for r, m in failed)))


def _step(what, fn, dist, device):
    """runs this rank's local step, then agrees on its status with every rank (agree); returns fn()'s value"""
    out, ok, err = None, True, ""
    try:
        out = fn()
    except Exception as e:  # noqa: BLE001 -- whatever the step raised travels to every rank
        ok, err = False, "%s: %s" % (type(e).__name__, e)
    agree(ok, err, what, dist, device)
    return out


def _sync(device):
    import torch
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def gather_signatures(sig_local, n_local, genome_base, n_genomes, dist, device):
    """all-gather of the per-rank signatures (n_local * SIG_WORDS int32 each, ranks hold different genome counts: padded to the
    largest) into ONE tensor of n_genomes * SIG_WORDS in global genome order, on `device`.  Raises on every rank when the ranks'
    ranges are not contiguous in rank order or do not cover the collection."""
    import torch
    world = dist.get_world_size()
    nccl = dist.get_backend() == "nccl"
    where = device if nccl else torch.device("cpu")
    meta = torch.tensor([n_local, genome_base], dtype=torch.int64, device=where)
    table = [torch.zeros(2, dtype=torch.int64, device=where) for _ in range(world)]
    dist.all_gather(table, meta)
    counts = [int(t[0]) for t in table]
    bases = [int(t[1]) for t in table]
    want = [sum(counts[:r]) for r in range(world)]
    if bases != want or sum(counts) != n_genomes or min(counts) < 1:
        raise RuntimeError("rank %d/%d: the ranks' genomes are not contiguous ranges in rank order covering %d genomes (counts %s, bases %s)"
                           % (dist.get_rank(), world, n_genomes, counts, bases))
    cap = max(counts) * SIG_WORDS
    mine = torch.zeros(cap, dtype=torch.int32, device=where)
    mine[: n_local * SIG_WORDS] = sig_local[: n_local * SIG_WORDS].to(where)
    parts = [torch.empty(cap, dtype=torch.int32, device=where) for _ in range(world)]
    dist.all_gather(parts, mine)
    return torch.cat([p[: c * SIG_WORDS] for p, c in zip(parts, counts)]).to(device)


def sharded_join_index_local(ctx, local, genome_base, n_genomes, hash_bits, dist, device, stream=0):
    """this rank's join-only index of a sharded all-vs-all when every rank holds ONLY the sketches of its own genomes
    (genome_base .. genome_base + local.count - 1 of n_genomes; contiguous ranges in rank order): all-gather of the genomes'
    signatures (68 bytes each) -> split of the local sketches into keys by destination shard -> ONE all-to-all of the keys ->
    build of this rank's shard from the keys that arrived -> the tile records' all-to-all -> rk_index_join_shard.  Every local step
    is followed by a status agreement (agree): a failure on any rank raises on every rank before the next collective.
    Returns (join index, part index, seconds [signatures + their all-gather, key split, key exchange, key build + record pack, record
    exchange, join build], records sent, records received) -- what sharded_join_index returns, with its phases split finer."""
    import time
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    t = [time.perf_counter()]
    n_local = local.count

    def signature():
        sig = torch.empty(max(1, n_local * SIG_WORDS), dtype=torch.int32, device=device)
        ctx.sketches_signature(local, sig.data_ptr(), stream)
        _sync(device)
        return sig
    sig_local = _step("signature", signature, dist, device)
    sig_all = gather_signatures(sig_local, n_local, genome_base, n_genomes, dist, device)
    _sync(device)
    t.append(time.perf_counter())

    def split():
        counts = ctx.sketches_shard_keys(local, genome_base, n_genomes, hash_bits, world)
        send = torch.empty(max(1, sum(counts) * KEY_BYTES), dtype=torch.uint8, device=device)
        ctx.sketches_shard_pack(local, genome_base, n_genomes, hash_bits, world, send.data_ptr(), stream)
        _sync(device)
        return send, counts
    send, key_counts = _step("key split", split, dist, device)
    t.append(time.perf_counter())
    recv, n_keys = exchange_records(send, key_counts, dist, device, rec_bytes=KEY_BYTES)
    del send
    _sync(device)
    t.append(time.perf_counter())

    def build():
        part = ctx.index_build_shard_keys(recv.data_ptr(), n_keys, sig_all.data_ptr(), n_genomes, hash_bits, rank, world)
        counts = part.shard_records(world)
        rec = torch.empty(max(1, sum(counts) * REC_BYTES), dtype=torch.uint8, device=device)
        part.shard_pack(rec.data_ptr(), stream)
        _sync(device)
        return part, rec, counts
    part, rec, rec_counts = _step("key build", build, dist, device)
    del recv
    t.append(time.perf_counter())
    rec_recv, n_recv = exchange_records(rec, rec_counts, dist, device)
    del rec
    _sync(device)
    t.append(time.perf_counter())
    join = _step("join build", lambda: ctx.index_join_shard(part, rec_recv.data_ptr(), n_recv), dist, device)
    t.append(time.perf_counter())
    secs = tuple(b - a for a, b in zip(t[:-1], t[1:]))
    return join, part, secs, sum(rec_counts), n_recv
