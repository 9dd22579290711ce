"""The sharded build from PER-RANK sketches (rk_sketches_signature / rk_sketches_shard_keys / _pack, rk_index_build_shard_keys,
shard.sharded_join_index_local): every rank holds only its own genomes, cuts them into keys by destination shard, one all-to-all moves
the keys, every shard builds its lists from what arrived.  CPU tier: the wire format against a hand-computed case, and the status
agreement of the per-rank flow (two gloo ranks, a stub context that fails on rank 1).  GPU tier: the keys against the numpy model,
every key-built shard against rk_index_build_shard over the whole collection, the union of the joins against the oracle."""
import os
import socket

import numpy as np
import pytest

from oracle import oracle as ok
from rabbitkssd_amd import shard, synth

BITS = 20
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6


def genome_bits(n_genomes):
    gb = 1
    while (1 << gb) < n_genomes:
        gb += 1
    return gb


def model_keys(h, off, genome_base, n_genomes, hash_bits, n_shards):
    """the wire format: destination = top shard_bits of the hash; key = the remaining bits << gb | global genome id.
    Returns one uint64 array per destination, in walk order."""
    sb = n_shards.bit_length() - 1
    gb = genome_bits(n_genomes)
    h = np.asarray(h, dtype=np.uint64)
    gid = np.repeat(np.arange(len(off) - 1, dtype=np.uint64) + np.uint64(genome_base), np.diff(off).astype(np.int64))
    dest = (h >> np.uint64(hash_bits - sb)) if sb else np.zeros(len(h), dtype=np.uint64)
    rem = h & np.uint64((1 << (hash_bits - sb)) - 1)
    keys = (rem << np.uint64(gb)) | gid
    return [keys[dest == d] for d in range(n_shards)]


def model_signature(h, off):
    n = len(off) - 1
    sig = np.zeros((n, 17), dtype=np.uint32)
    for g in range(n):
        a = np.asarray(h[int(off[g]):int(off[g + 1])], dtype=np.uint64)
        sig[g, 0] = len(a)
        f = (a[:16] ^ (a[:16] >> np.uint64(32))) & np.uint64(0xFFFFFFFF)
        sig[g, 1:1 + len(f)] = f.astype(np.uint32)
    return sig.reshape(-1)


def test_wire_format_model_hand_case():
    # 8-bit hashes, 4 shards (top 2 bits), a collection of 5 genomes (gb = 3); this rank holds genomes 2 and 3
    h = np.array([0x05, 0x41, 0x80, 0xFF], dtype=np.uint32)
    off = np.array([0, 2, 4], dtype=np.uint64)
    got = model_keys(h, off, 2, 5, 8, 4)
    want = [[5 << 3 | 2], [1 << 3 | 2], [0 << 3 | 3], [63 << 3 | 3]]
    assert [list(map(int, g)) for g in got] == want
    assert genome_bits(1) == 1 and genome_bits(2) == 1 and genome_bits(3) == 2 and genome_bits(1024) == 10 and genome_bits(1025) == 11
    sig = model_signature(np.array([7, 9, 11], dtype=np.uint64), np.array([0, 0, 3], dtype=np.uint64)).reshape(2, 17)
    assert list(sig[0]) == [0] * 17 and list(sig[1][:4]) == [3, 7, 9, 11] and not sig[1][4:].any()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _StubPart:
    def shard_records(self, n):
        return [3] * n

    def shard_pack(self, ptr, stream=0):
        pass


class _StubLocal:
    def __init__(self, count):
        self.count = count


class _StubCtx:
    """the calls sharded_join_index_local makes, without a device; rank 1 fails at `fail`"""
    def __init__(self, rank, fail):
        self.rank, self.fail = rank, fail

    def _maybe(self, stage):
        if self.rank == 1 and self.fail == stage:
            from rabbitkssd_amd import capi
            raise capi.RkError(RK_ERR_UNSUPPORTED, "stub failure at the " + stage)

    def sketches_signature(self, local, ptr, stream=0):
        pass

    def sketches_shard_keys(self, local, genome_base, n_genomes, hash_bits, n_shards):
        self._maybe("split")
        return [2] * n_shards

    def sketches_shard_pack(self, *args):
        pass

    def index_build_shard_keys(self, *args):
        self._maybe("build")
        return _StubPart()

    def index_join_shard(self, part, ptr, n):
        self._maybe("join")
        return "join"


def _worker_agreement(rank, port, outdir, fail):
    import datetime
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=30))
    try:
        counts = [3, 5]   # (uneven ranges)
        try:
            shard.sharded_join_index_local(_StubCtx(rank, fail), _StubLocal(counts[rank]), [0, 3][rank], 8, BITS, dist, torch.device("cpu"))
            msg = "no error"
        except RuntimeError as e:
            msg = "RuntimeError: " + str(e)
        open(os.path.join(outdir, "r%d" % rank), "w").write(msg)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fail", ["split", "build", "join"])
def test_status_agreement_every_rank_raises(tmp_path, fail):
    import time
    import torch.multiprocessing as mp
    t0 = time.time()
    mp.spawn(_worker_agreement, args=(_free_port(), str(tmp_path), fail), nprocs=2, join=True)
    assert time.time() - t0 < 30
    for r in range(2):
        msg = open(tmp_path / ("r%d" % r)).read()
        assert msg.startswith("RuntimeError") and "failed on rank(s) 1 " in msg and "stub failure at the " + fail in msg, msg


# ---- GPU tier ----------------------------------------------------------------------------------------------------------
def _slices(n, cuts):
    b = [0] + list(cuts) + [n]
    return [(b[i], b[i + 1]) for i in range(len(b) - 1)]


def _local(ctx, h, off, a, b, wide=False):
    lh = h[int(off[a]):int(off[b])]
    loff = (off[a:b + 1] - off[a]).astype(np.uint64)
    return (ctx.sketches_from_host64(lh, loff) if wide else ctx.sketches_from_host(lh, loff)), lh, loff


def _ranks_keys(ctx, h, off, cuts, bits, S, wide=False):
    """one GPU plays the ranks: per rank its signature and keys (torch tensors) -> the all-gathered signatures and, per shard, the keys
    that would arrive (the all-to-all emulated by concatenation)"""
    import torch
    n = len(off) - 1
    sigs, sends, counts = [], [], []
    for a, b in _slices(n, cuts):
        loc, _, _ = _local(ctx, h, off, a, b, wide)
        sig = torch.empty((b - a) * 17, dtype=torch.int32, device="cuda")
        ctx.sketches_signature(loc, sig.data_ptr())
        cnt = ctx.sketches_shard_keys(loc, a, n, bits, S)
        buf = torch.empty(max(1, sum(cnt)), dtype=torch.int64, device="cuda")
        ctx.sketches_shard_pack(loc, a, n, bits, S, buf.data_ptr())
        torch.cuda.synchronize()
        sigs.append(sig)
        sends.append(buf)
        counts.append(cnt)
        del loc
    sig_all = torch.cat(sigs)
    recv = []
    for d in range(S):
        parts = [sends[r][sum(counts[r][:d]):sum(counts[r][:d + 1])] for r in range(len(sends))]
        recv.append((torch.cat(parts + [torch.zeros(1, dtype=torch.int64, device="cuda")]), sum(counts[r][d] for r in range(len(sends)))))
    torch.cuda.synchronize()   # (the library works on its own stream: the concatenations must be complete)
    return sig_all, recv


def _join_all(ctx, parts, S, metric=0, kmer=20, D=0.1):
    """the record exchange (concatenation), rk_index_join_shard and the joins of every shard: the union, sorted by (row, col)"""
    import torch
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    got = []
    for d in range(S):
        recv = torch.cat([bufs[r][12 * sum(sent[r][:d]): 12 * sum(sent[r][:d + 1])] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        j = ctx.index_join_shard(parts[d], recv.data_ptr(), sum(sent[r][d] for r in range(S)))
        got.append(ctx.dist_rows(j, None, 1, metric, kmer, D)[0])
        del j
    merged = np.concatenate(got)
    return merged[np.lexsort((merged["col"], merged["row"]))]


def _same_hits(mine, want):
    assert len(mine) == len(want)
    for f in ("row", "col", "common", "size0", "size1", "jorc", "dist"):   # (field for field: everything but the padding)
        assert np.array_equal(mine[f], want[f]), f


@pytest.mark.gpu
def test_gpu_split_matches_the_wire_format_model():
    import torch
    from rabbitkssd_amd import capi
    names, h, off = synth.clade_sketches(300, 120, 32, seed=61)
    n = len(names)
    ctx = capi.Context(0)
    for S in (2, 4, 8):
        for a, b in _slices(n, (37, 150, 151)):
            loc, lh, loff = _local(ctx, h, off, a, b)
            cnt = ctx.sketches_shard_keys(loc, a, n, 32, S)
            want = model_keys(lh, loff, a, n, 32, S)
            assert cnt == [len(w) for w in want]
            buf = torch.empty(max(1, sum(cnt)), dtype=torch.int64, device="cuda")
            ctx.sketches_shard_pack(loc, a, n, 32, S, buf.data_ptr())
            torch.cuda.synchronize()
            got = buf.cpu().numpy().view(np.uint64)
            for d in range(S):
                mine = got[sum(cnt[:d]):sum(cnt[:d + 1])]
                assert np.array_equal(np.sort(mine), np.sort(want[d])), (S, a, d)
            sig = torch.empty((b - a) * 17, dtype=torch.int32, device="cuda")
            ctx.sketches_signature(loc, sig.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(sig.cpu().numpy().view(np.uint32), model_signature(lh, loff))
            del loc
    ctx.close()


def _build_parity(h, off, bits, S, cuts, want, wide=False, kmer=20, D=0.1):
    """every shard built from keys against rk_index_build_shard over the whole collection (order, total, shard records), then the
    union of the joins against `want`"""
    from rabbitkssd_amd import capi
    n = len(off) - 1
    ctx = capi.Context(0)
    sig_all, recv = _ranks_keys(ctx, h, off, cuts, bits, S, wide)
    whole = ctx.sketches_from_host64(h, off) if wide else ctx.sketches_from_host(h, off)
    parts = []
    for d in range(S):
        ref = ctx.index_build_shard(whole, bits, d, S)
        keys, n_keys = recv[d]
        part = ctx.index_build_shard_keys(keys.data_ptr(), n_keys, sig_all.data_ptr(), n, bits, d, S)
        assert part.genomes == n and part.total == ref.total == n_keys, (d, part.total, ref.total, n_keys)
        assert np.array_equal(part.order, ref.order), d
        assert part.shard_records(S) == ref.shard_records(S), d
        parts.append(part)
        del ref
    mine = _join_all(ctx, parts, S, 0, kmer, D)
    _same_hits(mine, want)
    del parts, whole, sig_all, recv
    ctx.close()
    return mine


def _clade_want(h, off, bits):
    postings, counts = ok.index_build32(h, off, bits)
    want, _ = ok.index_dist32(counts, bits, postings, np.diff(off).astype(np.uint32), h, off, 1, 0, 20, 0.1)
    return want


@pytest.mark.gpu
def test_gpu_key_built_shards_equal_sketch_built_shards():
    from rabbitkssd_amd import capi
    names, h, off = synth.clade_sketches(1600, 120, BITS, strains_per_clade=40, seed=53)
    n = len(names)
    want = _clade_want(h, off, BITS)
    assert len(want) > 1000
    # the unsharded build agrees with the oracle as well
    ctx = capi.Context(0)
    full = ctx.dist_rows(ctx.index_build(ctx.sketches_from_host(h, off), BITS), None, 1, 0, 20, 0.1)[0]
    _same_hits(full, want)
    ctx.close()
    for S, cuts in ((2, (777,)), (4, (13, 700, 701)), (8, (1, 170, 333, 500, 901, 1200, 1399))):   # (uneven: clades cut across ranks)
        _build_parity(h, off, BITS, S, cuts, want)


@pytest.mark.gpu
def test_gpu_key_built_shards_in_passes_and_on_a_skewed_hash_space(monkeypatch):
    names, h, off = synth.clade_sketches(1600, 120, BITS, strains_per_clade=40, seed=57)
    monkeypatch.setenv("RK_INDEX_PASS_BITS", "2")   # (read by both builds: passes inside a shard)
    _build_parity(h, off, BITS, 4, (300, 301, 1111), _clade_want(h, off, BITS))
    monkeypatch.delenv("RK_INDEX_PASS_BITS")
    h2, off2 = synth.canonical_skew(h, off, BITS, levels=2)
    _build_parity(h2, off2, BITS, 4, (99, 800, 1500), _clade_want(h2, off2, BITS))


@pytest.mark.gpu
def test_gpu_key_built_shards_wide_hashes():
    # 36-bit hashes (the 64-bit layout): keys of 36 - shard_bits hash bits and 11 genome bits; hits as the oracle's and the
    # sketch-built shards' (checked shard by shard inside _build_parity)
    names, h, off = synth.clade_sketches(1500, 150, 36, kmer_size=24, seed=15, wide=True)
    uhash, ucount, postings = ok.index_build64(h, off)
    want, _ = ok.index_dist64(uhash, ucount, postings, np.diff(off).astype(np.uint32), h, off, 1, 0, 24, 0.05)
    assert len(want) > 1000
    for S, cuts in ((2, (600,)), (4, (10, 750, 1234))):
        _build_parity(h, off, 36, S, cuts, want, wide=True, kmer=24, D=0.05)


def _worker_local_gpu(rank, port, outdir):
    """two ranks share cuda:0; each uploads ONLY its own genomes (an uneven split) and calls sharded_join_index_local"""
    import torch
    import torch.distributed as dist
    from rabbitkssd_amd import capi
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        torch.cuda.set_device(0)
        ctx = capi.Context(0)
        names, h, off = synth.clade_sketches(1500, 120, BITS, strains_per_clade=40, seed=53)
        n = len(names)
        a, b = [(0, 611), (611, n)][rank]
        loc, _, _ = _local(ctx, h, off, a, b)
        join, part, secs, n_sent, n_recv = shard.sharded_join_index_local(ctx, loc, a, n, BITS, dist, torch.device("cuda", 0))
        assert join.products == 6 and n_sent > 0 and n_recv > 0 and len(secs) == 6
        mine, _ = ctx.dist_rows(join, None, 1, 0, 20, 0.1)
        assert np.all(part.shard_of(mine, 2, shard.ROW_BLOCK) == rank)
        merged = shard.gather_hits(mine, dist, 0)
        if rank == 0:
            want = _clade_want(h, off, BITS)
            assert len(want) > 1000
            _same_hits(merged, want)
            open(os.path.join(outdir, "ok"), "w").write("%d" % len(merged))
        del join, part, loc
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_two_ranks_from_their_own_sketches_one_gpu(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker_local_gpu, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    assert int(open(tmp_path / "ok").read()) > 1000


@pytest.mark.gpu
def test_gpu_key_built_shard_needs_less_memory():
    import torch
    from rabbitkssd_amd import capi
    n, S, bits = 50000, 8, 28
    hs, offs, _ = synth.scale_collection_torch(n)
    torch.cuda.synchronize()
    prep = capi.Context(0)
    whole = prep.sketches_from_dev(hs.data_ptr(), offs.data_ptr(), n)
    sig = torch.empty(n * 17, dtype=torch.int32, device="cuda")
    prep.sketches_signature(whole, sig.data_ptr())
    cnt = prep.sketches_shard_keys(whole, 0, n, bits, S)
    keys = torch.empty(sum(cnt), dtype=torch.int64, device="cuda")
    prep.sketches_shard_pack(whole, 0, n, bits, S, keys.data_ptr())
    torch.cuda.synchronize()
    del whole
    prep.close()
    d = S - 1
    mine = keys[sum(cnt[:d]):sum(cnt[:d + 1])].clone()
    del keys
    torch.cuda.synchronize()
    fresh = capi.Context(0)
    before = fresh.pool_stats()[0]
    part = fresh.index_build_shard_keys(mine.data_ptr(), cnt[d], sig.data_ptr(), n, bits, d, S)
    grow_keys = fresh.pool_stats()[0] - before
    order_k, total_k, rec_k = part.order, part.total, part.shard_records(S)
    del part
    fresh.close()
    fresh = capi.Context(0)
    sk = fresh.sketches_from_dev(hs.data_ptr(), offs.data_ptr(), n)
    before = fresh.pool_stats()[0]
    ref = fresh.index_build_shard(sk, bits, d, S)
    grow_sk = fresh.pool_stats()[0] - before
    assert total_k == ref.total == cnt[d] and np.array_equal(order_k, ref.order) and rec_k == ref.shard_records(S)
    del ref, sk
    fresh.close()
    assert grow_keys <= 0.5 * grow_sk, (grow_keys, grow_sk)


@pytest.mark.gpu
def test_gpu_refusals():
    import torch
    from rabbitkssd_amd import capi
    ctx = capi.Context(0)
    h = np.array([5, 9, 9, 12, 3, 4], dtype=np.uint32)   # genome 0 lists 9 twice
    off = np.array([0, 4, 6], dtype=np.uint64)
    dup = ctx.sketches_from_host(h, off)
    with pytest.raises(capi.RkError) as e:
        ctx.sketches_shard_keys(dup, 0, 2, BITS, 2)
    assert e.value.code == RK_ERR_UNSUPPORTED
    buf = torch.empty(16, dtype=torch.int64, device="cuda")
    with pytest.raises(capi.RkError) as e:
        ctx.sketches_shard_pack(dup, 0, 2, BITS, 2, buf.data_ptr())
    assert e.value.code == RK_ERR_UNSUPPORTED
    good = ctx.sketches_from_host(np.array([5, 9, 12, 3, 4], dtype=np.uint32), np.array([0, 3, 5], dtype=np.uint64))
    for S in (3, 128, 0):
        with pytest.raises(capi.RkError) as e:
            ctx.sketches_shard_keys(good, 0, 2, BITS, S)
        assert e.value.code == RK_ERR_ARG, S
        with pytest.raises(capi.RkError) as e:
            ctx.sketches_shard_pack(good, 0, 2, BITS, S, buf.data_ptr())
        assert e.value.code == RK_ERR_ARG, S
        with pytest.raises(capi.RkError) as e:
            ctx.index_build_shard_keys(buf.data_ptr(), 1, buf.data_ptr(), 2, BITS, 0, S)
        assert e.value.code == RK_ERR_ARG, S
    for base, total in ((1, 2), (0, 1), (5, 6)):   # genome_base + count > n_genomes
        with pytest.raises(capi.RkError) as e:
            ctx.sketches_shard_keys(good, base, total, BITS, 2)
        assert e.value.code == RK_ERR_ARG, (base, total)
    assert ctx.sketches_shard_keys(good, 4, 6, BITS, 2) == [5, 0]
    del dup, good
    ctx.close()


@pytest.mark.gpu
def test_gpu_pack_leaves_out_hashes_beyond_hash_bits():
    """hashes beyond hash_bits: rk_sketches_shard_keys refuses them (RK_ERR_ARG), rk_sketches_shard_pack writes the keys of all the
    others and nothing else -- its own count pass flags them into the library's scratch, never through a null pointer"""
    import torch
    from rabbitkssd_amd import capi
    rng = np.random.default_rng(3)
    parts = [np.unique(rng.integers(0, 1 << 22, size=300)).astype(np.uint32) for _ in range(40)]   # a quarter of them >= 2^20
    h = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    ctx = capi.Context(0)
    loc = ctx.sketches_from_host(h, off)
    with pytest.raises(capi.RkError) as e:
        ctx.sketches_shard_keys(loc, 5, 50, BITS, 4)
    assert e.value.code == RK_ERR_ARG
    keep = h < (1 << BITS)
    assert 0 < keep.sum() < len(h)
    inside = np.concatenate([p[p < (1 << BITS)] for p in parts])
    ioff = np.concatenate([[0], np.cumsum([int((p < (1 << BITS)).sum()) for p in parts])]).astype(np.uint64)
    want = model_keys(inside, ioff, 5, 50, BITS, 4)
    sentinel = -7
    buf = torch.full((len(h),), sentinel, dtype=torch.int64, device="cuda")
    ctx.sketches_shard_pack(loc, 5, 50, BITS, 4, buf.data_ptr())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    n_in = sum(len(w) for w in want)
    assert np.all(got[n_in:] == sentinel)
    got = got[:n_in].view(np.uint64)
    at = 0
    for d in range(4):
        assert np.array_equal(np.sort(got[at:at + len(want[d])]), np.sort(want[d])), d
        at += len(want[d])
    del loc
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pass_bits", [None, "2"])
def test_gpu_keys_outside_the_wire_format_are_refused(monkeypatch, pass_bits):
    """a received key with hash bits beyond the shard's range, or a genome id beyond the collection: RK_ERR_ARG (in one pass through
    the partition's histogram, in several through the pass filter), never a build that silently drops or cuts the key"""
    import torch
    from rabbitkssd_amd import capi
    names, h, off = synth.clade_sketches(300, 80, BITS, seed=21)
    n, S = len(names), 2
    gb = genome_bits(n)
    if pass_bits:
        monkeypatch.setenv("RK_INDEX_PASS_BITS", pass_bits)
    ctx = capi.Context(0)
    sig_all, recv = _ranks_keys(ctx, h, off, (120,), BITS, S)
    keys, n_keys = recv[0]
    good = ctx.index_build_shard_keys(keys.data_ptr(), n_keys, sig_all.data_ptr(), n, BITS, 0, S)
    assert good.total == n_keys
    del good
    for corrupt in (lambda k: k | (1 << 40), lambda k: ((k >> gb) << gb) | n):
        bad = keys.clone()
        bad[n_keys // 2] = corrupt(int(bad[n_keys // 2]))
        torch.cuda.synchronize()
        with pytest.raises(capi.RkError) as e:
            ctx.index_build_shard_keys(bad.data_ptr(), n_keys, sig_all.data_ptr(), n, BITS, 0, S)
        assert e.value.code == RK_ERR_ARG
    again = ctx.index_build_shard_keys(keys.data_ptr(), n_keys, sig_all.data_ptr(), n, BITS, 0, S)   # (the context is still sound)
    assert again.total == n_keys
    del again
    ctx.close()


@pytest.mark.gpu
def test_gpu_key_build_needs_seven_hash_bits_per_shard():
    """8-bit hashes over 4 shards leave 6 bits inside a shard: too few buckets for the two-pass partition -> RK_ERR_UNSUPPORTED"""
    from rabbitkssd_amd import capi
    rng = np.random.default_rng(5)
    parts = [np.unique(rng.integers(0, 256, size=40)).astype(np.uint32) for _ in range(30)]
    h = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    ctx = capi.Context(0)
    sig_all, recv = _ranks_keys(ctx, h, off, (11,), 8, 4)
    keys, n_keys = recv[1]
    with pytest.raises(capi.RkError) as e:
        ctx.index_build_shard_keys(keys.data_ptr(), n_keys, sig_all.data_ptr(), len(parts), 8, 1, 4)
    assert e.value.code == RK_ERR_UNSUPPORTED
    ctx.close()
