"""The sketch kernels at their chunk, ticket, queue and dedup edges (GPU): rk_sketch_kernel with both LDS images, the two-stage
scan, k_chunk_table, k_dedup, k_size_scan, k_csr_place and dedup_big.

Every case compares the downloaded CSR with the oracle genome by genome (32-bit and 64-bit layouts) and the window count with
the oracle's, exactly.  That a case reached its edge is asserted from the record of the call (rk_sketch_last_plan) and from the
numpy model of the candidate stream (tests/_sketch_ref.py) -- conditions on the inputs, computed without the kernels."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _sketch_ref as sr
from oracle import oracle as ok
from rabbitkssd_amd import capi

pytestmark = pytest.mark.gpu

FIXED = {(10, 6, 3): (20, 8), (8, 5, 2): (16, 6), (10, 7, 4): (20, 6)}   # the parameter sets with a compile-time kernel
LDS_KEYS = {False: 16384, True: 8192}    # k_dedup's LDS sort: 64 KiB of 32-bit / 64-bit keys


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def one(seq):
    return seq, np.array([0, len(seq)], dtype=np.uint64)


def oracle_sets(ps, genomes, min_count=1, quals=None):
    """per genome (seq, rec_off): (hash set of the oracle, its window count), eight genomes at a time"""
    def job(i):
        seq, off = genomes[i]
        off = np.asarray(off, dtype=np.uint64)
        if quals is None:
            h = ok.sketch_records(ps.param, ps.table, seq, off)
        else:
            h = ok.sketch_records_fastq(ps.param, ps.table, seq, quals[i], off, 0, min_count)
        return h, ok.count_windows(ps.param, seq, off)
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(job, range(len(genomes))))


def sketch(ctx, ps, genomes, min_count=1, quals=None):
    flt = ctx.filter(capi.params_init(*ps.ksl), ps.table)
    rec_off, genome_rec = [np.zeros(1, dtype=np.uint64)], [0]
    at, n_rec = 0, 0
    for seq, off in genomes:
        off = np.asarray(off, dtype=np.uint64)
        rec_off.append(off[1:] - off[0] + np.uint64(at))
        at += int(off[-1] - off[0]) if len(off) else 0
        n_rec += len(off) - 1
        genome_rec.append(n_rec)
    seq = np.concatenate([g[0] for g in genomes]) if genomes else np.zeros(0, dtype=np.uint8)
    rec_off, genome_rec = np.concatenate(rec_off), np.array(genome_rec, dtype=np.uint64)
    if quals is None:
        sk = ctx.sketch_batch(flt, seq, rec_off, genome_rec)
    else:
        sk = ctx.sketch_batch_fastq(flt, seq, np.concatenate(quals), rec_off, genome_rec, 0, min_count)
    return sk, ctx.sketch_last_plan()


def compare(sk, ps, wants):
    """the CSR against per-genome (hash set, windows) of the oracle: offsets, contents, layout, window count"""
    gh, goff = sk.download()
    assert sk.count == len(wants) and sk.is64 == (ps.hash_bits > 32)
    want_off = np.concatenate([[0], np.cumsum([len(h) for h, _ in wants])]).astype(np.uint64)
    bad = np.nonzero(np.diff(goff.astype(np.int64)) != np.diff(want_off.astype(np.int64)))[0]
    assert not len(bad), "genome %d of %d: %d hashes, the oracle has %d" % (
        bad[0], len(wants), int(goff[bad[0] + 1] - goff[bad[0]]), len(wants[bad[0]][0]))
    assert np.array_equal(goff, want_off)
    want_h = np.concatenate([h for h, _ in wants]) if wants else np.zeros(0, dtype=np.uint64)
    if not np.array_equal(gh.astype(np.uint64), want_h):
        g = int(np.searchsorted(want_off, np.nonzero(gh.astype(np.uint64) != want_h)[0][0], side="right")) - 1
        mine, want = gh[int(goff[g]):int(goff[g + 1])].astype(np.uint64), wants[g][0]
        raise AssertionError("genome %d of %d: %d foreign hashes, %d missing" % (
            g, len(wants), len(np.setdiff1d(mine, want)), len(np.setdiff1d(want, mine))))
    assert sk.windows == sum(w for _, w in wants)


def run(ctx, ps, genomes, min_count=1, quals=None, wants=None):
    sk, plan = sketch(ctx, ps, genomes, min_count, quals)
    compare(sk, ps, oracle_sets(ps, genomes, min_count, quals) if wants is None else wants)
    return plan


def expect_kernel(plan, ps, img):
    """the kernel and the image a context created under RK_SKETCH_IMG=img must have used for this parameter set"""
    fixed = FIXED.get(ps.ksl)
    if img == 2 and fixed:
        assert plan["image"] == 2 and plan["kernel"] == "rk_scan2_kernel<%d, %d>" % fixed and not plan["exact"]
        return
    image = 0 if img == 0 else 1   # the two-stage scan has compile-time variants only: the rest falls back to image 1
    exact = image == 0 and len(ps.selected) <= 4096
    assert plan["image"] == image and plan["exact"] == exact
    assert plan["kernel"] == "rk_sketch_kernel<%d, %d, %s, %d>" % ((fixed or (0, 0)) + ("true" if exact else "false", image))


# ---------------------------------------------------------------------------------------- a. seams of chunks, blocks, lanes
def seam_genome(ps, rng, cb):
    """a clean genome of k + 2 chunks with a planted k-mer ending e bases past a chunk boundary, past a block boundary inside
    a chunk and past a lane boundary, for every e in 0 .. k-1 (a different boundary for every e); and what the model says"""
    k, chunk = ps.k, cb * 1024
    ends = []
    for e in range(k):
        b = (e + 1) * chunk
        ends += [b + e, b + 512 - 16 * (e % 7) + e]
        if cb >= 2:
            ends.append(b + 1024 * (1 + e % (cb - 1)) + e)
    seq = sr.plant(ps, rng, (k + 2) * chunk - 5, ends)
    pos = sr.candidates(ps, seq, [0, len(seq)])[1]
    for e in range(k):
        past = pos - e
        assert np.any((past % chunk == 0) & (past > 0)), "no selected window ends %d past a chunk boundary" % e
        assert cb < 2 or np.any((past % 1024 == 0) & (past % chunk != 0)), "... %d past a block boundary" % e
        assert np.any((past % 16 == 0) & (past % 1024 != 0)), "... %d past a lane boundary" % e
    return one(seq)


def seam_genomes(ps, rng, cb):
    k, chunk = ps.k, cb * 1024
    genomes = [seam_genome(ps, rng, cb)]
    # genomes that end flush with their last block (the next one starts without a carry), and one base beyond; chunks of cb
    # blocks (odd and even over the values of cb) and last chunks of one and two blocks
    for n in (1024, 1025, 2048, 2049, chunk, chunk + 1, 2 * chunk + 1024, 2 * chunk + 2048, 1023, k, k - 1):
        genomes.append(one(sr.dense(ps, rng, n // k + 1)[:n]))
    # one N, and one record end, at every offset -k .. +k around a chunk, a block and a lane boundary: one genome per offset
    nblk = max(6, cb + 3)
    edges = [chunk, chunk + 1024, chunk + 1024 + 16 * 37]
    for b in edges:
        for o in range(-k, k + 1):
            g = sr.LUT[rng.integers(0, 4, nblk * 1024 - 7)]
            lo = b - 3 * k + (o % k)
            g[lo:lo + 6 * k] = sr.dense(ps, rng, 6)   # selected windows on both sides, at every phase over the offsets
            n_gen = g.copy()
            n_gen[b + o] = ord("N")
            genomes.append(one(n_gen))
            # (the separator takes the byte at b + o of the packed genome)
            genomes.append((np.delete(g, b + o), np.array([0, b + o, len(g) - 1], dtype=np.uint64)))
    # records of exactly 1,023 bases (with its separator: one block) and 1,024 bases
    d = sr.dense(ps, rng, 4 * 1024 // k + 1)
    genomes.append((d[:4 * 1023], np.arange(5, dtype=np.uint64) * 1023))
    genomes.append((d[:4 * 1024], np.arange(5, dtype=np.uint64) * 1024))
    return genomes


@pytest.mark.parametrize("ksl", [(10, 6, 3), (8, 5, 2), (10, 7, 4), (7, 4, 1), (16, 6, 3)])
@pytest.mark.parametrize("img", [2, 1, 0])
def test_seams_of_chunks_blocks_and_lanes(monkeypatch, img, ksl):
    monkeypatch.setenv("RK_SKETCH_IMG", str(img))
    ps = sr.param_set(*ksl)
    ctx = capi.Context(0)
    try:
        for cb in (1, 2, 3, 16):
            monkeypatch.setenv("RK_SKETCH_CB", str(cb))
            genomes = seam_genomes(ps, np.random.default_rng(1000 * img + 10 * sum(ksl) + cb), cb)
            plan = run(ctx, ps, genomes)
            expect_kernel(plan, ps, img)
            assert plan["chunk_blocks"] == cb
            assert plan["n_chunks"] == sum(-(-(-(-(len(s) + len(o) - 2) // 1024)) // cb) for s, o in genomes)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- f. what the generic kernel alone serves
@pytest.mark.parametrize("ksl,img", [((11, 7, 4), 2), ((16, 4, 1), 2), ((11, 6, 2), 2), ((11, 6, 2), 0), ((16, 4, 1), 0)])
def test_seams_under_parameter_sets_of_the_generic_kernel(monkeypatch, ksl, img):
    """28 inner bits (hi_shift > 0); a 32-base window with 16 inner bits; 65,536 selected entries, with which the 144 KiB image
    runs without its exact table"""
    monkeypatch.setenv("RK_SKETCH_IMG", str(img))
    monkeypatch.setenv("RK_SKETCH_CB", "3")
    ps = sr.param_set(*ksl)
    assert ksl != (11, 6, 2) or len(ps.selected) > 4096
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, seam_genomes(ps, np.random.default_rng(sum(ksl) + img), 3))
        expect_kernel(plan, ps, img)
        assert plan["kernel"].startswith("rk_sketch_kernel<0, 0, ") and plan["chunk_blocks"] == 3
        assert plan["exact"] == (img == 0 and ksl == (16, 4, 1))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- b. many genomes
def pool_genomes(ps, rng, lengths, dims=None):
    """genomes of the given lengths cut from planted k-mers, each distinct length sketched by the oracle once:
    (genomes, wants)"""
    body = sr.dense(ps, rng, max(lengths) // ps.k + 2, dims)
    distinct = sorted(set(lengths))
    by_len = dict(zip(distinct, oracle_sets(ps, [one(body[:n]) for n in distinct])))
    return [one(body[:n]) for n in lengths], [by_len[n] for n in lengths]


@pytest.mark.parametrize("n", [1025, 2049, 3000])
def test_many_genomes_with_empty_ones_between(n):
    """k_size_scan beyond its first round of 1,024 genomes, k_chunk_table over rows with equal first chunks"""
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(n)
    lengths = rng.integers(40, 3073, n)
    run70 = 990 if n > 1100 else 925   # (from 2,049 genomes on the run of 70 lies across the end of the scan's first round)
    for at in [0, n - 1, 500] + list(range(700, 702)) + list(range(run70, run70 + 70)):   # first, last, single, two, 70
        lengths[at] = 0
    assert lengths[run70 - 1] and lengths[run70 + 70] and lengths[499] and lengths[501] and lengths[699] and lengths[702]
    genomes, wants = pool_genomes(ps, rng, [int(x) for x in lengths])
    assert all((len(h) > 0) == (ln > 0) for (h, _), ln in zip(wants, lengths))
    ctx = capi.Context(0)
    try:
        sk, plan = sketch(ctx, ps, genomes)
        compare(sk, ps, wants)
        assert plan["chunk_blocks"] == 16 and plan["n_chunks"] == int(np.count_nonzero(lengths)) and plan["attempts"] == 1
    finally:
        ctx.close()


def test_calls_that_scan_nothing():
    """no genomes, and genomes of no bytes: no chunk, so no scan kernel -- the record says kernel "" and grid 0 -- while the sizes,
    offsets and the read-back still run; then empty genomes around one of 1,025 bytes"""
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(5)
    empty = (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))   # a genome without records
    ctx = capi.Context(0)
    try:
        for genomes in ([], [empty, one(np.zeros(0, dtype=np.uint8)), empty]):
            sk, plan = sketch(ctx, ps, genomes)
            assert (plan["kernel"], plan["grid"], plan["n_chunks"], plan["attempts"]) == ("", 0, 0, 1)
            gh, goff = sk.download()
            assert sk.count == len(genomes) and len(goff) == len(genomes) + 1 and not np.any(goff) and len(gh) == 0
            assert sk.windows == 0 and sk.total == 0
        genomes = [empty, empty, one(sr.dense(ps, rng, 1025 // ps.k + 1)[:1025]), empty]
        wants = oracle_sets(ps, genomes)
        assert [len(h) > 0 for h, _ in wants] == [False, False, True, False]
        plan = run(ctx, ps, genomes, wants=wants)
        assert (plan["n_chunks"], plan["grid"], plan["attempts"]) == (1, 1, 1) and plan["kernel"] != ""
    finally:
        ctx.close()


def test_more_genomes_than_twice_the_wave_slots():
    """the second branch of the chunk-length formula (n_genomes >= 2 * wave slots)"""
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(3)
    slots = num_cu() * 2 * 16
    n = 2 * slots + 17
    lengths = rng.integers(1, 1400, n)
    lengths[rng.integers(0, n, 40)] = 0
    genomes, wants = pool_genomes(ps, rng, [int(x) for x in lengths])
    ctx = capi.Context(0)
    try:
        sk, plan = sketch(ctx, ps, genomes)
        compare(sk, ps, wants)
        total_blocks = int(np.sum((lengths + 1023) // 1024))
        assert n >= 2 * plan["grid"] * 16 and plan["grid"] == 2 * num_cu()
        assert plan["chunk_blocks"] == max(16, -(-total_blocks // (2 * slots))) > 1
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- c. the drain that outlives its genome
@pytest.mark.parametrize("img", [2, 1, 0])
def test_drain_in_flight_when_the_wave_moves_to_another_genome(monkeypatch, img):
    """RK_SKETCH_CB=1, one-block and two-block genomes of planted k-mers, more than twice as many chunks as waves: the two-stage
    scan leaves a chunk with a drain of its second queue in flight and finishes it inside the next genome's chunk.  Neighbours
    are planted from disjoint halves of the selected entries: a dr_tuple stored into the wrong region is a foreign hash."""
    monkeypatch.setenv("RK_SKETCH_IMG", str(img))
    monkeypatch.setenv("RK_SKETCH_CB", "1")
    ps = sr.param_set(10, 6, 3)
    rng = np.random.default_rng(40 + img)
    n = 3 * num_cu() * 16
    lengths = rng.integers(700, 2049, n)
    genomes, wants = [None] * n, [None] * n
    for parity in (0, 1):
        sub = [int(x) for x in lengths[parity::2]]
        genomes[parity::2], wants[parity::2] = pool_genomes(ps, rng, sub, ps.selected[parity::2])
        # the genomes of a parity are prefixes of one body.  By the model every chunk ends with selected windows in its last 256
        # bases: they sit in the wave's queues when the chunk ends
        longest = max(genomes[parity::2], key=lambda g: len(g[0]))[0]
        pos = sr.candidates(ps, longest, [0, len(longest)])[1]
        for end in [1024] + sorted(set(sub)):
            assert np.any((pos >= end - 256) & (pos < end)), "no selected window at the end of a chunk"
    a, b = wants[0][0], wants[1][0]
    assert len(a) > 20 and len(b) > 20 and not len(np.intersect1d(a, b))
    ctx = capi.Context(0)
    try:
        sk, plan = sketch(ctx, ps, genomes)
        compare(sk, ps, wants)
        expect_kernel(plan, ps, img)
        assert plan["chunk_blocks"] == 1 and plan["n_chunks"] == int(np.sum((lengths + 1023) // 1024))
        assert plan["n_chunks"] >= 2 * plan["grid"] * 16   # most chunks are a wave's second or later one
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- d. ticket groups
@pytest.mark.parametrize("groups", [1, 2, 3, 5, 0])
@pytest.mark.parametrize("img", [2, 1, 0])
def test_ticket_groups(monkeypatch, img, groups):
    """chunk counts that give 1, 2, 3, 5 and the largest number of ticket groups (`groups` 0: 32, and grid / 16 on image 0).
    With w workgroups wanted (16 chunks each) the host takes n_groups = min(w, cap) / 16 and trims the grid to a multiple of
    8 * n_groups: w = 16 * n_groups + 15 is trimmed by 15 workgroups, whose chunks and all later ones come by ticket only.
    One group means fewer than 32 workgroups, which are never trimmed: there every chunk is some wave's first."""
    monkeypatch.setenv("RK_SKETCH_IMG", str(img))
    monkeypatch.setenv("RK_SKETCH_CB", "1")
    ps = sr.param_set(10, 6, 3)
    rng = np.random.default_rng(10 * img + groups)
    cap = num_cu() * (1 if img == 0 else 2)
    n_chunks = (16 * groups + 15) * 16 - 3 if groups else cap * 16 + 16 * 50 + 5
    # three long genomes (the group ranges cut through them) and a tail of one- and two-block ones
    blocks = [n_chunks // 4, n_chunks // 5, n_chunks // 7]
    while sum(blocks) < n_chunks:
        blocks.append(min(n_chunks - sum(blocks), int(rng.integers(1, 3))))
    order = rng.permutation(len(blocks))
    genomes = []
    for i in order:
        n = blocks[i] * 1024 - int(rng.integers(0, 1024))
        genomes.append(one(sr.LUT[rng.integers(0, 4, n)] if blocks[i] > 2 else sr.dense(ps, rng, n // ps.k + 1)[:n]))
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, genomes)
        expect_kernel(plan, ps, img)
        assert plan["chunk_blocks"] == 1 and plan["n_chunks"] == n_chunks
        if groups == 1:
            assert plan["n_groups"] == 1 and plan["grid"] == 31 and n_chunks > 30 * 16
        else:
            want_groups = groups or min(32, cap // 16)
            assert plan["n_groups"] == want_groups and plan["grid"] % (8 * want_groups) == 0
            assert n_chunks > plan["grid"] * 16                       # chunks beyond every wave's first: by ticket
            if groups:
                assert plan["grid"] == 16 * groups                    # 15 workgroups were trimmed away
            else:
                assert plan["grid"] == cap - cap % (8 * want_groups)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- e. dedup and capacity
def reg_cap(ps, length):
    return 2 * (length >> (4 * ps.ksl[2])) + 192   # the candidate region of a genome of `length` packed bytes


def length_for_cap(ps, cap):
    assert cap >= 192 and cap % 2 == 0
    return ((cap - 192) // 2) << (4 * ps.ksl[2])


def genome_with(ps, rng, n_cand, length):
    """a single-record genome of `length` bases with exactly n_cand candidates by the model: planted k-mers, cut, then N"""
    d = sr.dense(ps, rng, n_cand + 2)
    assert len(d) <= length, "%d candidates do not fit %d bases" % (n_cand, length)
    seq = np.full(length, ord("N"), dtype=np.uint8)
    seq[:len(d)] = sr.with_candidates(ps, d, n_cand)
    assert len(sr.candidates(ps, seq, [0, length])[0]) == n_cand
    return one(seq)


@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_dedup_candidate_counts_around_its_powers_of_two(ksl):
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(sum(ksl))
    counts = [0, 1, 2, 1023, 1024, 1025, 4096, 4097]
    genomes = [genome_with(ps, rng, n, max(length_for_cap(ps, max(192, n + n % 2)), (n + 2) * ps.k)) for n in counts]
    assert all(reg_cap(ps, len(g)) >= n for (g, _), n in zip(genomes, counts))
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, genomes)
        assert plan["attempts"] == 1 and plan["n_big"] == 0 and plan["max_candidates"] == 4097
    finally:
        ctx.close()


@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_candidate_region_exactly_full_and_one_beyond(ksl):
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(1 + sum(ksl))
    length = 300000
    cap = reg_cap(ps, length)
    small = genome_with(ps, rng, 7, 5000)
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, [small, genome_with(ps, rng, cap, length), small])
        assert (plan["attempts"], plan["max_candidates"], plan["max_reg_cap"]) == (1, cap, cap)
        plan = run(ctx, ps, [small, genome_with(ps, rng, cap + 1, length), small])
        assert (plan["attempts"], plan["max_candidates"], plan["max_reg_cap"]) == (2, cap + 1, cap + 1)   # exact on the retry
        assert plan["n_big"] == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_regions_at_the_lds_sort_ceiling_and_beyond(ksl):
    """reg_cap == the LDS sort's capacity (sorted in LDS, P == the ceiling with more than half of it in candidates) and the
    first reg_cap beyond it (device-wide sort), for 32-bit and for 64-bit keys"""
    ps = sr.param_set(*ksl)
    wide = ps.hash_bits > 32
    ceiling = LDS_KEYS[wide]
    rng = np.random.default_rng(2 + sum(ksl))
    at, beyond = length_for_cap(ps, ceiling), length_for_cap(ps, ceiling + 2)
    assert reg_cap(ps, at) == ceiling and reg_cap(ps, beyond) == ceiling + 2
    n_half = ceiling // 2 + 900
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, [genome_with(ps, rng, n_half, at), genome_with(ps, rng, 300, at)])
        assert (plan["attempts"], plan["n_big"], plan["max_reg_cap"], plan["max_candidates"]) == (1, 0, ceiling, n_half)
        plan = run(ctx, ps, [genome_with(ps, rng, 300, at), genome_with(ps, rng, n_half, beyond)])
        assert (plan["attempts"], plan["n_big"], plan["max_reg_cap"], plan["max_candidates"]) == (1, 1, ceiling + 2, n_half)
    finally:
        ctx.close()


@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_overflow_that_turns_the_genome_into_a_big_one(ksl):
    ps = sr.param_set(*ksl)
    ceiling = LDS_KEYS[ps.hash_bits > 32]
    rng = np.random.default_rng(3 + sum(ksl))
    n = ceiling + 500
    g = genome_with(ps, rng, n, (n + 2) * ps.k)
    assert reg_cap(ps, len(g[0])) < ceiling < n
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, [genome_with(ps, rng, 50, 4000), g])
        assert (plan["attempts"], plan["n_big"], plan["max_reg_cap"], plan["max_candidates"]) == (2, 1, n, n)
    finally:
        ctx.close()


def kmer_records(kmers, pad=0):
    """every k-mer a record of its own (one window each); `pad` bases of N as a last record widen the candidate region"""
    n, k = kmers.shape
    seq = np.concatenate([kmers.reshape(-1), np.full(pad, ord("N"), dtype=np.uint8)])
    off = np.concatenate([np.arange(n + 1) * k, [n * k + pad] if pad else []]).astype(np.uint64)
    return seq, off


def test_five_thousand_times_one_hash():
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(8)
    g = kmer_records(np.repeat(sr.planted_kmers(ps, rng, 1), 5000, axis=0))
    dr = sr.candidates(ps, *g)[0]
    assert len(dr) == 5000 and len(np.unique(dr)) == 1
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, [g, genome_with(ps, rng, 9, 3000)])
        assert plan["max_candidates"] == 5000 and plan["attempts"] == 2   # 5,000 candidates in 85 kB: the region overflows first
    finally:
        ctx.close()


@pytest.mark.parametrize("n_runs,big", [(2600, False), (3000, True)])
@pytest.mark.parametrize("min_count", [2, 3])
def test_occurrence_threshold_with_runs_across_threads_waves_and_blocks(min_count, n_runs, big):
    """min_count > 1 with more than 4,096 candidates: every thread of k_dedup owns a stretch of `per` > 1 sorted keys, and runs
    of min_count - 1, min_count and min_count + 1 equal hashes cross the stretches of two threads, of two waves and the
    128-element blocks of the sort; the same through the device-wide path"""
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(100 * min_count + n_runs)
    kmers = np.unique(sr.planted_kmers(ps, rng, n_runs), axis=0)
    reps = rng.integers(min_count - 1, min_count + 2, len(kmers))
    rows = rng.permutation(np.repeat(np.arange(len(kmers)), reps))
    n = len(rows)
    g = kmer_records(kmers[rows], pad=length_for_cap(ps, (LDS_KEYS[False] + 2) if big else n + n % 2))
    dr = np.sort(sr.candidates(ps, *g)[0])
    cap = reg_cap(ps, len(g[0]) + len(g[1]) - 2)
    assert len(dr) == n > 4096 and cap >= n and (cap > LDS_KEYS[False]) == big
    # runs of each length, and runs that straddle a thread's stretch, a wave's (64 threads) and a 128-element block
    starts = np.nonzero(np.concatenate([[True], dr[1:] != dr[:-1]]))[0]
    ends = np.concatenate([starts[1:], [n]])   # exclusive
    for want_len in (min_count - 1, min_count, min_count + 1):
        if want_len:
            assert np.any(ends - starts == want_len)
    per = -(-n // 1024)
    assert per > 1
    for stride in (per, 64 * per, 128):
        assert np.any((ends - 1) // stride != starts // stride), "no run of equal hashes crosses a multiple of %d" % stride
    quals = [np.full(len(g[0]), ord("I"), dtype=np.uint8)]
    ctx = capi.Context(0)
    try:
        plan = run(ctx, ps, [g], min_count, quals)
        assert (plan["attempts"], plan["n_big"], plan["max_candidates"]) == (1, 1 if big else 0, n)
        assert len(sr.kept(dr, min_count)) < len(starts)   # the threshold does drop hashes
    finally:
        ctx.close()
