"""Counted sketches on the GPU: rk_sketch_batch_counts through k_dedup<K, true>, dedup_big's run-length route and the placement of
the counts, rk_sketches_from_host_counts, and `rabbit_kssd sketch --abund` / `abund`.

The model is tests/_sketch_ref.py: the wanted counts are np.unique(candidates, return_counts=True), the survivors those with
count >= min_count (tests/_abund_ref.py: counted).  Every case compares hashes, offsets and counts exactly and asserts from the
record of the call (rk_sketch_last_plan: attempts, n_big, max_candidates) that it took the path it is about.  A second reference
that does not go through the model: the oracle's sketch_records_fastq at every least_num.

(A hash of all ones at 32 hash bits cannot be planted: the outer context of a canonical k-mer would have to be all T on both
sides, and then its reverse complement, which starts with A, is the smaller strand.)"""
import gzip
import os
import subprocess

import numpy as np
import pytest

import _abund_ref as ab
import _sketch_ref as sr
from conftest import ROOT
from oracle import oracle as ok
from rabbitkssd_amd import capi
from test_gpu_sketch_edges import LDS_KEYS, genome_with, kmer_records, length_for_cap, reg_cap

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "rabbitkssd_amd", "rabbit_kssd")
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6


def batch_args(genomes):
    rec_off, genome_rec = [np.zeros(1, dtype=np.uint64)], [0]
    at, n_rec = 0, 0
    for seq, off in genomes:
        off = np.asarray(off, dtype=np.uint64)
        rec_off.append(off[1:] - off[0] + np.uint64(at))
        at += int(off[-1] - off[0]) if len(off) else 0
        n_rec += len(off) - 1
        genome_rec.append(n_rec)
    seq = np.concatenate([g[0] for g in genomes]) if genomes else np.zeros(0, dtype=np.uint8)
    return seq, np.concatenate(rec_off), np.array(genome_rec, dtype=np.uint64)


def sketch_counted(ctx, ps, genomes, min_count=1, quals=None, least_qual=0):
    """(hashes, off, counts, plan) of rk_sketch_batch_counts"""
    flt = ctx.filter(capi.params_init(*ps.ksl), ps.table)
    seq, rec_off, genome_rec = batch_args(genomes)
    sk = ctx.sketch_batch_counts(flt, seq, rec_off, genome_rec, None if quals is None else np.concatenate(quals), least_qual, min_count)
    plan = ctx.sketch_last_plan()
    assert sk.has_counts and sk.is64 == (ps.hash_bits > 32) and sk.count == len(genomes)
    h, off = sk.download()
    return h, off, sk.download_counts(), plan


def sketch_plain(ctx, ps, genomes, min_count=1, quals=None, least_qual=0):
    flt = ctx.filter(capi.params_init(*ps.ksl), ps.table)
    seq, rec_off, genome_rec = batch_args(genomes)
    if quals is None:
        sk = ctx.sketch_batch(flt, seq, rec_off, genome_rec)
    else:
        sk = ctx.sketch_batch_fastq(flt, seq, np.concatenate(quals), rec_off, genome_rec, least_qual, min_count)
    return sk, ctx.sketch_last_plan()


def same(got, want):
    """hashes, offsets and counts of a counted call against the model's, exactly"""
    (h, off, c), (wh, woff, wc) = got, want
    assert np.array_equal(off, woff), "offsets differ (first at genome %d)" % int(np.nonzero(np.diff(off.astype(np.int64)) != np.diff(woff.astype(np.int64)))[0][:1].sum())
    assert np.array_equal(h.astype(np.uint64), wh), "hashes differ"
    assert c.dtype == np.uint32 and len(c) == len(wc)
    bad = np.nonzero(c != wc)[0]
    assert not len(bad), "%d of %d counts differ, first at %d: %d, the model has %d" % (len(bad), len(c), bad[0], c[bad[0]], wc[bad[0]])


def check(ctx, ps, genomes, min_count=1, quals=None, least_qual=0):
    h, off, c, plan = sketch_counted(ctx, ps, genomes, min_count, quals, least_qual)
    want = ab.counted(ps, genomes, min_count, quals, least_qual)
    same((h, off, c), want)
    return plan, want


def high_quals(genomes):
    return [np.full(len(g[0]), ord("I"), dtype=np.uint8) for g in genomes]


# ---------------------------------------------------------------------------------------- counted against uncounted
def read_set(ps, rng, n_reads=260, read_len=120):
    """reads sampled with repeats from one genome of planted k-mers, random qualities: (genome of one record per read, qualities); a
    last record of N widens the candidate region to 4,096 slots, so that the first attempt fits"""
    genome = sr.dense(ps, rng, 700)   # a coverage of two to three: counts from 1 to well beyond 3
    starts = rng.integers(0, len(genome) - read_len, n_reads)
    pad = length_for_cap(ps, 4096)
    seq = np.concatenate([genome[s:s + read_len] for s in starts] + [np.full(pad, ord("N"), dtype=np.uint8)])
    off = np.concatenate([np.arange(n_reads + 1) * read_len, [n_reads * read_len + pad]]).astype(np.uint64)
    assert n_reads * read_len // ps.k < 4096
    return (seq, off), rng.integers(33, 74, len(seq), dtype=np.uint8)


@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_counted_call_against_the_uncounted_one_and_the_model(ksl):
    ps = sr.param_set(*ksl)
    g, qual = read_set(ps, np.random.default_rng(sum(ksl)))
    ctx = capi.Context(0)
    try:
        for least_qual in (0, 35):
            full = ab.counted(ps, [g], 1, [qual], least_qual)
            assert full[2].max() >= 4 and full[2].min() == 1 and len(full[0]) > 50
            for min_count in (1, 2, 3):
                plan, want = check(ctx, ps, [g], min_count, [qual], least_qual)
                assert (plan["attempts"], plan["n_big"]) == (1, 0)
                assert len(want[0]) < len(full[0]) or min_count == 1   # the threshold drops hashes, the counts it leaves are not clipped
                sk, plan_u = sketch_plain(ctx, ps, [g], min_count, [qual], least_qual)
                assert not sk.has_counts and plan_u == plan
                with pytest.raises(capi.RkError) as e:
                    sk.download_counts()
                assert e.value.code == RK_ERR_UNSUPPORTED
                uh, uoff = sk.download()
                ch, coff, _, _ = sketch_counted(ctx, ps, [g], min_count, [qual], least_qual)
                assert uh.tobytes() == ch.tobytes() and uoff.tobytes() == coff.tobytes() and uh.dtype == ch.dtype
        gated, ungated = ab.counted(ps, [g], 1, [qual], 35), ab.counted(ps, [g], 1, [qual], 0)
        assert gated[2].sum() < ungated[2].sum()   # the gate removes windows before they are counted
    finally:
        ctx.close()


def test_survivors_at_every_threshold_are_the_oracle_s():
    """independent of the model: {h : count[h] >= n} == sketch_records_fastq(least_num = n) for n = 1 .. largest count + 1"""
    ps = sr.param_set(8, 5, 2)
    g, qual = read_set(ps, np.random.default_rng(77), n_reads=150)
    ctx = capi.Context(0)
    try:
        for least_qual in (0, 35):
            h, off, c, plan = sketch_counted(ctx, ps, [g], 1, [qual], least_qual)
            assert (plan["attempts"], plan["n_big"]) == (1, 0) and c.max() >= 3
            for n in range(1, int(c.max()) + 2):
                want = ok.sketch_records_fastq(ps.param, ps.table, g[0], qual, g[1], least_qual, n)
                assert np.array_equal(h[c >= n].astype(np.uint64), want), (least_qual, n)
            assert not np.any(c >= int(c.max()) + 1)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- sizes and alignment
@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_candidate_counts_around_the_powers_of_two(ksl):
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(sum(ksl))
    n_cand = [0, 1, 2, 1023, 1024, 1025, 4096, 4097]
    genomes = [genome_with(ps, rng, n, max(length_for_cap(ps, max(192, n + n % 2)), (n + 2) * ps.k)) for n in n_cand]
    ctx = capi.Context(0)
    try:
        plan, want = check(ctx, ps, genomes)
        assert (plan["attempts"], plan["n_big"], plan["max_candidates"]) == (1, 0, 4097)
        assert [int(want[2][int(a):int(b)].sum()) for a, b in zip(want[1][:-1], want[1][1:])] == n_cand   # every candidate is counted once
    finally:
        ctx.close()


def test_many_genomes_with_runs_of_empty_ones():
    """1,500 genomes cut from one body of few distinct k-mers (so that counts above 1 abound), runs of empty genomes among them: the
    counts stay aligned with the offsets beyond the size scan's first round of 1,024"""
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(1500)
    n = 1500
    pool = sr.planted_kmers(ps, rng, 25)
    body = pool[rng.integers(0, len(pool), 3072 // ps.k + 2)].reshape(-1)
    lengths = rng.integers(40, 3073, n)
    for at in [0, n - 1, 500] + list(range(700, 702)) + list(range(990, 1060)):
        lengths[at] = 0
    dr, pos, _ = sr.candidates(ps, body, [0, len(body)])
    hs, cs, off = [], [], [0]
    for ln in lengths:   # a prefix of the body holds the candidates that end inside it
        u, c = np.unique(dr[pos < ln], return_counts=True)
        hs.append(u), cs.append(c), off.append(off[-1] + len(u))
    want = (np.concatenate(hs), np.array(off, dtype=np.uint64), np.concatenate(cs).astype(np.uint32))
    assert want[2].max() >= 5 and np.count_nonzero(np.diff(off) == 0) >= 75
    genomes = [(body[:ln], np.array([0, ln], dtype=np.uint64)) for ln in lengths]
    ctx = capi.Context(0)
    try:
        h, off_, c, plan = sketch_counted(ctx, ps, genomes)
        same((h, off_, c), want)
        assert (plan["attempts"], plan["n_big"], plan["n_chunks"]) == (1, 0, int(np.count_nonzero(lengths)))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- runs across seams
@pytest.mark.parametrize("n_runs,big", [(2600, False), (3000, True)])
def test_runs_across_threads_waves_and_blocks(n_runs, big):
    """the construction of test_occurrence_threshold_with_runs_across_threads_waves_and_blocks with runs of 1 to 3 equal hashes:
    they cross the stretches of two threads, of two waves and the 128-element blocks of the sort; in LDS and device-wide"""
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(n_runs)
    kmers = np.unique(sr.planted_kmers(ps, rng, n_runs), axis=0)
    reps = rng.integers(1, 4, len(kmers))
    rows = rng.permutation(np.repeat(np.arange(len(kmers)), reps))
    n = len(rows)
    g = kmer_records(kmers[rows], pad=length_for_cap(ps, (LDS_KEYS[False] + 2) if big else n + n % 2))
    dr = np.sort(sr.candidates(ps, *g)[0])
    cap = reg_cap(ps, len(g[0]) + len(g[1]) - 2)
    assert len(dr) == n > 4096 and cap >= n and (cap > LDS_KEYS[False]) == big
    starts = np.nonzero(np.concatenate([[True], dr[1:] != dr[:-1]]))[0]
    ends = np.concatenate([starts[1:], [n]])   # exclusive
    for want_len in (1, 2, 3):
        assert np.any(ends - starts == want_len)
    per = -(-n // 1024)
    assert per > 1
    for stride in (per, 64 * per, 128):
        assert np.any((ends - 1) // stride != starts // stride), "no run of equal hashes crosses a multiple of %d" % stride
    ctx = capi.Context(0)
    try:
        for min_count in (1, 2):
            plan, want = check(ctx, ps, [g], min_count, high_quals([g]))
            assert (plan["attempts"], plan["n_big"], plan["max_candidates"]) == (1, 1 if big else 0, n)
            assert len(want[0]) == np.count_nonzero(ends - starts >= min_count) and (min_count == 1 or len(want[0]) < len(starts))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- long runs in LDS
def fitted(ps, kmers, cap=None):
    """every k-mer a record, padded so that the candidate region holds them all (`cap`: exactly that capacity)"""
    n = len(kmers)
    want_cap = cap if cap is not None else max(192, n + n % 2)
    pad = max(0, length_for_cap(ps, want_cap) - n * (ps.k + 1)) + 8
    g = kmer_records(kmers, pad=pad)
    assert reg_cap(ps, len(g[0]) + len(g[1]) - 2) == want_cap or cap is None
    assert reg_cap(ps, len(g[0]) + len(g[1]) - 2) >= n
    return g


def test_one_hash_five_thousand_times_among_others():
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(8)
    others = np.unique(sr.planted_kmers(ps, rng, 700), axis=0)
    kmers = np.concatenate([others[:350], np.repeat(sr.planted_kmers(ps, rng, 1), 5000, axis=0), others[350:]])
    g = fitted(ps, kmers[rng.permutation(len(kmers))])
    ctx = capi.Context(0)
    try:
        for min_count in (1, 2, 5000, 5001):
            plan, want = check(ctx, ps, [g, genome_with(ps, rng, 9, 3000)], min_count, high_quals([g, genome_with(ps, rng, 9, 3000)]))
            assert (plan["attempts"], plan["n_big"], plan["max_candidates"]) == (1, 0, len(kmers))
        assert ab.counted(ps, [g])[2].max() == 5000
    finally:
        ctx.close()


@pytest.mark.parametrize("ksl,n", [((8, 5, 2), 4096), ((8, 5, 2), LDS_KEYS[False]), ((11, 5, 2), LDS_KEYS[True])])
def test_one_hash_fills_the_whole_sorted_array(ksl, n):
    """n == P: no padding key at all, the run is the array -- at 4,096 and at the ceiling of the LDS sort in both widths"""
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(n)
    g = fitted(ps, np.repeat(sr.planted_kmers(ps, rng, 1), n, axis=0), cap=n)
    ctx = capi.Context(0)
    try:
        for min_count in (1, n, n + 1):
            plan, want = check(ctx, ps, [g], min_count, high_quals([g]))
            assert (plan["attempts"], plan["n_big"], plan["max_candidates"], plan["max_reg_cap"]) == (1, 0, n, n)
            assert (len(want[0]), list(want[2])) == ((1, [n]) if min_count <= n else (0, []))
    finally:
        ctx.close()


@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_the_largest_hash_repeated_up_to_where_the_padding_begins(ksl):
    """n no power of two and the run of the largest hash ends at a[n - 1]: the search must stop at n, not in the padding"""
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(5 + sum(ksl))
    kmers = np.unique(sr.planted_kmers(ps, rng, 700), axis=0)
    dr = sr.candidates(ps, *kmer_records(kmers))[0]
    assert len(dr) == len(kmers)
    top = int(np.argmax(dr))
    g = fitted(ps, np.concatenate([kmers, np.repeat(kmers[top:top + 1], 36, axis=0)]))
    want = ab.counted(ps, [g])
    n = int(want[2].sum())
    assert n & (n - 1) and want[2][-1] == 37 and want[0][-1] == dr.max()
    ctx = capi.Context(0)
    try:
        for min_count in (1, 37, 38):
            plan, _ = check(ctx, ps, [g], min_count, high_quals([g]))
            assert (plan["attempts"], plan["n_big"], plan["max_candidates"]) == (1, 0, n)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- overflow
@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_overflow_retry_and_overflow_into_a_big_genome_count_like_a_fit(ksl):
    ps = sr.param_set(*ksl)
    ceiling = LDS_KEYS[ps.hash_bits > 32]
    rng = np.random.default_rng(3 + sum(ksl))
    pool = np.unique(sr.planted_kmers(ps, rng, 900), axis=0)
    small = genome_with(ps, rng, 50, 4000)
    ctx = capi.Context(0)
    try:
        for n, n_big in ((3000, 0), (ceiling + 500, 1)):
            g = kmer_records(pool[rng.integers(0, len(pool), n)])   # no padding: the region is far too small
            assert reg_cap(ps, len(g[0]) + len(g[1]) - 2) < n
            for min_count in (1, 2):
                plan, want = check(ctx, ps, [small, g, small], min_count, high_quals([small, g, small]))
                assert (plan["attempts"], plan["n_big"], plan["max_candidates"], plan["max_reg_cap"]) == (2, n_big, n, n)
                assert want[2].max() >= 5
            fit = fitted(ps, kmer_records_kmers(g, ps.k), cap=None) if not n_big else None
            if fit is not None:   # the same k-mers in a region that holds them: one attempt, the same counts
                h, off, c, plan = sketch_counted(ctx, ps, [fit])
                assert plan["attempts"] == 1
                same((h, off, c), ab.counted(ps, [g]))
    finally:
        ctx.close()


def kmer_records_kmers(g, k):
    """the k-mers of a kmer_records genome without padding, as an n x k array"""
    return g[0].reshape(-1, k)


# ---------------------------------------------------------------------------------------- import
@pytest.mark.parametrize("wide", [False, True])
def test_import_round_trip_refusals_and_consumers(wide):
    rng = np.random.default_rng(11 + wide)
    bits = 36 if wide else 24
    dt = np.uint64 if wide else np.uint32
    sizes = [400, 0, 1, 350, 0, 380]
    # genomes that share hashes, so that the join has pairs to report
    base = np.unique(rng.integers(0, 1 << bits, 600))
    parts = [np.sort(rng.choice(base, n, replace=False)) for n in sizes]
    hashes = np.concatenate(parts).astype(dt)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    counts = rng.integers(1, 1000, len(hashes)).astype(np.uint32)
    counts[:3] = [1, 0xFFFFFFFF, 2]
    L = capi.lib()
    ctx = capi.Context(0)
    try:
        sk = ctx.sketches_from_host_counts(hashes, counts, off)
        assert sk.has_counts and sk.is64 == wide and sk.count == len(sizes) and sk.total == len(hashes)
        h, o = sk.download()
        assert h.tobytes() == hashes.tobytes() and np.array_equal(o, off) and np.array_equal(sk.download_counts(), counts)
        plain = (ctx.sketches_from_host64 if wide else ctx.sketches_from_host)(hashes, off)
        assert not plain.has_counts and L.rk_sketches_counts_dev(plain._h) is None and L.rk_sketches_counts_dev(sk._h) is not None
        # every consumer ignores the counts: the index and the self join of the counted object are those of the uncounted one
        i_c, i_p = ctx.index_build(sk, bits), ctx.index_build(plain, bits)
        lists = (lambda i: i.export64()) if wide else (lambda i: i.export_lists())
        assert [x.tobytes() for x in lists(i_c)] == [x.tobytes() for x in lists(i_p)] and len(lists(i_c)[0]) == len(hashes)
        r_c, r_p = ctx.dist_rows(i_c, None, 1, 0, 20, 1.0)[0], ctx.dist_rows(i_p, None, 1, 0, 20, 1.0)[0]
        assert len(r_c) > 0 and r_c.tobytes() == r_p.tobytes()
        q_c, q_p = ctx.dist_rows(i_p, sk, 0, 0, 20, 1.0)[0], ctx.dist_rows(i_p, plain, 0, 0, 20, 1.0)[0]
        assert len(q_c) > 0 and q_c.tobytes() == q_p.tobytes()
        # ---- refusals: descending hashes, a repeat, a zero count, nulls
        a, b = int(off[3]), int(off[3]) + 1
        for what in ("descending", "repeat", "zero"):
            bh, bc = hashes.copy(), counts.copy()
            if what == "descending":
                bh[[a, b]] = bh[[b, a]]
            elif what == "repeat":
                bh[b] = bh[a]
            else:
                bc[len(bc) - 1] = 0
            with pytest.raises(capi.RkError) as e:
                ctx.sketches_from_host_counts(bh, bc, off)
            assert e.value.code == RK_ERR_ARG, what
        bh = hashes.copy()
        bh[[0, int(off[3]) - 1]] = bh[[int(off[3]) - 1, 0]]   # a descent inside the first genome
        with pytest.raises(capi.RkError):
            ctx.sketches_from_host_counts(bh, counts, off)
        out = capi.C.c_void_p()
        p = lambda x: x.ctypes.data_as(capi.C.c_void_p)
        for args in ((None, p(hashes), p(counts), p(off)), (ctx._h, None, p(counts), p(off)), (ctx._h, p(hashes), None, p(off)), (ctx._h, p(hashes), p(counts), None)):
            assert L.rk_sketches_from_host_counts(args[0], args[1], int(wide), args[2], args[3], len(sizes), capi.C.byref(out)) == RK_ERR_ARG
        assert L.rk_sketches_from_host_counts(ctx._h, p(hashes), int(wide), p(counts), p(off), len(sizes), None) == RK_ERR_ARG
        assert L.rk_sketches_download_counts(sk._h, None) == RK_ERR_ARG
        # genomes of nothing at all
        empty = ctx.sketches_from_host_counts(np.zeros(0, dtype=dt), np.zeros(0, dtype=np.uint32), np.zeros(3, dtype=np.uint64))
        assert empty.has_counts and empty.total == 0 and len(empty.download_counts()) == 0
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- the tool
def tool(args, cwd, env=None):
    p = subprocess.run([TOOL] + [str(a) for a in args], cwd=cwd, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stderr.decode()


def fasta_text(name, seq, width=70, eol=b"\n"):
    body = seq.tobytes()
    return b">" + name.encode() + eol + eol.join(body[i:i + width] for i in range(0, len(body), width)) + eol


def fastq_text(reads, quals):
    return b"".join(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + q.tobytes() + b"\n" for i, (r, q) in enumerate(zip(reads, quals)))


def sidecar_of(tmp_path, stem, ksl):
    names, h, off = ab.read_sketches(tmp_path / (stem + ".sketch"), ksl)
    sizes, counts = ab.read_abund(tmp_path / (stem + ".sketch.abund"))
    assert np.array_equal(sizes, np.diff(off.astype(np.int64)))
    return names, h, off, counts


def test_tool_fasta_list_plain_gz_and_streamed(tmp_path):
    """a FASTA list through the packed batches, a .gz member, and a 1.3 MB file streamed in pieces of 64 KB (RK_STAGE_MB=1) whose
    repeated k-mers lie in different pieces; with index files.  The side-car is the model's, the other files those without --abund"""
    ksl = (8, 5, 2)
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(21)
    tool(["shuffle", "-k", ksl[0], "-s", ksl[1], "-l", ksl[2], "-o", "s.shuf"], tmp_path)
    pool = sr.planted_kmers(ps, rng, 40)
    genomes = []
    for i, n in enumerate((30_000, 55_000, 1_300_000, 20_000)):
        seq = sr.LUT[rng.integers(0, 4, n)]
        for at in rng.integers(0, n - ps.k, n // 400):   # the same few k-mers all over the file
            seq[at:at + ps.k] = pool[rng.integers(0, len(pool))]
        genomes.append((seq, np.array([0, n], dtype=np.uint64)))
    files = []
    for i, (seq, _) in enumerate(genomes):
        gz = i == 1
        path = tmp_path / ("g%d.fa%s" % (i, ".gz" if gz else ""))
        path.write_bytes(gzip.compress(fasta_text("g%d" % i, seq), 1, mtime=0) if gz else fasta_text("g%d" % i, seq))
        files.append(str(path))
    (tmp_path / "fa.list").write_text("".join(f + "\n" for f in files))
    env = {"RK_STAGE_MB": "1", "RK_BIG_PIECE_KB": "64", "RK_BIG_DEV_MB": "1", "RK_TIMING": "1"}
    err = tool(["sketch", "-i", "fa.list", "-L", "s.shuf", "-o", "ab", "-t", 4, "--abund"], tmp_path, env)
    assert "big file: " in err and int(err.split("big file: ")[1].split(" piece(s)")[0]) > 10 and ": upload + sketch of" in err
    tool(["sketch", "-i", "fa.list", "-L", "s.shuf", "-o", "pl", "-t", 4], tmp_path, env)
    for ext in (".sketch", ".sketch.dict", ".sketch.index"):
        assert (tmp_path / ("ab" + ext)).read_bytes() == (tmp_path / ("pl" + ext)).read_bytes(), ext
    assert not (tmp_path / "pl.sketch.abund").exists()
    names, h, off, counts = sidecar_of(tmp_path, "ab", ksl)
    want = ab.counted(ps, genomes)
    assert names == files
    same((h, off, counts), want)
    big = counts[int(off[2]):int(off[3])]
    assert big.max() >= 20   # a k-mer of the pool occurs all over the streamed file: its occurrences lie in different pieces
    p = subprocess.run([TOOL, "sketch", "-i", "ab.sketch", "-o", "copy.sketch", "--abund"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--abund" in p.stderr and not (tmp_path / "copy.sketch").exists()


def test_tool_fastq_plain_gz_streamed_and_the_threshold(tmp_path):
    """FASTQ, plain and .gz, the big one streamed by the sequential reader; then sketch -n 1 --abund -q followed by abund --min-count 2
    is sketch -n 2 -q, with the model's counts of the survivors"""
    ksl = (8, 5, 2)
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(22)
    tool(["shuffle", "-k", ksl[0], "-s", ksl[1], "-l", ksl[2], "-o", "s.shuf"], tmp_path)
    genome = sr.dense(ps, rng, 700)
    sets = []
    for n_reads in (600, 9000):
        starts = rng.integers(0, len(genome) - 150, n_reads)
        reads = np.stack([genome[s:s + 150] for s in starts])
        quals = rng.integers(33, 75, reads.shape, dtype=np.uint8)
        quals[::7, 0] = ord("@")
        sets.append((reads, quals))
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress(fastq_text(*sets[0]), 1, mtime=0))
    (tmp_path / "b.fq").write_bytes(fastq_text(*sets[1]))
    assert (tmp_path / "b.fq").stat().st_size > (2 << 20)
    files = [str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq")]
    (tmp_path / "fq.list").write_text("".join(f + "\n" for f in files))
    genomes = [(r.reshape(-1), np.arange(len(r) + 1, dtype=np.uint64) * 150) for r, _ in sets]
    quals = [q.reshape(-1) for _, q in sets]
    env = {"RK_STAGE_MB": "1", "RK_BIG_PIECE_KB": "64", "RK_BIG_DEV_MB": "1", "RK_TIMING": "1"}
    for least_qual in (0, 36):
        err = tool(["sketch", "-i", "fq.list", "-L", "s.shuf", "-o", "n1", "-t", 4, "-q", "-Q", least_qual, "-n", 1, "--abund"], tmp_path, env)
        assert "big file (sequential reader):" in err
        tool(["sketch", "-i", "fq.list", "-L", "s.shuf", "-o", "p1", "-t", 4, "-q", "-Q", least_qual, "-n", 1], tmp_path, env)
        assert (tmp_path / "n1.sketch").read_bytes() == (tmp_path / "p1.sketch").read_bytes()
        assert not (tmp_path / "n1.sketch.index").exists()
        names, h, off, counts = sidecar_of(tmp_path, "n1", ksl)
        assert names == files
        same((h, off, counts), ab.counted(ps, genomes, 1, quals, least_qual))
        assert counts.max() >= 10
        tool(["sketch", "-i", "fq.list", "-L", "s.shuf", "-o", "n2", "-t", 4, "-q", "-Q", least_qual, "-n", 2], tmp_path, env)
        tool(["abund", "-i", "n1.sketch", "--min-count", 2, "-o", "t2.sketch"], tmp_path)
        assert (tmp_path / "t2.sketch").read_bytes() == (tmp_path / "n2.sketch").read_bytes()
        _, h2, off2, counts2 = sidecar_of(tmp_path, "t2", ksl)
        want2 = ab.counted(ps, genomes, 2, quals, least_qual)
        same((h2, off2, counts2), want2)
        assert 0 < len(h2) < len(h)
        # -n 2 --abund: the full counts of the survivors, straight from the sketcher
        tool(["sketch", "-i", "fq.list", "-L", "s.shuf", "-o", "a2", "-t", 4, "-q", "-Q", least_qual, "-n", 2, "--abund"], tmp_path, env)
        assert (tmp_path / "a2.sketch").read_bytes() == (tmp_path / "n2.sketch").read_bytes()
        assert (tmp_path / "a2.sketch.abund").read_bytes() == (tmp_path / "t2.sketch.abund").read_bytes()


def test_tool_batch_call_route(tmp_path):
    """a big file with CR LF line ends is left to the serial reader by the streamed one: the whole file through
    rk_sketch_batch_counts (the batch call); 64-bit hashes, two records per file"""
    ksl = (11, 5, 2)
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(23)
    tool(["shuffle", "-k", ksl[0], "-s", ksl[1], "-l", ksl[2], "-o", "s.shuf"], tmp_path)
    pool = sr.planted_kmers(ps, rng, 30)
    genomes = []
    for i, n in enumerate((1_200_000, 40_000)):
        seq = sr.LUT[rng.integers(0, 4, n)]
        for at in rng.integers(0, n - ps.k, n // 500):
            seq[at:at + ps.k] = pool[rng.integers(0, len(pool))]
        cut = n // 3   # two records
        eol = b"\r\n" if i == 0 else b"\n"
        (tmp_path / ("w%d.fa" % i)).write_bytes(fasta_text("a", seq[:cut], eol=eol) + fasta_text("b", seq[cut:], eol=eol))
        genomes.append((seq, np.array([0, cut, n], dtype=np.uint64)))
    files = [str(tmp_path / "w0.fa"), str(tmp_path / "w1.fa")]
    (tmp_path / "w.list").write_text("".join(f + "\n" for f in files))
    env = {"RK_STAGE_MB": "1", "RK_TIMING": "1"}
    err = tool(["sketch", "-i", "w.list", "-L", "s.shuf", "-o", "w", "-t", 4, "-q", "--abund"], tmp_path, env)
    # the streamed reader gave w0.fa up before its sketch call (complete() never ran); w1.fa came in a packed batch
    assert "big file: " in err and "sketch kernels: 0.000 s" in err and ": upload + sketch of" in err
    names, h, off, counts = sidecar_of(tmp_path, "w", ksl)
    assert h.dtype == np.uint64
    same((h, off, counts), ab.counted(ps, genomes))
    assert counts.max() >= 20
    tool(["sketch", "-i", "w.list", "-L", "s.shuf", "-o", "wp", "-t", 4, "-q"], tmp_path, env)
    assert (tmp_path / "w.sketch").read_bytes() == (tmp_path / "wp.sketch").read_bytes()
