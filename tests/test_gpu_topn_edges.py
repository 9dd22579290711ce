"""`dist -N` on the device (rk_dist_topn: rk_distq_kernel counts-only + k_topn_select) at the edges of its selection rule, against
tests/_topn_ref.py -- the cells from the hash sets, the distances in float64 with the C library's log, the oracle's heap -- and against
rk_dist_rows + rk_topn_rows on the same inputs: all seven fields of every record, bit for bit, in the same order.

  a  collections and -N on the step seams (256, 1,280 cells) and the set seams (256, 1,024 bounds), six row patterns per call;
  b  kmer_size 1 .. 5 and -D 1.0 .. 2.0: shared cells beyond -D (the key-space reject at -D fires), shared cells in (1.0, -D],
     zero-common cells at exactly 1.0, and a row whose heap fills with zero-common cells ahead of farther shared cells;
  c  -D exactly on a cell's distance: emitted, never certain;
  d  one ratio from different triples, on both seams: equals after the seam replace nothing, a closer cell replaces one;
  e  the number of candidate records of a call (RK_MS_TOPN_CANDIDATES) equals the numpy model's (tests/test_topn_cpu.py), wherever
     the call took the device path -- asserted inside a .. d, f and g, and once more with a candidate buffer of 16 records;
  f  1 .. 5 rows of more than 2,048 candidates each: the key bits of the device sort;
  g  23 rows in block-cyclic shards whose last block is partial x batches of one and of three rows x the look-ups.

The count of (e) is exact only where a device log a few ulps off cannot flip a comparison: model_count() asserts first that any two
distinct values among a row's host distances and -D differ by more than 2^-30 relative (identical values are allowed: both sides
decide a tie the same way, and the key-space rejects only remove cells that would be neither emitted nor added)."""
import numpy as np
import pytest

import _topn_ref as tr
from _selfjoin_cases import csr
from rabbitkssd_amd import capi, synth
from test_topn_cpu import select_model

pytestmark = pytest.mark.gpu
FIELDS = ("row", "col", "common", "size0", "size1", "jorc", "dist")
TOPN_MAX = 1024      # kTopnMaxN: beyond it the call runs rk_dist_rows + rk_topn_rows inside


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    c.set_timing(True)     # (the candidate count of a call is kept with the stage times)
    return c


class Case:
    """reference sets, query sets and their cells (tests/_topn_ref.py), computed once and never changed"""
    def __init__(self, refs, queries, bits=24, wide=False, cell=None):
        self.refs, self.queries, self.bits, self.wide = refs, queries, bits, wide
        self.cell = cell if cell is not None else tr.cells(refs, queries)
        for a in self.cell:
            a.setflags(write=False)
        self._dist = {}

    def first(self, n_rows):
        """the case of the first n_rows queries"""
        return Case(self.refs, self.queries[:n_rows], self.bits, self.wide, (self.cell[0][:n_rows], self.cell[1], self.cell[2][:n_rows]))

    def upload(self, ctx):
        dtype, put = (np.uint64, ctx.sketches_from_host64) if self.wide else (np.uint32, ctx.sketches_from_host)
        return ctx.index_build(put(*csr(self.refs, dtype)), self.bits), put(*csr(self.queries, dtype))

    def dist(self, metric, k):
        """host distances float64[Q, R]"""
        if (metric, k) not in self._dist:
            common, size0, size1 = self.cell
            self._dist[(metric, k)] = np.array([tr.distances(common[q], size0, np.full(len(size0), size1[q]), metric, k)[1]
                                                for q in range(len(size1))]).reshape(len(size1), len(size0))
        return self._dist[(metric, k)]


def assert_same(mine, want, what):
    assert len(mine) == len(want), (what, len(mine), len(want))
    for f in FIELDS:
        a, b = np.ascontiguousarray(mine[f]), np.ascontiguousarray(want[f])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert not len(bad), (what, f, int(bad[0]), mine[bad[0]], want[bad[0]])


def model_count(case, metric, k, D, N, rows=None):
    """(candidates k_topn_select emits over the rows by the model, rows x R); asserts the separation condition of every row first"""
    common, size0, size1 = case.cell
    h = case.dist(metric, k)
    rows = range(len(size1)) if rows is None else rows
    total = 0
    for q in rows:
        v = np.unique(np.concatenate([h[q], [D]]))
        assert (np.diff(v) > 2.0 ** -30 * v[1:]).all(), ("two distinct distances closer than 2^-30", q, metric, k, D)
        total += len(select_model(common[q], size0, np.full(len(size0), size1[q]), metric, k, D, N, h[q]))
    return total, len(rows) * len(size0)


def check(ctx, idx, qs, case, metric, k, D, N, **shard):
    """one call against the reference, against the plain path, and its candidate count against the model; returns the records"""
    what = (len(case.refs), metric, k, D, N, shard)
    rows = tr.shard_rows(len(case.queries), **shard) if shard else None
    mine = ctx.dist_topn(idx, qs, metric, k, D, N, **shard)
    n_cand = ctx.last_ms(capi.MS_TOPN_CANDIDATES)
    assert_same(mine, tr.reference(case.cell, metric, k, D, N, rows), (what, "the reference"))
    assert_same(mine, capi.topn_rows(ctx.dist_rows(idx, qs, 0, metric, k, D, **shard)[0], N), (what, "rk_dist_rows + rk_topn_rows"))
    if N <= TOPN_MAX and D >= 1.0 and len(case.refs) and (rows is None or len(rows)):   # the device path
        want, every = model_count(case, metric, k, D, N, rows)
        print("candidates", what, "device", int(n_cand), "model", want, "cells", every)
        assert n_cand == want, (what, n_cand, want)
        assert want == every or n_cand < every, what     # where the model prunes, so does the kernel
    return mine


# ---- a. step and set seams --------------------------------------------------------------------------------------------------------
SEAM_R = (1, 2, 255, 256, 257, 511, 512, 513, 1279, 1280, 1281, 1500)
SEAM_N = (1, 2, 255, 256, 257, 1023, 1024, 1025)
ASC, DESC, RANDOM, SPARSE, SAME, EMPTY = range(6)
_seam = {}


def seam_case(R):
    """Six query rows against R references of one size S (the same-triple row needs one size, and a strictly descending row over
    R references of one size needs R different counts: S = R + R/4 + 120, beyond 500 from R = 304 on).  With one size both metrics
    are monotone in `common`.  Empty references: column 0, R // 3 and R - 2 (R = 2: column 0; R = 1: none)."""
    if R not in _seam:
        rng, pool = np.random.default_rng(100 + R), tr.Pool(24, 100 + R)
        S = R + R // 4 + 120
        sizes = np.full(R, S)
        sizes[np.array([0, R // 3, R - 2] if R >= 255 else ([0] if R == 2 else []), dtype=np.int64)] = 0
        col = np.arange(R)
        common = np.zeros((6, R), dtype=np.int64)
        common[ASC] = (R - col) // 4 + 1                       # distance ascending with the column: only the first N matter
        common[DESC] = col + 1                                 # strictly descending: every cell a candidate
        common[RANDOM] = rng.integers(0, 61, size=R)
        common[SPARSE] = np.where(rng.random(R) < 0.9, 0, rng.integers(1, 31, size=R))
        common[SAME] = 7
        common[:, sizes == 0] = 0
        queries = [np.sort(pool.take(n)) for n in (R // 4 + 11, R + 15, 200, 90, 50, 0)]
        _seam[R] = Case([r.astype(np.uint32) for r in tr.build_refs(pool, rng, queries, common, sizes)],
                        [q.astype(np.uint32) for q in queries])
        assert np.array_equal(_seam[R].cell[0], common)
    return _seam[R]


@pytest.mark.parametrize("R", SEAM_R)
def test_step_and_set_seams(ctx, R):
    case = seam_case(R)
    idx, qs = case.upload(ctx)
    for metric in (0, 1):
        h = case.dist(metric, 20)
        live = case.cell[1] > 0
        assert (np.diff(h[ASC][live]) >= 0).all() and (np.diff(h[DESC][live]) < 0).all() and len(np.unique(h[SAME][live])) == 1
        assert (h[EMPTY] == 1.0).all() and (R < 255 or (h[SPARSE] == 1.0).mean() >= 0.8) and (h[:, ~live] == 1.0).all()
        got = {N: check(ctx, idx, qs, case, metric, 20, 1.0, N) for N in SEAM_N}
        for N in SEAM_N:
            assert len(got[N]) == 6 * min(N, R)     # -D 1.0 keeps every cell: N records per row, R where N > R
        # N > R and N = 1025 (the plain path inside the call) against their neighbours: from N = R on the heap turns nothing away,
        # the pushes and so the pops are the same -- one sequence of bytes, which check() has compared with the reference's
        whole = [N for N in SEAM_N if N >= R]
        for N in whole[1:]:
            assert got[N].tobytes() == got[whole[0]].tobytes(), (R, metric, N)


# ---- b. small k ---------------------------------------------------------------------------------------------------------------------
SMALL_D = (1.0, 1.5, 2.0)
SPECIAL = 2          # the row with two shared cells at or below 1.0
_small = {}


def small_k_case(R, k):
    """Two general rows and the special row.  A cell's `common` is drawn through a target containment distance, so that the rows
    hold distances on both sides of 1.0, 1.5 and 2.0; three columns (one per step region) hold one hash of every query and are big
    enough for a distance beyond 2.0 under both metrics: 500 hashes up to k = 3; at k = 5 that takes sketches of more than e^10 =
    22,026 hashes on BOTH sides (containment divides by the smaller one), so there the queries hold 23,000 and those three references
    26,000.  The special row: two shared cells at or below 1.0 (columns R // 4 and R - 10), every other shared cell beyond 1.0."""
    if (R, k) not in _small:
        rng, pool = np.random.default_rng(1000 * k + R), tr.Pool(24, 1000 * k + R)
        s1 = {1: (120, 300, 480), 2: (120, 300, 480), 3: (480, 470, 460), 5: (23000, 23100, 23200)}[k]
        far, near = [3, R // 2, R - 3], [R // 4, R - 10]
        sizes = rng.integers(20, 501, size=R)
        sizes[far], sizes[near] = (26000 if k == 5 else 500), 500
        common = np.zeros((3, R), dtype=np.int64)
        for j in range(R):
            left = int(sizes[j])
            for q in (0, 1, SPECIAL):
                lo = 0.05 if q == j % 2 else 1.05
                c = int(round(np.exp(-k * rng.uniform(lo, 2.6)) * min(left, s1[q])))
                if rng.random() < 0.3:
                    c = 0
                common[q, j] = min(c, left, s1[q])
                left -= common[q, j]
        common[:, far] = 1
        common[:, near] = [[20], [20], [450]]
        if k == 5:   # against 23,000 hashes a cell in (1.0, 1.5] by jaccard that is beyond 1.0 by containment too: 9 of a reference's 1,500
            mid = [7, R // 2 + 5, R - 7]
            sizes[mid], common[:, mid] = 1500, 9
        # the special row: no other shared cell at or below 1.0, under either metric
        for metric in (0, 1):
            d = tr.distances(common[SPECIAL], sizes, np.full(R, s1[SPECIAL]), metric, k)[1]
            d[near] = 2.0
            common[SPECIAL, (d <= 1.0) & (common[SPECIAL] > 0)] = 0
        queries = [np.sort(pool.take(n)) for n in s1]
        _small[(R, k)] = Case([r.astype(np.uint32) for r in tr.build_refs(pool, rng, queries, common, sizes)],
                              [q.astype(np.uint32) for q in queries])
        assert np.array_equal(_small[(R, k)].cell[0], common)
    return _small[(R, k)]


@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("R", [257, 1281])
def test_small_k_cells_beyond_the_threshold_and_beyond_one(ctx, R, k):
    case = small_k_case(R, k)
    common = case.cell[0]
    idx, qs = case.upload(ctx)
    for metric in (0, 1):
        h = case.dist(metric, k)
        shared = common > 0
        assert ((shared[SPECIAL]) & (h[SPECIAL] <= 1.0)).sum() == 2
        for D in SMALL_D:
            for q in range(3):   # the three classes, in every row (at -D 1.0 the interval (1.0, -D] is empty by definition)
                assert (shared[q] & (h[q] > D)).any() and (~shared[q]).sum() >= 10, (metric, D, q)
                assert D == 1.0 or (shared[q] & (h[q] > 1.0) & (h[q] <= D)).any(), (metric, D, q)
            for N in (1, 3, 256):
                mine = check(ctx, idx, qs, case, metric, k, D, N)
                zeros = np.nonzero(~shared[SPECIAL])[0]
                assert R < 1281 or len(zeros) >= 254
                if N > 2 and len(zeros) >= N - 2:
                    # the special row: its two near cells and zero-common cells at exactly 1.0 -- N - 2 of the row's first N: once N
                    # cells at or below 1.0 are in, nothing at 1.0 or beyond gets in, and a shared cell beyond 1.0 displaces none
                    row = mine[mine["row"] == SPECIAL]
                    assert len(row) == N and (row["common"] > 0).sum() == 2 and (row["dist"] <= 1.0).all()
                    assert set(row["col"][row["common"] == 0].tolist()) <= set(zeros[:N].tolist()), (metric, D, N)


# ---- c. a cell on the threshold -----------------------------------------------------------------------------------------------------
THRESHOLD_R, THRESHOLD_K = 700, 2
CHOSEN = ((0, 100), (1, 500), (2, 600))     # (row, column) of the cell that gives -D: first step, a later step, the row's last stream cell
_threshold = []


def threshold_case():
    """Three rows of 300 hashes at kmer_size 2; the chosen cell of a row is (7, 59, 300): 1.07 by containment, 1.62 by jaccard, and no
    other cell of the row has its distance (the test asserts it).  After its chosen cell row 2 holds only cells that share one hash with references
    of 200 hashes or more (beyond 2.6 under both metrics), so the chosen cell is the last cell of its stream."""
    if not _threshold:
        rng, pool = np.random.default_rng(77), tr.Pool(23, 77)
        R, k = THRESHOLD_R, THRESHOLD_K
        sizes = rng.integers(61, 301, size=R)
        common = np.zeros((3, R), dtype=np.int64)
        for j in range(R):
            left = int(sizes[j])
            for q in range(3):
                c = 0 if rng.random() < 0.5 else int(round(np.exp(-k * rng.uniform(0.2, 2.6)) * left))
                common[q, j] = min(c, left, 300)
                left -= common[q, j]
        sizes[601:] = rng.integers(200, 301, size=R - 601)
        common[:, 601:] = [[0], [0], [1]]
        for q, j in CHOSEN:
            sizes[j], common[:, j] = 59, 0
            common[q, j] = 7
        queries = [np.sort(pool.take(300)) for _ in range(3)]
        _threshold.append(Case([r.astype(np.uint32) for r in tr.build_refs(pool, rng, queries, common, sizes)],
                               [q.astype(np.uint32) for q in queries], bits=23))
        assert np.array_equal(_threshold[0].cell[0], common)
    return _threshold[0]


@pytest.mark.parametrize("row,col", CHOSEN)
def test_a_cell_exactly_on_the_threshold(ctx, row, col):
    case = threshold_case()
    idx, qs = case.upload(ctx)
    for metric in (0, 1):
        h = case.dist(metric, THRESHOLD_K)
        D = float(h[row, col])
        assert D >= 1.0 and (h[row] == D).sum() == 1
        beyond = np.nonzero(h[row] == h[row][h[row] > D].min())[0]     # the next larger distinct value of the row
        stream = np.nonzero(h[row] <= D)[0]
        n_stream = len(stream)
        assert 256 < n_stream < TOPN_MAX
        if row == 2:
            assert stream[-1] == col     # the N-th cell of its stream at N = n_stream: it fills the heap, and the kernel never counts it
        for N in (n_stream, n_stream + 1, TOPN_MAX, n_stream - 1, 3):
            mine = check(ctx, idx, qs, case, metric, THRESHOLD_K, D, N)
            cols = mine["col"][mine["row"] == row]
            assert (col in cols) == (N >= n_stream) and not np.isin(beyond, cols).any(), (metric, N)
            if N >= n_stream:
                assert sorted(cols.tolist()) == stream.tolist() and cols[0] == col     # popped first: the farthest of the heap


# ---- d. ties --------------------------------------------------------------------------------------------------------------------------
TIE_R = 1400
GROUPS = ((250, 262), (1275, 1290))     # the tie group of row 0 and of row 1, first and last column: across 256 and across 1,280
_ties = {}


def tie_case(metric):
    """Two rows; row r has a group of cells of ONE ratio from three different triples at the columns GROUPS[r] (containment 1/2 as
    2/4, 3/6, 50/100 under a query of 200; jaccard 1/3 as 10/(20+20-10), 15/(40+20-15), 20/(60+20-20) under a query of 20), one closer
    cell three columns behind the group, and everywhere else cells that are farther than the group."""
    if metric not in _ties:
        rng, pool = np.random.default_rng(31 + metric), tr.Pool(22, 31 + metric)
        s1, triples, closer = (200, ((2, 4), (3, 6), (50, 100)), (100, 199)) if metric else (20, ((10, 20), (15, 40), (20, 60)), (20, 59))
        sizes = rng.integers(60, 151, size=TIE_R)
        common = np.zeros((2, TIE_R), dtype=np.int64)
        for q in range(2):
            common[q] = np.where(rng.random(TIE_R) < 0.3, 0, np.minimum(rng.integers(0, 10, size=TIE_R), s1 // 2 - 1))
        for q, (lo, hi) in enumerate(GROUPS):
            for j in range(lo, hi + 1):
                c, sizes[j] = triples[(j - lo) % 3]
                common[:, j] = 0
                common[q, j] = c
            common[:, hi + 3] = 0
            common[q, hi + 3], sizes[hi + 3] = closer
        queries = [np.sort(pool.take(s1)) for _ in range(2)]
        _ties[metric] = Case([r.astype(np.uint32) for r in tr.build_refs(pool, rng, queries, common, sizes)],
                             [q.astype(np.uint32) for q in queries], bits=22)
        assert np.array_equal(_ties[metric].cell[0], common)
    return _ties[metric]


@pytest.mark.parametrize("tie_metric", [0, 1])
def test_ties_across_the_step_seams(ctx, tie_metric):
    case = tie_case(tie_metric)
    idx, qs = case.upload(ctx)
    h = case.dist(tie_metric, 20)
    seams = (256, 1280)
    for q, (lo, hi) in enumerate(GROUPS):
        group = np.arange(lo, hi + 1)
        assert len(np.unique(h[q, group])) == 1 and len(set(zip(case.cell[0][q, group].tolist(), case.cell[1][group].tolist()))) == 3
        v = h[q, lo]
        assert h[q, hi + 3] < v and (np.delete(h[q], np.append(group, hi + 3)) > v).all()
        assert lo < seams[q] <= hi
    for metric in (tie_metric, 1 - tie_metric):     # (the other metric: the same sets, no designed ties)
        for N in (1, 2, 5, 6, 7, 13, 16, 17, 100):
            mine = check(ctx, idx, qs, case, metric, 20, 1.0, N)
            if metric != tie_metric:
                continue
            for q, (lo, hi) in enumerate(GROUPS):
                cols = mine["col"][mine["row"] == q]
                before, after = seams[q] - lo, hi + 1 - seams[q]
                assert cols[-1] == hi + 3 and len(cols) == N     # the closer cell: in, and popped last
                if N <= hi + 1 - lo:
                    # the first N equals filled the heap, a later equal never replaces (strict <), the closer cell replaced the top:
                    # N - 1 of the first N stay -- for N <= `before` nothing from beyond the seam, though the kernel emits those cells
                    assert set(cols[:-1].tolist()) <= set(range(lo, lo + N)) and len(set(cols.tolist())) == N
                    assert N > before or not np.isin(np.arange(seams[q], hi + 1), cols).any()
                assert before in (5, 6) and after >= 7


# ---- e. the candidate count under a candidate buffer of 16 records --------------------------------------------------------------------
def test_candidate_count_is_unchanged_by_the_retry(monkeypatch):
    case = seam_case(513)
    monkeypatch.setenv("RK_TOPN_CAND_CAP", "16")
    small = capi.Context(0)
    small.set_timing(True)
    idx, qs = case.upload(small)
    for metric in (0, 1):
        for N in (2, 257):
            check(small, idx, qs, case, metric, 20, 1.0, N)     # (asserts the count against the model)
            assert small.last_ms(capi.MS_TOPN_CANDIDATES) > 16
    small.close()


# ---- f. key bits of the device sort -----------------------------------------------------------------------------------------------------
def test_key_bits_of_the_device_sort(ctx):
    """Reference j holds j + 1 hashes of the rows' common base and two private ones: strictly descending under both metrics, all
    2,500 cells of every row are candidates -- more than the 2,048 from which the candidates are ordered on the device, with 33 key
    bits at one and two rows, 34 at three, 35 at five."""
    R = 2500
    rng, pool = np.random.default_rng(9), tr.Pool(24, 9)
    base = np.sort(pool.take(2600))
    refs = [r.astype(np.uint32) for r in tr.build_refs(pool, rng, [base], [np.arange(R) + 1], np.arange(R) + 3)]
    queries = [np.sort(np.concatenate([base, pool.take(7 * r)])).astype(np.uint32) for r in range(5)]
    whole = Case(refs, queries)
    assert (whole.cell[0] == np.arange(R) + 1).all()
    for Q in (1, 2, 3, 5):
        case = whole.first(Q)
        idx, qs = case.upload(ctx)
        for metric in (0, 1):
            assert (np.diff(case.dist(metric, 20), axis=1) < 0).all()
            assert all(model_count(case, metric, 20, 1.0, 3, [q])[0] == R > 2048 for q in range(Q))
            mine = check(ctx, idx, qs, case, metric, 20, 1.0, 3)
            assert mine["col"].tolist() == [R - 3, R - 2, R - 1] * Q


# ---- g. shards x batches x look-up ------------------------------------------------------------------------------------------------------
SHARD = dict(row_step=3, row_block=4)     # 23 rows: blocks 0 .. 5, block 5 (rows 20 .. 22) is partial and belongs to shard 2
N_ROWS = 23
_legs = {}


def shard_case(leg):
    if leg not in _legs:
        if leg == "shuffled":     # clades in a shuffled caller order: the index renumbers them
            names, h, off = synth.clade_sketches(1000, 40, 24, strains_per_clade=10, seed=61)
            names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(1000, "shuffled", seed=3))
            refs = [np.unique(h[int(off[i]):int(off[i + 1])]) for i in range(1000)]
            rng = np.random.default_rng(62)
            queries = [np.unique(np.concatenate([refs[i] for i in rng.choice(1000, size=1 + q % 3, replace=False)])) for q in range(N_ROWS)]
            _legs[leg] = Case(refs, queries)
        else:
            wide = leg == "wide"
            bits = 36 if wide else 24
            rng, pool = np.random.default_rng(63 + wide), tr.Pool(bits, 63 + wide)
            R = 300
            sizes = rng.integers(100, 501, size=R)
            sizes[[0, 17]] = 0
            queries = [np.sort(pool.take(int(n))) for n in rng.integers(30, 201, size=N_ROWS)]
            queries[5] = queries[5][:0]
            common = np.zeros((N_ROWS, R), dtype=np.int64)
            for j in range(R):
                left = int(sizes[j])
                for q in rng.permutation(N_ROWS):
                    common[q, j] = 0 if rng.random() < 0.6 else min(int(rng.integers(1, 12)), left, len(queries[q]))
                    left -= common[q, j]
            dtype = np.uint64 if wide else np.uint32
            _legs[leg] = Case([r.astype(dtype) for r in tr.build_refs(pool, rng, queries, common, sizes)],
                              [q.astype(dtype) for q in queries], bits=bits, wide=wide)
            assert np.array_equal(_legs[leg].cell[0], common)
    return _legs[leg]


@pytest.mark.parametrize("leg", ["default", "sliced", "wide", "shuffled"])
def test_shards_with_a_partial_block_in_batches(monkeypatch, leg):
    case = shard_case("default" if leg == "sliced" else leg)
    R, N, k, D = len(case.refs), 5, 20, 1.0
    row_bytes = 4 * R + 144 * min(R, 1024 + 16 * N)     # a counter row and the candidate room of a row
    monkeypatch.setenv("RK_TOPN_CAND_CAP", "16")
    for rows_per_batch in (1, 3):     # 3: a batch boundary inside every block of 4
        monkeypatch.setenv("RK_TOPN_BATCH_BYTES", str(rows_per_batch * row_bytes + row_bytes // 2))
        c = capi.Context(0)     # (the knobs are read when a context is made)
        c.set_timing(True)
        idx, qs = case.upload(c)
        if leg == "shuffled":
            assert not np.array_equal(idx.order, np.arange(R))
        if leg == "sliced":
            plain_name = c.dist_kernel_name(idx, qs, 0, 0, k, D)
            monkeypatch.setenv("RK_DISTQ_SLICED", "1")
            assert c.dist_kernel_name(idx, qs, 0, 0, k, D) != plain_name     # the pre-resolved look-up is what runs
        for metric in (0, 1):
            whole = check(c, idx, qs, case, metric, k, D, N)
            assert len(whole) == N_ROWS * N
            parts = [check(c, idx, qs, case, metric, k, D, N, row_first=r, **SHARD) for r in range(3)]
            assert [len(p) // N for p in parts] == [8, 8, 7] and parts[2]["row"][-1] == 22
            merged = np.concatenate(parts)
            assert merged[np.argsort(merged["row"], kind="stable")].tobytes() == whole.tobytes()
            assert len(check(c, idx, qs, case, metric, k, D, N, row_first=7, row_step=9, row_block=4)) == 0     # a shard without rows
        monkeypatch.delenv("RK_DISTQ_SLICED", raising=False)
        c.close()
