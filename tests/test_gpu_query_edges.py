"""rk_distq_kernel (rabbitkssd_amd/csrc/rk_distq.hip) at its tile, counter and look-up edges, against CPU references:
ok.index_dist32 for hash spaces up to 28 bits, ok.index_dist64 for 64-bit hashes, tests/_query_ref.py (the oracle's sparse
path, held equal to a numpy model) for 32-bit hashes.  Integers and jorc bit for bit; dist bit for bit through
rk_dist_rows, within 1e-12 through rk_dist_rows_dev.  Every case asserts the kernel variant it reached and, from the
reference, the property it was built for; sizes make that property hold by arithmetic (the whole LDS is 160 KiB), not by
the planner's constants."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle as ok
from rabbitkssd_amd import capi

import _gpu_join as gj
import _query_ref as qr
from _gpu_join import REC, check_dev
from _rows_ref import min_common      # (the row-level reject is the same expression in rk_distq_kernel and rk_dist_kernel)

pytestmark = pytest.mark.gpu
K = 20
LDS_BYTES = 160 * 1024     # all the LDS of a CU: a counter row above it cannot be one tile
CORES = min(16, os.cpu_count() or 1)


def make_ctx(relabel):
    old = os.environ.get("RK_INDEX_RELABEL")
    if relabel:
        os.environ.pop("RK_INDEX_RELABEL", None)
    else:
        os.environ["RK_INDEX_RELABEL"] = "0"     # (read when the context is created)
    try:
        return capi.Context(0)
    finally:
        if old is None:
            os.environ.pop("RK_INDEX_RELABEL", None)
        else:
            os.environ["RK_INDEX_RELABEL"] = old


@pytest.fixture(scope="module")
def ctxs():
    c = {"identity": make_ctx(False), "shipped": make_ctx(True)}
    yield c
    for x in c.values():
        x.close()


def upload(ctx, h, off):
    return ctx.sketches_from_host64(h, off) if h.dtype == np.uint64 else ctx.sketches_from_host(h, off)


def dev_records(ctx, idx, qs, triangle, metric, D, cap, **shard):
    return gj.dev_records(ctx, idx, qs, triangle, metric, D, K, cap, **shard)


def check_both(ctx, idx, qs, want, triangle, metric, D, wdense=None, **shard):
    """the synchronous API (bit for bit, with the dense counter matrix where a reference is given) and the device-resident one"""
    mine, dense = ctx.dist_rows(idx, qs, triangle, metric, K, D, want_dense=wdense is not None, **shard)
    qr.assert_same_hits(mine, want, "rk_dist_rows metric=%d D=%g" % (metric, D))
    if wdense is not None:
        assert np.array_equal(dense, wdense)
        mine, _ = ctx.dist_rows(idx, qs, triangle, metric, K, D, **shard)     # (without the matrix: the clean-kept row)
        qr.assert_same_hits(mine, want, "rk_dist_rows, no matrix, metric=%d D=%g" % (metric, D))
    n, dev = dev_records(ctx, idx, qs, triangle, metric, D, len(want) + 1024, **shard)
    assert n == len(want)
    check_dev(dev, want)


def reference(rh, roff, bits, qh, qoff, triangle, metric, D, want_dense=False):
    if rh.dtype == np.uint64:
        uhash, ucount, postings = ok.index_build64(rh, roff)
        return ok.index_dist64(uhash, ucount, postings, np.diff(roff).astype(np.uint32), qh, qoff, triangle, metric, K, D,
                               threads=CORES, want_dense=want_dense)
    if bits > 28:
        return qr.ref_wide(rh, roff, qh, qoff, triangle, metric, K, D, want_dense=want_dense, threads=CORES)
    postings, counts = ok.index_build32(rh, roff, bits)
    return ok.index_dist32(counts, bits, postings, np.diff(roff).astype(np.uint32), qh, qoff, triangle, metric, K, D,
                           threads=CORES, want_dense=want_dense)


def clades(rng, n_clades, strains, m, space, keep):
    """(ancestors [n_clades, m], strains [n_clades * strains, m]): strain 0 is the ancestor, the others keep a hash with
    probability `keep`"""
    anc = rng.integers(0, space, size=(n_clades, m), dtype=np.uint64)
    mat = np.repeat(anc, strains, axis=0)
    mut = rng.random(mat.shape) >= keep
    mut[::strains] = False
    return anc, np.where(mut, rng.integers(0, space, size=mat.shape, dtype=np.uint64), mat)


def relatives(rng, anc, space, keep, extra):
    """one query per row of `anc`: its hashes kept with probability `keep`, plus `extra` fresh ones"""
    mut = rng.random(anc.shape) >= keep
    q = np.where(mut, rng.integers(0, space, size=anc.shape, dtype=np.uint64), anc)
    return np.concatenate([q, rng.integers(0, space, size=(len(anc), extra), dtype=np.uint64)], axis=1)


def csr_parts(h, off):
    return [h[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


# ---- 1. tiled counter rows ---------------------------------------------------------------------------------------------
LEAD = 3     # references ahead of the first clade: clade c holds columns 3 + 10 c .. 12 + 10 c, so no multiple of 128 falls between two clades
TILE_LEGS = {
    # width: (clades, hash bits, kernel)            n_ref * cbits / 8 > 160 KiB: more than one tile however the plan splits
    "8": (17000, 24, "rk_distq_kernel<8, 0, true>"),      # 170,003 B
    "16": (8400, 24, "rk_distq_kernel<16, 0, true>"),     # 168,006 B
    "32": (4200, 24, "rk_distq_kernel<32, 0, false>"),    # 168,012 B; no list records (a reference repeats a hash): the plain look-up
    "32s": (4200, 24, "rk_distq_kernel<32, 0, true>"),    # 168,012 B; set references, 32 bits for a sketch of 65,536 hashes
    "64": (4200, 36, "rk_distq_kernel<32, 2, false>"),    # 168,012 B, 36-bit hashes: directory + binary search on u64
}


@functools.lru_cache(maxsize=1)
def tile_data(width):
    n_clades, bits, _ = TILE_LEGS[width]
    cbits = 32 if width in ("64", "32s") else int(width)
    dtype = np.uint64 if width == "64" else np.uint32
    rng = np.random.default_rng(900 + cbits + bits + (3 if width == "32s" else 0))
    space = 1 << bits
    anc, strains = clades(rng, n_clades, 10, 12, space, 0.92)
    rh, roff = qr.rows_to_csr(strains, dtype)
    lead = [np.unique(rng.integers(0, space, size=12, dtype=np.uint64)).astype(dtype) for _ in range(LEAD)]
    qh, qoff = qr.rows_to_csr(relatives(rng, anc, space, 0.95, 3), dtype)
    extra_q = [np.unique(rng.integers(0, space, size=15, dtype=np.uint64)).astype(dtype) for _ in range(50)]   # unrelated
    extra_q.append(np.zeros(0, dtype=dtype))
    if width == "16":
        # one reference and one query of 300 hashes: an intersection can reach 300, which needs 16 bits
        lead[1] = np.unique(rng.integers(0, space, size=300, dtype=np.uint64)).astype(dtype)[:300]
        extra_q.append(lead[1].copy())
    if width == "32s":
        # one reference and one query of 65,536 hashes: sets on both sides, yet an intersection can need 17 bits
        lead[1] = np.unique(rng.integers(0, space, size=80000, dtype=np.uint64)).astype(dtype)[:65536]
        extra_q.append(lead[1].copy())
    if width in ("32", "64"):
        # a reference that lists a hash twice: the references are no sets, no bound holds, 32-bit counters
        lead[1] = np.sort(np.concatenate([lead[1], lead[1][:2]]))
        extra_q.append(np.unique(lead[1]))
    r_parts = lead + csr_parts(rh, roff)
    q_parts = csr_parts(qh, qoff) + extra_q
    rh, roff = qr.csr(r_parts, dtype)
    qh, qoff = qr.csr(q_parts, dtype)
    n_ref = len(roff) - 1
    assert n_ref * cbits // 8 > LDS_BYTES                    # more than one tile, by arithmetic
    return dict(bits=bits, cbits=cbits, rh=rh, roff=roff, qh=qh, qoff=qoff, n_ref=n_ref, n_clades=n_clades, want={})


def tile_want(d, metric, D):
    if (metric, D) not in d["want"]:
        d["want"][(metric, D)] = reference(d["rh"], d["roff"], d["bits"], d["qh"], d["qoff"], 0, metric, D)[0]
    return d["want"][(metric, D)]


def boundary_columns(n_ref):
    """first column of every tile but the first, for a split into 2, 3 or 4 equal tiles of whole 128-column groups"""
    out = set()
    for nt in (2, 3, 4):
        tile = ((n_ref + nt - 1) // nt + 127) & ~127
        out.update(j * tile for j in range(1, nt) if j * tile < n_ref)
    return sorted(out)


@pytest.mark.parametrize("leg", ["identity", "shipped"])
@pytest.mark.parametrize("width", ["8", "16", "32", "32s", "64"])
def test_tiled_counter_rows(ctxs, width, leg):
    """More references than one LDS row holds at this counter width (n_tiles > 1), clades of 10 with one related query each:
    the c < ncol range test, compact lists and the wave's 32-column window across col0 / col1, the shorter last tile, the
    padded unit order; hit records of every query for both metrics, dense mode (D = 1.5) and the dense counter matrix for the
    queries whose relatives sit on the possible tile boundaries; a block-cyclic shard union.
    Asserted from the reference: hits in the last column and in columns 128 k - 1 and 128 k for every k."""
    d = tile_data(width)
    ctx = ctxs[leg]
    n_ref, bits = d["n_ref"], d["bits"]
    idx = ctx.index_build(upload(ctx, d["rh"], d["roff"]), bits)
    qs = upload(ctx, d["qh"], d["qoff"])
    assert ctx.dist_kernel_name(idx, qs, 0, 0, K, 0.1) == TILE_LEGS[width][2]
    order = idx.order                       # order[i]: the caller's id of internal column i
    if leg == "identity" or width in ("32", "64"):      # (a collection that is no set keeps the caller's order too)
        assert np.array_equal(order, np.arange(n_ref))
    inv = np.empty(n_ref, dtype=np.int64)
    inv[order] = np.arange(n_ref)
    ks = np.arange(1, (n_ref - 1) // 128 + 1)
    for metric in (0, 1):
        want = tile_want(d, metric, 0.1)
        has = np.zeros(n_ref, dtype=bool)
        has[inv[want["col"]]] = True        # columns as the kernel numbers them
        assert has[n_ref - 1] and has[ks * 128 - 1].all() and has[ks * 128].all()
        assert len(want) > 9 * d["n_clades"]
        check_both(ctx, idx, qs, want, 0, metric, 0.1)
    # a block-cyclic shard of the query rows: the union is the whole
    want = tile_want(d, 0, 0.1)
    parts = [ctx.dist_rows(idx, qs, 0, 0, K, 0.1, row_first=r, row_step=3, row_block=16)[0] for r in range(3)]
    for r, p in enumerate(parts):
        assert len(p) and np.all((p["row"] // 16) % 3 == r)
    merged = np.concatenate(parts)
    qr.assert_same_hits(merged[np.lexsort((merged["col"], merged["row"]))], want, "shard union")
    # dense mode and the counter matrix: the queries related to the clades on every possible tile boundary, the first and the
    # last column, an unrelated query and the queries added for this width
    cols = [0, n_ref - 1] + [c + o for c in boundary_columns(n_ref) for o in (-1, 0)]
    sel = sorted({int((order[c] - LEAD) // 10) for c in cols if order[c] >= LEAD} | {d["n_clades"], len(d["qoff"]) - 2})
    q_parts = csr_parts(d["qh"], d["qoff"])
    sh, soff = qr.csr([q_parts[q] for q in sel], d["qh"].dtype)
    sqs = upload(ctx, sh, soff)
    for metric, D in ((0, 1.5), (1, 1.5), (1, 0.1)):
        want, wdense = reference(d["rh"], d["roff"], bits, sh, soff, 0, metric, D, want_dense=True)
        assert D < 1 or len(want) == len(sel) * n_ref
        assert wdense[:, [order[c] for c in cols if order[c] >= LEAD]].max(axis=0).min() > 0     # every boundary column is counted into
        check_both(ctx, idx, sqs, want, 0, metric, D, wdense=wdense)
    if width == "16":
        assert wdense.max() >= 256
    if width == "32s":
        assert wdense.max() == 65536
    if width in ("32", "64"):
        assert wdense[-1, 1] == len(q_parts[-1]) + 2       # the reference's repeats are counted


@pytest.mark.parametrize("leg", ["identity", "shipped"])
def test_tiled_counter_rows_triangle(ctxs, leg):
    """The alldist form with explicit queries over a tiled row (16-bit leg): the triangle skips `col1 <= row + 1` and `jbeg`
    inside a tile, on the caller's ids where the index is renumbered.  Sparse: every row against ok.index_dist32.  Dense mode
    (D = 1.5, where a wrong `jbeg` reports cells left of the diagonal): a block-cyclic shard of 2-row blocks spread over the
    whole collection against the numpy model, which the same rows of the sparse reference hold to the oracle."""
    d = tile_data("16")
    ctx = ctxs[leg]
    n_ref, bits = d["n_ref"], d["bits"]
    rsk = upload(ctx, d["rh"], d["roff"])
    idx = ctx.index_build(rsk, bits)
    assert ctx.dist_kernel_name(idx, rsk, 1, 0, K, 0.1) == "rk_distq_kernel<16, 0, true>"
    assert n_ref * 2 > LDS_BYTES
    shard = dict(row_first=1, row_step=4000, row_block=2)
    rows = [r for r in range(n_ref) if (r // 2) % 4000 == 1]
    assert rows[0] == 2 and rows[-1] > n_ref - 8000 and len(rows) >= 20
    for metric in (0, 1):
        want = reference(d["rh"], d["roff"], bits, d["rh"], d["roff"], 1, metric, 0.1)[0]
        assert len(want) > 30 * d["n_clades"] and np.all(want["col"] > want["row"])
        check_both(ctx, idx, rsk, want, 1, metric, 0.1)
        part, _ = qr.numpy_model(d["rh"], d["roff"], d["rh"], d["roff"], 1, metric, K, 0.1, rows=rows)
        qr.assert_same_hits(part, want[np.isin(want["row"], rows)], "numpy model on the shard's rows")
        check_both(ctx, idx, rsk, part, 1, metric, 0.1, **shard)
        full, _ = qr.numpy_model(d["rh"], d["roff"], d["rh"], d["roff"], 1, metric, K, 1.5, rows=rows)
        assert len(full) == sum(n_ref - 1 - r for r in rows)
        check_both(ctx, idx, rsk, full, 1, metric, 1.5, **shard)


def test_tiled_counter_rows_without_the_pipelined_lookup(ctxs, monkeypatch):
    """the 8-bit leg once more through the unpipelined rank-bitmap look-up (RK_DISTQ_PIPE=0)"""
    d = tile_data("8")
    ctx = ctxs["identity"]
    idx = ctx.index_build(upload(ctx, d["rh"], d["roff"]), d["bits"])
    qs = upload(ctx, d["qh"], d["qoff"])
    monkeypatch.setenv("RK_DISTQ_PIPE", "0")
    assert ctx.dist_kernel_name(idx, qs, 0, 0, K, 0.1) == "rk_distq_kernel<8, 0, false>"
    check_both(ctx, idx, qs, tile_want(d, 0, 0.1), 0, 0, 0.1)


# ---- 2. the prefix directory + binary search on 32-bit hashes ----------------------------------------------------------
def dir32_data():
    rng = np.random.default_rng(3232)
    space = 1 << 32
    anc, strains = clades(rng, 300, 10, 60, space, 0.9)
    strains[0, 0], strains[1, 0], strains[2, :2] = 0, 0xFFFFFFFF, (0, 0xFFFFFFFF)     # both ends of the hash space
    strains[3, :4] = (1, 2, 0xFFFFFFFE, 0x80000000)
    rh, roff = qr.rows_to_csr(strains)
    r_parts = csr_parts(rh, roff)
    q = csr_parts(*qr.rows_to_csr(relatives(rng, anc, space, 0.9, 8)))
    for r in (0, 1, 2, 3, 17, 1500, 2999):
        own = r_parts[r].astype(np.int64)
        near = np.concatenate([own[::2], own[1::3] - 1, own[2::3] + 1])      # hashes just below and just above indexed ones
        q.append(np.unique(near[(near >= 0) & (near < space)]).astype(np.uint32))
    q += [np.unique(rng.integers(0, space, size=s, dtype=np.uint64)).astype(np.uint32) for s in (70, 500, 3)]   # absent
    q += [np.zeros(0, dtype=np.uint32)]
    q += [np.array([v], dtype=np.uint32) for v in (0, 0xFFFFFFFF, 1, 0xFFFFFFFD, int(r_parts[9][5]), int(r_parts[9][5]) + 1)]
    q += [np.array([0, 0xFFFFFFFF], dtype=np.uint32), np.zeros(0, dtype=np.uint32)]
    qh, qoff = qr.csr(q)
    return rh, roff, qh, qoff


@pytest.mark.parametrize("leg", ["identity", "shipped"])
def test_lookup_by_directory_and_binary_search_32bit(ctxs, leg):
    """hash_bits = 32 (K12 L4, K11 L3): above the rank bitmap's 30 bits, so the look-up is kLookDir32.  3,000 references with
    hashes over the whole 32-bit range, 0 and 0xFFFFFFFF among them; queries with relatives, with hashes one below and one
    above indexed ones, absent hashes, empty and one-hash queries."""
    rh, roff, qh, qoff = dir32_data()
    assert rh.min() == 0 and rh.max() == 0xFFFFFFFF and np.all(np.diff(np.histogram(rh, bins=16, range=(0, 1 << 32))[0]) < len(rh) // 64)
    ctx = ctxs[leg]
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), 32)
    qs = ctx.sketches_from_host(qh, qoff)
    name = ctx.dist_kernel_name(idx, qs, 0, 0, K, 0.1)
    assert name == "rk_distq_kernel<8, 1, false>" and name.split(", ")[1] == "1"
    nq = len(qoff) - 1
    for metric, D in ((0, 0.1), (1, 0.1), (0, 1.5), (1, 1.5)):
        want, wdense = reference(rh, roff, 32, qh, qoff, 0, metric, D, want_dense=True)
        assert len(want) >= (nq * 3000 if D > 1 else 2500)
        check_both(ctx, idx, qs, want, 0, metric, D, wdense=wdense)
    one = wdense[nq - 8: nq - 2]      # the one-hash queries: 0, 0xFFFFFFFF, 1, 0xFFFFFFFD, an indexed hash, its successor
    assert one[0, 0] == 1 and one[0, 2] == 1 and one[1, 1] == 1 and one[1, 2] == 1 and one[2, 3] == 1 and one[4, 9] == 1
    assert one[3].sum() == 0 and one.sum(axis=1).tolist()[:3] == [2, 2, 1]
    assert wdense[nq - 2, 2] == 2 and wdense[nq - 1].sum() == 0 and wdense[nq - 9].sum() == 0


# ---- 3. counter saturation and the width boundaries --------------------------------------------------------------------
def sat_data(size):
    """a family of 12 references around one set S of `size` hashes (8 of them S itself, in columns 0, 2, 4..7 and the rest
    close variants no larger than S) and 20 small clades; queries: S, S without its last hash, a variant, unrelated, empty"""
    rng = np.random.default_rng(size)
    bits, space = 24, 1 << 24
    S = np.unique(rng.integers(0, space, size=size + size // 4 + 8, dtype=np.uint64))
    rng.shuffle(S)
    S = np.sort(S[:size]).astype(np.uint32)

    def variant(drop):
        keep = S[rng.random(size) >= drop]
        fresh = rng.integers(0, space, size=max(1, (size - len(keep)) // 2), dtype=np.uint64).astype(np.uint32)
        return np.unique(np.concatenate([keep, fresh]))[:size]
    fam = [S, variant(0.1), S, variant(0.2), S, S, S, S, variant(0.05), variant(0.3), variant(0.1), variant(0.5)]
    anc, strains = clades(rng, 20, 10, 40, space, 0.9)
    rh, roff = qr.csr(fam + csr_parts(*qr.rows_to_csr(strains)))
    q = [S, S[:-1], fam[3], np.unique(rng.integers(0, space, size=size // 2, dtype=np.uint64)).astype(np.uint32),
         np.zeros(0, dtype=np.uint32)] + csr_parts(*qr.rows_to_csr(relatives(rng, anc, space, 0.9, 5)))
    qh, qoff = qr.csr(q)
    return bits, rh, roff, qh, qoff


@pytest.mark.parametrize("leg", ["identity", "shipped"])
@pytest.mark.parametrize("size,cbits", [(255, 8), (256, 16), (65535, 16), (65536, 32)])
def test_counter_saturation_at_the_width_boundaries(ctxs, size, cbits, leg):
    """The largest sketch on both sides is 255 / 256 / 65,535 / 65,536 hashes: the bound sits on either side of a counter
    width, and a query that equals a reference drives cells to the bound -- at 255 and 65,535 to the cell's maximum -- while
    the other cells of the same LDS word hold counts of their own (the four columns 0..3 in identity order).  All lists of S
    are compact and share one 32-column window, so the wave counts them 64 at a time (bump_n adds n = 64)."""
    bits, rh, roff, qh, qoff = sat_data(size)
    assert np.diff(roff).max() == size and np.diff(qoff).max() == size
    ctx = ctxs[leg]
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), bits)
    qs = ctx.sketches_from_host(qh, qoff)
    assert ctx.dist_kernel_name(idx, qs, 0, 0, K, 0.1) == "rk_distq_kernel<%d, 0, false>" % cbits
    for metric, D in ((0, 0.1), (1, 0.1), (0, 1.5)):
        want, wdense = reference(rh, roff, bits, qh, qoff, 0, metric, D, want_dense=True)
        assert len(want) > 0
        word = wdense[0, :4]      # one LDS word of 8-bit cells, two of 16-bit ones
        assert word[0] == size and word[2] == size and 0 < word[1] < size and 0 < word[3] < size
        assert np.all(wdense[0, 4:8] == size) and np.all(wdense[1, 4:8] == size - 1)
        if size in (255, 65535):
            assert word[0] == (1 << cbits) - 1     # the cell's maximum
        check_both(ctx, idx, qs, want, 0, metric, D, wdense=wdense)


def repeats_data():
    rng = np.random.default_rng(77)
    bits, space = 22, 1 << 22
    A = np.unique(rng.integers(0, space, size=120, dtype=np.uint64)).astype(np.uint32)[:85]
    B = np.unique(rng.integers(0, space, size=100, dtype=np.uint64)).astype(np.uint32)[:64]
    anc, strains = clades(rng, 30, 10, 60, space, 0.9)
    r_parts = [A, A[:-5], A[:-10], A[20:], B, B[:-3], B[5:], B] + csr_parts(*qr.rows_to_csr(strains))
    rel = csr_parts(*qr.rows_to_csr(relatives(rng, anc, space, 0.9, 5)))
    return bits, r_parts, A, B, rel


@pytest.mark.parametrize("leg", ["identity", "shipped"])
@pytest.mark.parametrize("case,name", [("q255", "rk_distq_kernel<8, 0, false>"), ("q256", "rk_distq_kernel<16, 0, false>"),
                                       ("refs", "rk_distq_kernel<32, 0, false>")])
def test_repeated_hashes_pick_the_counter_width(ctxs, case, name, leg):
    """A query that repeats hashes against set references is bounded by its own length only (bound = qs->max_size): 85 hashes
    three times (255 -> 8 bits, the cell of that reference reaches 255) and 64 hashes four times (256 -> 16 bits).  References
    that repeat a hash bound nothing: 32 bits."""
    bits, r_parts, A, B, rel = repeats_data()
    if case == "q255":
        q_parts, cell = [np.sort(np.tile(A, 3))] + rel, (0, 255)
    elif case == "q256":
        q_parts, cell = [np.sort(np.tile(B, 4))] + rel, (4, 256)
    else:
        r_parts = r_parts[:2] + [np.sort(np.concatenate([A[:-10], A[:7]]))] + r_parts[3:]
        q_parts, cell = [A] + rel, (2, 75 + 7)
    rh, roff = qr.csr(r_parts)
    qh, qoff = qr.csr(q_parts)
    ctx = ctxs[leg]
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), bits)
    qs = ctx.sketches_from_host(qh, qoff)
    assert ctx.dist_kernel_name(idx, qs, 0, 0, K, 0.1) == name
    for metric, D in ((0, 0.1), (1, 0.1), (1, 1.5)):
        want, wdense = reference(rh, roff, bits, qh, qoff, 0, metric, D, want_dense=True)
        w0 = cell[0] // 4 * 4      # the cell's LDS word (8-bit cells) or pair of words: every cell of it counts something
        assert wdense[0, cell[0]] == cell[1] and np.all(wdense[0, w0:w0 + 4] > 0) and len(want) > 0
        check_both(ctx, idx, qs, want, 0, metric, D, wdense=wdense)


# ---- 4. the sparse epilogue's overflow paths ---------------------------------------------------------------------------
FAMILIES = (257, 258, 259, 260, 300, 700)      # references per family: just above the 256-cell list, and well above it
N_EPI_QUERIES = 6400


@functools.lru_cache(maxsize=1)
def epilogue_data():
    """~4,000 references of 40 hashes: six families whose members all hold their family's 30-hash core (a query that is the
    core is reportable against every member) and clades of 10; 6,400 queries: a quarter heavy (a core), half light (a clade's
    relative or unrelated), a quarter empty, in random order; also returns the heavy queries' numbers"""
    rng = np.random.default_rng(4242)
    bits, space = 24, 1 << 24
    r_parts, cores = [np.unique(rng.integers(0, space, size=40, dtype=np.uint64)).astype(np.uint32) for _ in range(5)], []   # (families start off a quad boundary)
    for n in FAMILIES:
        core = rng.integers(0, space, size=30, dtype=np.uint64)
        cores.append(np.unique(core).astype(np.uint32))
        own = rng.integers(0, space, size=(n, 10), dtype=np.uint64)
        r_parts += csr_parts(*qr.rows_to_csr(np.concatenate([np.tile(core, (n, 1)), own], axis=1)))
    anc, strains = clades(rng, 220, 10, 40, space, 0.9)
    r_parts += csr_parts(*qr.rows_to_csr(strains))
    light = csr_parts(*qr.rows_to_csr(relatives(rng, anc, space, 0.9, 4)))
    # the kinds in random order: a workgroup's units lie a whole grid apart, so a pattern whose period divides the grid would
    # hand every workgroup one kind only
    kinds = rng.integers(0, 4, size=N_EPI_QUERIES)
    q_parts, n_heavy = [], 0
    for i in range(N_EPI_QUERIES):
        if kinds[i] == 0:
            q_parts.append(cores[n_heavy % len(cores)])
            n_heavy += 1
        elif kinds[i] == 3:
            q_parts.append(np.zeros(0, dtype=np.uint32))
        else:
            q_parts.append(light[(i * 7) % len(light)] if kinds[i] == 1 else np.unique(rng.integers(0, space, size=30, dtype=np.uint64)).astype(np.uint32))
    rh, roff = qr.csr(r_parts)
    qh, qoff = qr.csr(q_parts)
    return bits, rh, roff, qh, qoff, np.flatnonzero(kinds == 0)


@pytest.mark.parametrize("leg", ["identity", "shipped"])
def test_sparse_epilogue_overflows_its_list_and_its_stage(ctxs, leg):
    """More than 256 candidate cells in a unit (families of 257..260 references leave a quad that fits the list partly or not
    at all: the 0xFFFFFFFF marker, the leftover walk, the re-zeroing of a clean-kept row), more hits than every workgroup of
    the largest possible grid can stage (96 each), and 6,400 units -- heavy, light and empty interleaved -- so that workgroups
    take several in turn on one row.  Also with the dense counter matrix (the row zeroed per unit, the whole-row walk)."""
    bits, rh, roff, qh, qoff, heavy = epilogue_data()
    ctx = ctxs[leg]
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), bits)
    qs = ctx.sketches_from_host(qh, qoff)
    assert ctx.dist_kernel_name(idx, qs, 0, 0, K, 0.1) == "rk_distq_kernel<8, 0, false>"
    n_ref, nq = len(roff) - 1, len(qoff) - 1
    assert 3000 <= n_ref < 8000 and nq >= 6000
    # the largest grid: the LDS of a CU over the smallest footprint of a workgroup (the 256-thread one's queues, list and
    # stage: 4 x 1,024 + 2,048 + 4,608 + 64 bytes, no counter row at all) on every CU
    max_grid = torch.cuda.get_device_properties(0).multi_processor_count * (LDS_BYTES // (4 * 1024 + 256 * 8 + 96 * REC + 64))
    sizes, qsizes = np.diff(roff).astype(np.int64), np.diff(qoff).astype(np.int64)
    for metric in (0, 1):
        want, wdense = reference(rh, roff, bits, qh, qoff, 0, metric, 0.1, want_dense=True)
        cand = np.array([(wdense[q] >= min_common(metric, 0.1, int(qsizes[q]), int(sizes.min()))).sum() if qsizes[q] else 0 for q in range(nq)])
        assert cand[heavy[:6]].tolist() == list(FAMILIES) and np.all(cand[heavy] > 256) and len(heavy) >= nq // 5
        assert len(want) > 96 * max_grid, (len(want), max_grid)
        check_both(ctx, idx, qs, want, 0, metric, 0.1)
    # the matrix of the last metric, for a slice of the queries (heavy, light and empty ones)
    sub = slice(0, 400)
    sh, soff = qh[: int(qoff[400])], qoff[:401]
    want, wd = reference(rh, roff, bits, sh, soff, 0, 1, 0.1, want_dense=True)
    assert np.array_equal(wd, wdense[sub])
    check_both(ctx, idx, ctx.sketches_from_host(sh, soff), want, 0, 1, 0.1, wdense=wd)


# ---- 5. rk_dist_rows_dev over its capacity -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [0.1, 1.5])
def test_device_hits_over_capacity(ctxs, D):
    """hits_cap at a third of the true count (sparse: staged and directly written records; dense mode: reserved slots):
    *n_hits_dev still counts every hit, the `cap` records written are distinct members of the result, and the bytes behind
    the buffer keep their pattern."""
    bits, rh, roff, qh, qoff, _ = epilogue_data()
    nq = len(qoff) - 1 if D < 1 else 96
    qh, qoff = qh[: int(qoff[nq])], qoff[: nq + 1]
    ctx = ctxs["shipped"]
    idx = ctx.index_build(ctx.sketches_from_host(rh, roff), bits)
    qs = ctx.sketches_from_host(qh, qoff)
    assert ctx.dist_kernel_name(idx, qs, 0, 0, K, D) == "rk_distq_kernel<8, 0, false>"
    n_ref = len(roff) - 1
    for metric in (0, 1):
        want = reference(rh, roff, bits, qh, qoff, 0, metric, D)[0]
        assert len(want) > 100000 and (D < 1 or len(want) == nq * n_ref)
        cap = len(want) // 3
        n, got = dev_records(ctx, idx, qs, 0, metric, D, cap)       # (asserts the guard)
        gj.assert_capped_records(n, got, want, cap, n_ref)
