"""Generators and a plain model for the pruning bounds of the self join (tests/test_prune_ref_cpu.py, tests/test_gpu_prune_edges.py).

Every kernel of the self join skips what "cannot hold a reportable pair": common >= min_jorc * (a lower bound of the
denominator).  The model restates the four places that rule lives in with numpy and Python integers -- the launch prefix
of the tile directory (`launch_grid`), the tile kernel's own test (`tiles`: records and lb per tile), the row bound of
rk_near_kernel and rk_dist_kernel (`floor_common`) and the far records of a unit of rk_near_kernel (`far_records`,
`falls_back`) -- and the generators build collections whose pairs sit ON those bounds.  Hashes are disjoint by
construction (a counter times an odd constant modulo 2^bits), so two sketches share exactly what the generator gave them.
What is reportable is never a formula here: `first_reportable` asks the oracle's distance."""
import functools
import math

import numpy as np

from oracle import oracle as ok

K = 20
BITS = 26
_ODD = 0x9E3779B1


class Hashes:
    """n fresh hashes at a time, never one twice: i -> i * odd mod 2^bits is a bijection"""

    def __init__(self, bits=BITS):
        self.bits, self.next = bits, 1

    def take(self, n):
        assert self.next + n <= 1 << self.bits
        a = (np.arange(self.next, self.next + n, dtype=np.uint64) * np.uint64(_ODD)) & np.uint64((1 << self.bits) - 1)
        self.next += n
        return a.astype(np.uint32)


def csr(parts):
    """(hashes, off) with every genome's hashes ascending"""
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    h = np.concatenate([np.sort(np.asarray(p, dtype=np.uint32)) for p in parts]) if parts else np.zeros(0, dtype=np.uint32)
    return np.ascontiguousarray(h), off


# ---- the model -----------------------------------------------------------------------------------------------------------
def min_jorc(metric, D):
    """rk_min_jorc (rk_dist_plan.h)"""
    t = math.exp(-float(K) * D)
    return (t if metric else t / (2.0 - t)) * (1.0 - 1e-6)


def floor_common(metric, D, qsize, min_ref_size):
    """the row bound of rk_near_kernel and rk_dist_kernel: cells below it are never evaluated"""
    lb = min(qsize, min_ref_size) if metric else qsize
    return max(1, int(math.floor(min_jorc(metric, D) * lb)))


@functools.lru_cache(maxsize=None)
def first_reportable(metric, D, size0, size1_rule):
    """the smallest `common` the oracle's distance reports under D (dist < D, src/dist.cpp:232) for a row of size0 and a column
    whose size is size1_rule -- an integer, or "subset": the column IS the shared part (size1 = common).  None: none."""
    for c in range(1, size0 + 1):
        size1 = c if size1_rule == "subset" else int(size1_rule)
        if c > size1:
            return None
        if ok.distance(c, size0, size1, metric, K)[1] < D:
            return c
    return None


def launch_kk(metric, D):
    """the level tile_launch_shape looks up for a threshold"""
    return int(math.ceil(-8.0 * math.log2(min_jorc(metric, D))))


_MEMO = {}


def _lists(h, off):
    """(the distinct hashes ascending, the starts of their member lists, the members, every list's largest member), memoised per array"""
    key = (h.ctypes.data, len(h), len(off))
    if key not in _MEMO:
        sizes = np.diff(off).astype(np.int64)
        gid = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
        order = np.lexsort((gid, h))
        ph, pg = h[order], gid[order]
        starts = np.flatnonzero(np.r_[True, ph[1:] != ph[:-1]]) if len(ph) else np.zeros(0, dtype=np.int64)
        ends = np.r_[starts, len(ph)].astype(np.int64)
        _MEMO[key] = (h, ph[starts] if len(ph) else ph, ends, pg, pg[ends[1:] - 1])   # (h: the key's address stays this array's)
    return _MEMO[key][1:]


def tiles(h, off):
    """identity order: for every pair of 32-id blocks (b <= w) that some posting list touches, the number of lists with a
    member in b and one in w (b == w: at least two members in b); the blocks' smallest NON-EMPTY sketches; lb per tile for
    jaccard (the larger of the two minima) and containment (the smaller).  Tiles ascend by (b, w)."""
    sizes = np.diff(off).astype(np.int64)
    n = len(sizes)
    nb = (n + 31) // 32
    blk_min = np.full(nb, 0xFFFFFFFF, dtype=np.int64)
    for b in range(nb):
        s = sizes[b * 32:(b + 1) * 32]
        if np.any(s > 0):
            blk_min[b] = s[s > 0].min()
    _, starts, pg, _ = _lists(h, off)
    rec = {}
    for a in np.flatnonzero(np.diff(starts) >= 2):
        blocks, cnt = np.unique(pg[starts[a]:starts[a + 1]] >> 5, return_counts=True)
        for i, b in enumerate(blocks):
            if cnt[i] >= 2:
                rec[(int(b), int(b))] = rec.get((int(b), int(b)), 0) + 1
            for w in blocks[i + 1:]:
                rec[(int(b), int(w))] = rec.get((int(b), int(w)), 0) + 1
    keys = sorted(rec)
    kb = np.array([k[0] for k in keys], dtype=np.int64)
    kw = np.array([k[1] for k in keys], dtype=np.int64)
    return dict(keys=keys, records=np.array([rec[k] for k in keys], dtype=np.int64), blk_min=blk_min,
                lb=(np.maximum(blk_min[kb], blk_min[kw]), np.minimum(blk_min[kb], blk_min[kw])))


def thresholds():
    """theta(k) of the tile directory's 256 levels, in float32 as the device has them: 2^(-k/8) less a margin of 1e-4"""
    return np.exp2(-np.arange(256, dtype=np.float32) / np.float32(8)).astype(np.float32) * (np.float32(1) - np.float32(1e-4))


def tile_ratios(t, metric):
    return t["records"].astype(np.float32) / t["lb"][1 if metric else 0].astype(np.float32)


def tile_levels(t, metric):
    """smallest k with ratio >= theta(k) per tile (256: none)"""
    ge = tile_ratios(t, metric)[:, None] >= thresholds()[None, :]
    return np.where(ge.any(axis=1), ge.argmax(axis=1), 256)


def launch_grid(t, metric, D):
    """(workgroups the tile launch starts, smallest relative distance of any tile's ratio from any of the 256 thresholds)"""
    ratio, theta = tile_ratios(t, metric), thresholds()
    rel = float(np.min(np.abs(ratio.astype(np.float64)[:, None] - theta.astype(np.float64)[None, :]) / theta.astype(np.float64)[None, :])) if len(ratio) else 1.0
    mj = min_jorc(metric, D)
    if mj <= 0.0:
        return len(ratio), rel
    kk = launch_kk(metric, D)
    if kk >= 256:
        return len(ratio), rel
    return int(np.count_nonzero(ratio >= theta[max(kk, 0)])), rel


def far_records(h, off, row, pair=True):
    """hashes of `row` with a member beyond the window of the row's unit: columns first + 1 .. first + 32, first = the unit's
    first row (pair: the even row of the pair).  A hash the first row shares with its partner is the partner's as well: it
    counts here for either row that holds it."""
    first = row & ~1 if pair else row
    ph, _, _, last = _lists(h, off)
    mine = h[int(off[row]):int(off[row + 1])]
    return int(np.count_nonzero(last[np.searchsorted(ph, mine)] > first + 32))


def falls_back(h, off, metric, D, min_ref_size, pair=True):
    """first rows of the units rk_near_kernel hands to its fallback: some row of the unit has far_records >= floor_common"""
    sizes = np.diff(off).astype(np.int64)
    n, out = len(sizes), []
    for first in range(0, n, 2 if pair else 1):
        rows = [first] + ([first + 1] if pair and first + 1 < n else [])
        if any(far_records(h, off, r, pair) >= floor_common(metric, D, int(sizes[r]), min_ref_size) for r in rows):
            out.append(first)
    return out


def brute_force_tiles(h, off):
    """records per tile from all pairs of genomes, for small collections: a hash is a record of (b, w) when two DIFFERENT
    genomes hold it, one in b and one in w"""
    n = len(off) - 1
    sets = [set(h[int(off[g]):int(off[g + 1])].tolist()) for g in range(n)]
    per = {}
    for i in range(n):
        for j in range(i + 1, n):
            for x in sets[i] & sets[j]:
                per.setdefault((i >> 5, j >> 5), set()).add(x)
    return {k: len(v) for k, v in per.items()}


# ---- section 2: tiles that hold exactly one cell -------------------------------------------------------------------------
COMMONS = (1, 2, 3, 15, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1025)
CELL_EDGE = (0, 3, 6, 9)      # these pairs: row 31 of their block against column 0 of theirs
CELL_DIAGONAL = 16            # this pair: inside one block
CELL_BG = 1500


@functools.lru_cache(maxsize=None)
def cells_collection():
    """24 blocks less 7 genomes of 1,500 private hashes; seventeen identical pairs (a sketch of `common` hashes, twice), one
    member in a block of the first half, one in the second; (h, off, bits, [(i, j, common)])"""
    n = 24 * 32 - 7
    pool, parts, pairs = Hashes(), [None] * n, []
    for p, c in enumerate(COMMONS):
        if p == CELL_DIAGONAL:
            i, j = 5 * 32 + 3, 5 * 32 + 28
        else:
            b, w = p % 12, 12 + (p * 5 + p // 12) % 12
            edge = p in CELL_EDGE
            i = b * 32 + (31 if edge else (7 * p + 2) % 31)
            j = w * 32 + (0 if edge else 1 + (11 * p) % 24)     # (1 .. 24: inside the partial last block too)
        assert parts[i] is None and parts[j] is None and i < j < n
        parts[i] = pool.take(c)
        parts[j] = parts[i].copy()
        pairs.append((i, j, c))
    for g in range(n):
        if parts[g] is None:
            parts[g] = pool.take(CELL_BG)
    h, off = csr(parts)
    for a in (h, off):
        a.setflags(write=False)
    return h, off, BITS, tuple(pairs)


# ---- section 3: tiles on the bound ---------------------------------------------------------------------------------------
BOUND_D = (0.02, 0.05, 0.1)
LEVELS = (5, 17, 30, 45)      # levels of the 256-entry table with a pair of thresholds on either side
BOUND_S, LEVEL_S, BOUND_BG = 200, 661, 700
BOUND_MIN_REF_SIZE = 1        # the one-hash sketch


def level_thresholds(k):
    """(D tight, D loose): jaccard thresholds whose min_jorc lies a thousandth above / below 2^(-k/8)"""
    out = []
    for side in (1.0 + 1e-3, 1.0 - 1e-3):
        mj = 2.0 ** (-k / 8.0) * side
        out.append(-math.log(2.0 * mj / (1.0 + mj)) / K)
    return tuple(out)


def bound_specs():
    """(kind, metric the pair is tight for, D, row size, column size rule, common): every designated pair of the collection"""
    specs = []
    for D in BOUND_D:
        for delta in (0, -1):
            specs.append(("subset", 0, D, BOUND_S, "subset", first_reportable(0, D, BOUND_S, "subset") + delta))
    for k in LEVELS:
        D = level_thresholds(k)[0]
        specs.append(("subset", 0, D, LEVEL_S, "subset", first_reportable(0, D, LEVEL_S, "subset")))
    for D in BOUND_D:
        for delta in (0, -1):
            specs.append(("equal", 1, D, BOUND_S, BOUND_S, first_reportable(1, D, BOUND_S, BOUND_S) + delta))
    for delta in (0, -1):   # the row three times its column: a bound built from the row alone is wrong
        specs.append(("bigrow", 1, 0.05, 3 * BOUND_S, BOUND_S, first_reportable(1, 0.05, 3 * BOUND_S, BOUND_S) + delta))
    return specs


@functools.lru_cache(maxsize=None)
def bounds_collection():
    """Two blocks per designated pair (row block 2q, column block 2q + 1), 700 private hashes in every other genome, so both
    members are their blocks' smallest and the pair is alone in its tile; an empty sketch in the column block of pair 0 and a
    one-hash sketch in that of pair 1 (both jaccard pairs: lb stays the row's size).  (h, off, bits, [(i, j, spec)])"""
    specs = bound_specs()
    n = 2 * len(specs) * 32 - 5
    pool, parts, pairs = Hashes(), [None] * n, []
    for q, spec in enumerate(specs):
        kind, _, _, s0, rule, c = spec
        i, j = 2 * q * 32 + (5 * q + 31) % 32, (2 * q + 1) * 32 + (3 * q) % 26
        if kind == "subset":
            parts[i] = pool.take(s0)
            parts[j] = parts[i][:c].copy()
        else:
            shared = pool.take(c)
            parts[i] = np.concatenate([shared, pool.take(s0 - c)])
            parts[j] = np.concatenate([shared, pool.take(int(rule) - c)])
        pairs.append((i, j, spec))
    parts[pairs[0][1] + 1] = np.zeros(0, dtype=np.uint32)
    parts[pairs[1][1] + 1] = pool.take(1)
    for g in range(n):
        if parts[g] is None:
            parts[g] = pool.take(BOUND_BG)
    h, off = csr(parts)
    for a in (h, off):
        a.setflags(write=False)
    return h, off, BITS, tuple(pairs)


def bound_thresholds():
    """[(metric, D)] the bounds collection is joined under: the three D for both metrics, the level thresholds for jaccard"""
    out = [(m, D) for m in (0, 1) for D in BOUND_D]
    for k in LEVELS:
        out += [(0, D) for D in level_thresholds(k)]
    return out


# ---- section 4: sites of the near-window kernel ---------------------------------------------------------------------------
SITE_D = {0: 0.05, 1: 0.1}
SITE_Q = 1000                          # a site's row
SITE_PAD = 200                         # jaccard: a genome that holds fewer hashes of a row is padded to this with private ones
SITE_STRIDE = 80


FAMILY = 20                            # more than a cell list of 16 entries holds


def site_counts(metric):
    """(floor_common of a site's row, first_reportable of a relative)"""
    D = SITE_D[metric]
    return (floor_common(metric, D, SITE_Q, SITE_Q),
            first_reportable(metric, D, SITE_Q, "subset" if metric == 0 else SITE_Q))


def site_min_ref_size(kind, metric):
    """the smallest sketch: containment collections hold nothing below a row's 1,000 hashes (the bound of every row is built
    from it); jaccard: the far genome of floor_common - 1 hashes, or the padded one of the loud collection"""
    return SITE_Q if metric else min(site_counts(0)[0] - 1, SITE_PAD if kind in ("loud", "family") else SITE_Q)


def site_specs(kind, metric):
    """[(row odd?, row size, [(column - unit's first row, shared hashes, their first position in the row)])].
    jaccard relatives are subsets of the row; containment relatives have the row's 1,000 hashes, the shared part among them."""
    fc, fr = site_counts(metric)
    quiet = [
        (0, SITE_Q, [(1, fr, 0), (32, fr, fr), (33, fc - 1, 2 * fr)]),             # first row: window's first and last column, far below the bound
        (1, SITE_Q, [(2, fr, 0), (32, fr, fr), (33, fc - 1, 2 * fr)]),             # partner: its r + 1, first + 32, far
    ]
    if metric:
        quiet.append((0, 3 * SITE_Q, [(1, fr, 0), (32, fr, fr), (33, fc - 1, 2 * fr)]))   # the row three times its columns
    loud = [
        (0, SITE_Q, [(1, fr, 0), (33, fc, fr)]),               # far == floor_common: falls back, not reported
        (0, SITE_Q, [(1, fr, 0), (33, fr, fr)]),               # far == first_reportable, first column behind the window: reported
        (1, SITE_Q, [(2, fr, 0), (33, fr, fr)]),               # the same for the partner: only 32 columns away, still outside
        (0, SITE_Q, [(33, fr - 1, 0), (50, 1, fr - 1)]),       # the far hashes over two genomes: falls back, nothing to report
        (0, SITE_Q, [(1, 700, 0), (33, fr, 0)]),               # hashes of the first row, its partner AND a far genome: the shared slices
    ]
    if metric:
        loud.append((0, 3 * SITE_Q, [(33, fr, 0)]))
    # a far family: FAMILY genomes behind the window with first_reportable hashes of the row each -- the row falls back and
    # brings that many cells into the fallback's cell list
    family = [(0, SITE_Q, [(33 + i, fr, 0) for i in range(FAMILY)])]
    return {"quiet": quiet, "edge": quiet + loud[:1], "loud": quiet + loud, "family": quiet + loud + family}[kind]


@functools.lru_cache(maxsize=None)
def sites_collection(kind, metric, big=False):
    """Sites 80 ids apart that share nothing with each other, an odd number of genomes with one more site on the last two
    rows (the row n - 2 and its relative n - 1, a unit without a partner); big: one genome of 66,000 private hashes (32-bit
    counters in rk_dist_kernel).  (h, off, bits)"""
    specs = site_specs(kind, metric)
    fc, fr = site_counts(metric)
    n = SITE_STRIDE * len(specs) + 13
    pool, held, rows = Hashes(), {}, {}
    for t, (odd, size, rels) in enumerate(specs):
        first = SITE_STRIDE * t + 10
        rowh = pool.take(size)
        rows[first + odd] = rowh
        for col, cnt, at in rels:
            assert at + cnt <= size and first + col not in rows
            held.setdefault(first + col, []).append(rowh[at:at + cnt])
    rows[n - 2] = pool.take(SITE_Q)
    held.setdefault(n - 1, []).append(rows[n - 2][:fr])
    parts = []
    for g in range(n):
        if g in rows:
            assert g not in held
            parts.append(rows[g])
            continue
        got = held.get(g, [])
        have = sum(len(x) for x in got)
        if metric:
            want = SITE_Q
        else:
            want = 300 if not got else max(have, SITE_PAD)
        if big and g == 5:
            want = 66000
        parts.append(np.concatenate(got + [pool.take(want - have)]))
    h, off = csr(parts)
    for a in (h, off):
        a.setflags(write=False)
    return h, off, BITS


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_index(key):
    h, off, bits = collection(key)[:3]
    return ok.index_build32(h, off, bits)


def collection(key):
    """a collection by its key: ("cells",), ("bounds",), ("sites", kind, metric[, big])"""
    return {"cells": cells_collection, "bounds": bounds_collection, "sites": sites_collection}[key[0]](*key[1:])


@functools.lru_cache(maxsize=None)
def oracle_hits(key, metric, D):
    h, off, bits = collection(key)[:3]
    postings, counts = _oracle_index(key)
    want, _ = ok.index_dist32(counts, bits, postings, np.diff(off).astype(np.uint32), h, off, 1, metric, K, D, threads=8)
    want.setflags(write=False)
    return want
