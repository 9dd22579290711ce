"""Generators and a plain model for the self join with full counter rows, rk_dist_kernel (tests/test_rows_ref_cpu.py,
tests/test_gpu_rows_edges.py).

The model restates with numpy what the kernel's paths depend on, from the sketches alone:

    slices()        the slice records of the index (rk_index.hip k_self_raw / compact_slice): one per (genome, hash) with later
                    holders; compact or posting range; covered by the row's pair partner or open
    unit_classes()  per unit (a row, or the pair r, r + 1) the path every slice takes: counted in the 32-column window, the
                    rotated bit walk, a range of <= 8 / 9..24 / > 24 postings, held by the partner, shared with the partner;
                    and its place in the batches of THREADS slices (which long ranges meet in one wave)
    candidates()    per unit and column tile the cells that enter the cell list (common >= the row bound, min_common)
    list_events()   what the per-unit list and the two batch lists do with a run of units: wait, flush, overflow, final

and the generators place slices and candidate counts ON those seams.  Nothing is drawn at random: hashes ascend in the order
they are handed out (`Ascending`), so a row's slices lie in the order of its specification.  Bands are not modelled: the GPU
tests read the plan's own `band:` lines (RK_DIST_DEBUG=1) where tiles matter."""
import functools

import numpy as np

from oracle import oracle as ok

import _prune_ref as pr

K = pr.K
BITS = 26
csr = pr.csr
min_jorc = pr.min_jorc
# the row-level reject of rk_dist_kernel and rk_distq_kernel (floor_common in the kernels): max(1, floor(min_jorc * lb)),
# lb = the row's size (jaccard) / min(the row's size, the smallest non-empty sketch) (containment)
min_common = pr.floor_common

WINDOW, ROTATED, SHORT, MID, LONG = range(5)     # the path of a slice
FORM_NAMES = ("window", "rotated", "range<=8", "range9..24", "range>24")
GROUP = 8                                        # postings a quad gathers (kGroup)


class Ascending:
    """fresh hashes, ascending in the order they are taken (a row's slices lie in its sketch's order) and spread over the space"""

    def __init__(self, stride=977, bits=BITS):
        self.stride, self.bits, self.next = stride, bits, 1

    def take(self, n=1):
        a = np.arange(self.next, self.next + n, dtype=np.uint64) * np.uint64(self.stride)
        assert int(a[-1]) < 1 << self.bits
        self.next += n
        return a.astype(np.uint32)


# ---- the model -----------------------------------------------------------------------------------------------------------
SLICE_DTYPE = np.dtype([("g", "<i8"), ("e", "<i8"), ("lo", "<i8"), ("hi", "<i8"), ("first", "<i8"), ("last", "<i8"),
                        ("n", "<i8"), ("compact", "?"), ("covered", "?")])


def slices(h, off):
    """dict(rec, postings, sets, row_off): `rec` holds one record per (genome g, source element e) whose hash has later holders
    -- their posting positions [lo, hi) in `postings` (every hash's holders ascending, hashes ascending), first / last holder,
    n = hi - lo -- in the order of the index: rows ascending, a row's open records in source order, then its covered ones.
    compact: the sketches are sets and last - first <= 31.  covered: g is odd, g - 1 holds the hash (and the slice is not empty).
    row_off[g] .. row_off[g + 1]: the records of row g."""
    sizes = np.diff(off).astype(np.int64)
    n = len(sizes)
    gid = np.repeat(np.arange(n, dtype=np.int64), sizes)
    order = np.lexsort((gid, h))                  # (stable: a genome's repeats of a hash keep their source order)
    ph, pg = h[order], gid[order]
    new = np.r_[True, ph[1:] != ph[:-1]] if len(ph) else np.zeros(0, dtype=bool)
    starts = np.flatnonzero(new)
    end_of = np.r_[starts[1:], len(ph)][np.cumsum(new) - 1] if len(ph) else np.zeros(0, dtype=np.int64)
    k = np.arange(len(ph), dtype=np.int64)
    prev = np.r_[-1, pg[:-1]]
    sets = not bool(np.any(~new & (prev == pg)))
    has = k + 1 < end_of
    covered = has & (pg % 2 == 1) & ~new & (prev == pg - 1)
    kk = k[has]
    rec = np.zeros(len(kk), dtype=SLICE_DTYPE)
    rec["g"], rec["e"], rec["lo"], rec["hi"] = pg[kk], order[kk], kk + 1, end_of[kk]
    rec["first"], rec["last"] = pg[kk + 1], pg[end_of[kk] - 1]
    rec["n"] = rec["hi"] - rec["lo"]
    rec["compact"] = sets & (rec["last"] - rec["first"] <= 31)
    rec["covered"] = covered[kk]
    rec = rec[np.lexsort((rec["e"], rec["covered"], rec["g"]))]
    row_off = np.searchsorted(rec["g"], np.arange(n + 1))
    return dict(rec=rec, postings=pg, sets=sets, row_off=row_off)


def slice_totals(s):
    """what rk_index_self_stats reports: [0] records, [1] compact ones, [2] records the pair kernel walks (all of an even row,
    the open ones of an odd row)"""
    rec = s["rec"]
    return len(rec), int(rec["compact"].sum()), int(np.count_nonzero((rec["g"] % 2 == 0) | ~rec["covered"]))


def brute_force_totals(h, off):
    """the same three numbers from Python lists, for tiny collections"""
    n = len(off) - 1
    sk = [h[int(off[g]):int(off[g + 1])].tolist() for g in range(n)]
    sets = all(len(set(x)) == len(x) for x in sk)
    records = compact = walked = 0
    for g in range(n):
        for i, x in enumerate(sk[g]):
            later = [j for j in range(g + 1, n) for y in sk[j] if y == x] + [g] * sk[g][i + 1:].count(x)
            if not later:
                continue
            later.sort()
            records += 1
            compact += sets and later[-1] - later[0] <= 31
            is_covered = g % 2 == 1 and x in sk[g - 1] and sk[g][:i].count(x) == 0
            walked += not is_covered
    return records, compact, walked


UNIT_DTYPE = np.dtype([("pos", "<i8"), ("batch", "<i8"), ("wave", "<i8"), ("lane", "<i8"), ("form", "<i8"), ("n", "<i8"),
                       ("first", "<i8"), ("last", "<i8"), ("in_b", "?"), ("shared", "?"), ("rec", "<i8")])


def unit_classes(s, row, pair, threads):
    """the slices unit `row` walks, in the order of its batches: a single row walks all its records (open, then covered); a pair
    (row even) walks the first row's records and then the partner's OPEN ones.  form: compact records are counted in the window
    iff first - base < 32 and no bit is shifted out (last - base <= 31), base = row + 1, else walked bit by bit from a rotated
    start; ranges by length.  in_b: held by the partner; shared: a first-row record whose first holder is the partner.
    wave: within the batch; rec: index into s["rec"]."""
    rec, ro = s["rec"], s["row_off"]
    n = len(ro) - 1
    idx = list(range(ro[row], ro[row + 1]))
    n_a = len(idx)
    partner = row + 1 if pair and row + 1 < n else -1
    if pair:
        assert row % 2 == 0
        if partner >= 0:
            idx += [i for i in range(ro[partner], ro[partner + 1]) if not rec["covered"][i]]
    out = np.zeros(len(idx), dtype=UNIT_DTYPE)
    base = row + 1
    for p, i in enumerate(idx):
        r = rec[i]
        if r["compact"]:
            form = WINDOW if r["first"] - base < 32 and r["last"] - base <= 31 else ROTATED
        else:
            form = SHORT if r["n"] <= GROUP else (MID if r["n"] <= GROUP + 16 else LONG)
        in_b = p >= n_a
        out[p] = (p, p // threads, (p % threads) // 64, p % 64, form, r["n"], r["first"], r["last"], in_b,
                  (not in_b) and partner >= 0 and r["first"] == partner, i)
    return out


def long_ranges_per_wave(u):
    """{(batch, wave): lengths of the ranges longer than 8 that wave holds in that batch, in lane order}"""
    out = {}
    for x in u[u["form"] >= MID]:
        out.setdefault((int(x["batch"]), int(x["wave"])), []).append(int(x["n"]))
    return out


def common_matrix(h, off):
    """[n, n] int32: hashes two genomes share (set sketches); the diagonal holds the sketch sizes"""
    s = slices(h, off)
    assert s["sets"]
    n = len(off) - 1
    m = np.zeros((n, n), dtype=np.int32)
    pg = s["postings"]
    sizes = np.diff(off).astype(np.int64)
    m[np.arange(n), np.arange(n)] = sizes
    rec = s["rec"]
    np.add.at(m, (np.repeat(rec["g"], rec["n"]), np.concatenate([pg[a:b] for a, b in zip(rec["lo"], rec["hi"])]) if len(rec) else np.zeros(0, dtype=np.int64)), 1)
    return m + np.triu(m, 1).T


def candidates(common, sizes, metric, D, unit_rows=1, tile_cols=None, col_base=0):
    """[units, tiles] cells behind the diagonal that enter the cell list: common >= min_common of their row.  A unit is
    unit_rows consecutive rows from an even row on (the last may be a lone row); tiles of tile_cols columns from col_base."""
    n = len(sizes)
    nz = sizes[sizes > 0]
    mrs = int(nz.min()) if len(nz) else 0
    tile_cols = tile_cols or max(1, n - col_base)
    n_tiles = (n - col_base + tile_cols - 1) // tile_cols
    n_units = (n + unit_rows - 1) // unit_rows
    out = np.zeros((n_units, n_tiles), dtype=np.int64)
    for r in range(n):
        if sizes[r] == 0:
            continue
        cols = r + 1 + np.flatnonzero(common[r, r + 1:] >= min_common(metric, D, int(sizes[r]), mrs))
        cols = cols[cols >= col_base]
        np.add.at(out[r // unit_rows], (cols - col_base) // tile_cols, 1)
    return out


def list_events(counts, cap, batch):
    """what the sparse epilogue does with a run of consecutive units of one workgroup whose cell counts are `counts`.
    batch (from 512 threads on): entries wait in the current list over several units; ("overflow", waiting, n) when a unit
    brings the list above cap, ("flush", total) from cap / 2 on, ("wait", total) below, and ("final", waiting) at the end of the
    run.  Per-unit list (below 512 threads): ("overflow", 0, n) above cap, else ("fits", n)."""
    ev, waiting = [], 0
    for n in counts:
        n = int(n)
        if not batch:
            ev.append(("overflow", 0, n) if n > cap else ("fits", n))
            continue
        total = waiting + n
        if total > cap:
            ev.append(("overflow", waiting, n))
            waiting = 0
        elif total >= cap // 2:
            ev.append(("flush", total))
            waiting = 0
        else:
            ev.append(("wait", total))
            waiting = total
    if batch:
        ev.append(("final", waiting))
    return ev


def run_events(unit_counts, cap, batch, units_per_wg):
    """list_events of every run of units_per_wg consecutive units (RK_DIST_PERSIST=2: run k is the units k * units_per_wg ..)"""
    return [list_events(unit_counts[a:a + units_per_wg], cap, batch) for a in range(0, len(unit_counts), units_per_wg)]


# ---- collection 1: slice forms and pair sharing (legs A and B) -------------------------------------------------------------
FORMS_N = 337                 # odd: the last unit is a lone row, and (337 - 1) / 2 = 168 is the first unit of an XCD chunk of 8
HUB, PAIR_A = 10, 40          # the hub row (base 11) and the pair (40, 41) (base 41)
EMPTY_FIRST, EMPTY_SECOND = 320, 325   # empty sketches behind every spread list: the first member of (320, 321), the second of (324, 325)
FORMS_D = 0.35                # containment: every designated cell is reportable (asserted from the oracle's hits)
RANGE_LENGTHS = (2, 7, 8, 9, 23, 24, 25, 24 + 63, 24 + 64, 24 + 65, 24 + 128, 24 + 129)
SIX = (9, 24, 16, 10, 12, 30)           # four ranges for the 16-lane rows, a fifth and a sixth for the whole wave
SIX_WAVES = (0, 3, 4, 7, 8, 15, 16)     # of the hub row: first wave, last wave and second batch at 256, 512 and 1,024 threads
HUB_SLICES = 17 * 64 + 12


def spread(length, start, room):
    """`length` distinct offsets from `start` on that span more than 31 ids"""
    span = max(40, 2 * (length - 1))
    assert start + span < room
    return [start + (i * span) // (length - 1) for i in range(length)]


def hub_specs(room):
    """[(kind, offsets from the base of the holders of one hub hash)] in slice order; waves of 64"""
    specs = []
    # wave 0: compact lists at the window's last column, against the rotated walk
    for first in (0, 1, 30, 31):
        for last in (31, 32):
            specs.append(("edge", [first, last] if first != last else [first]))     # (0, 32) spans 32 ids: a range of two
    specs.append(("all32", list(range(32))))                  # every bit, in the window
    specs.append(("all32_rot", list(range(1, 33))))           # every bit, one column on: rotated walk
    specs.append(("bit31", [5, 36]))                          # the only far bit is bit 31
    for t in range(8):                                        # eight neighbours: every rotation lane & 7
        specs.append(("rot8", [2 + t, 9 + t, 33 + t]))
    six = lambda w: [("six", spread(n, 0 if (i + w) % 2 == 0 else 2, room)) for i, n in enumerate(SIX)]
    specs += six(0)
    fill = lambda k: [("fill", [(len(specs) + j) % 24]) for j in range(k)]
    specs += fill(64 - len(specs))
    # wave 1: ranges of every length at the seams 8 | 9, 24 | 25 and the stream's trips of 128
    specs += [("range", spread(n, 1 + i % 3, room)) for i, n in enumerate(RANGE_LENGTHS)]
    specs += fill(128 - len(specs))
    # wave 2: exactly four ranges for the 16-lane rows
    specs += [("four", spread(n, 2, room)) for n in (9, 24, 10, 23)]
    specs += fill(192 - len(specs))
    for w in range(3, 18):
        if w in SIX_WAVES:
            specs += fill(20)
            specs += six(w)
        specs += fill(min(HUB_SLICES, (w + 1) * 64) - len(specs))
    assert len(specs) == HUB_SLICES
    return specs


def pair_specs(room):
    """[(holders of the pair: "ab" | "a" | "b", kind, offsets from the base 41 of the LATER holders; 0 is the partner itself)]"""
    specs = [("ab", "only", [])]                                          # held by 2p and 2p + 1 only: mask 1, nothing for the partner
    specs += [("ab", "compact", [3, 7]), ("ab", "compact", [1, 31])]
    specs += [("ab", "range", spread(n - 1, 2, room)) for n in (8, 9, 24, 25, 26, 40, 24 + 65)]   # (n counts the partner)
    specs += [("b", "compact", [1, 2]), ("b", "compact", [2, 31]), ("b", "rotated", [2, 32])]
    specs += [("b", "range", spread(n, 1, room)) for n in (5, 12, 30)]
    specs += [("a", "compact", [1, 5]), ("a", "rotated", [3, 33])]
    specs += [("a", "range", spread(n, 2, room)) for n in (6, 14, 28)]
    return specs


@functools.lru_cache(maxsize=None)
def forms_collection(multiset=False):
    """337 genomes: the hub row 10 with 1,100 slices of every form, placed wave by wave (hub_specs); the pair (40, 41) with
    hashes of both, of either (pair_specs); the empty sketches 320 and 325, whose partners hold hashes with later genomes; two
    private hashes everywhere else.  multiset: genome 200 holds one of its hashes twice, which 201 and 250 hold as well.
    (h, off, bits, designated) -- designated: {(row, col): common}, every non-zero cell of the rows 10, 40, 41, 61, 70 by the generator's count."""
    n = FORMS_N
    pool, parts, want = Ascending(), [[] for _ in range(n)], {}
    a, b = PAIR_A, PAIR_A + 1
    special = {HUB, a, b, EMPTY_FIRST + 1, EMPTY_SECOND - 1}
    empty = {EMPTY_FIRST, EMPTY_SECOND}

    def give(rows, cols):
        x = pool.take(1)
        for g in list(rows) + list(cols):
            assert g < n and g not in empty
            parts[g].append(x)
        for r in special & (set(rows) | set(cols)):     # (every hash of a designated row comes through here)
            for c in set(rows) | set(cols):
                if c > r:
                    want[(r, c)] = want.get((r, c), 0) + 1

    base = HUB + 1
    for _, offs in hub_specs(n - base):
        give([HUB], [base + o for o in offs])
    for who, _, offs in pair_specs(n - b):
        give({"ab": [a, b], "a": [a], "b": [b]}[who], [b + o for o in offs if o > 0])
    give([EMPTY_FIRST + 1], [322, 323, 330])
    give([EMPTY_SECOND - 1], [326, 333])
    for g in range(n):
        if g not in special | empty:
            parts[g].append(pool.take(2))
    if multiset:
        x = pool.take(1)
        for g in (200, 200, 201, 250):
            parts[g].append(x)
    h, off = csr([np.concatenate(p) if p else np.zeros(0, dtype=np.uint32) for p in parts])
    for arr in (h, off):
        arr.setflags(write=False)
    return h, off, BITS, want


# ---- collection 2: cell counts on the list's capacity (leg C) ---------------------------------------------------------------
LISTS_N = 1001
LISTS_D = 0.1                 # containment; every cell with a shared hash is a candidate AND reportable (a row of <= 2 hashes)
LISTS_T0, LISTS_T1 = 133, 532  # the target genomes: off a quad boundary (133 = 16 * 8 + 5), across column 512
LISTS_CAPS = (256, 16)
WELL_ABOVE = {256: 400, 16: 40}


def lists_row_counts():
    """cells behind the diagonal, row by row (128 rows).  Per capacity c, 64 rows: the sweep c - 4 .. c + 9 and one row well
    above, every one followed by a row of 3 (single rows: the unit after an overflow; pairs: c - 1 .. c + 12); then four runs of
    four pairs for the batch lists (units_per_wg = 4): [h, 1, 0, 0] (exactly cap / 2: flush; entries left at the end),
    [h - 1, h + 2, 3, 0] (cap + 1 though the unit fits), [c + 5, 2, 0, 0] (alone above cap), [h - 1, h + 1, 0, 0] (exactly cap)."""
    rows = []
    for c in LISTS_CAPS:
        hh = c // 2
        for v in list(range(c - 4, c + 10)) + [WELL_ABOVE[c]]:
            rows += [v, 3]
        rows += [0, 0]
        for run in ([hh, 1, 0, 0], [hh - 1, hh + 2, 3, 0], [c + 5, 2, 0, 0], [hh - 1, hh + 1, 0, 0]):
            for u in run:
                rows += [u - u // 4, u // 4]
    assert len(rows) == 128
    return rows


@functools.lru_cache(maxsize=None)
def lists_collection():
    """1,001 genomes.  Row r < 128 holds one or two hashes (r odd: two) that its lists_row_counts()[r] targets hold as well:
    the rows of the first 64 take targets from 133 upwards, the others from 532 downwards (the tile boundary 512 cuts both
    kinds); everything else holds one private hash.  (h, off, bits)"""
    n = LISTS_N
    pool, parts = Ascending(), [[] for _ in range(n)]
    for r, cnt in enumerate(lists_row_counts()):
        x = pool.take(1 + r % 2)
        parts[r].append(x)
        targets = range(LISTS_T0, LISTS_T0 + cnt) if r < 64 else range(LISTS_T1 - cnt + 1, LISTS_T1 + 1)
        assert cnt <= LISTS_T1 - LISTS_T0 + 1
        for t in targets:
            parts[t].append(x)
    for g in range(n):
        if not parts[g] or g >= 128:
            parts[g].append(pool.take(1))
    h, off = csr([np.concatenate(p) for p in parts])
    for arr in (h, off):
        arr.setflags(write=False)
    return h, off, BITS


def tile_cols_of(n_cols, n_tiles):
    """make_plan: the columns are shared evenly among the tiles, in whole stretches of 64"""
    return ((n_cols + n_tiles - 1) // n_tiles + 63) & ~63


# ---- collection 3: counter width (leg E) ------------------------------------------------------------------------------------
WIDTH_BIG = (6, 9, 12)


@functools.lru_cache(maxsize=None)
def width_collection(big, repeat=False):
    """35 genomes: three identical sketches of `big` hashes at ids 6, 9 and 12 -- the cell (6, 9) is the high half of its LDS
    word, (6, 12) and (9, 12) the low half, and all count `big`; small sketches that share 3 hashes with them in the other halves
    of those words (8 and 13) and around (7, 10, 11, 20); repeat: genome 9 holds one more copy of its first hash.  (h, off, bits)"""
    n = 35
    pool, parts = Ascending(stride=500), [[] for _ in range(n)]
    x = pool.take(big)
    for g in WIDTH_BIG:
        parts[g].append(x)
    if repeat:
        parts[9].append(x[:1])
    for g in (7, 8, 10, 11, 13, 20):
        parts[g].append(x[g:g + 3])
    for g in range(n):
        if g not in WIDTH_BIG:
            parts[g].append(pool.take(5))
    h, off = csr([np.concatenate(p) for p in parts])
    for arr in (h, off):
        arr.setflags(write=False)
    return h, off, BITS


# ---- collection 4: more units than the chip holds workgroups (leg C3) -------------------------------------------------------
QUEUES_N, QUEUES_ROWS, QUEUES_T0 = 2199, 1800, 1879      # 320 targets from 1879 (off a quad boundary) to the end


@functools.lru_cache(maxsize=None)
def queues_collection():
    """2,199 genomes, 1,100 pairs.  The rows below 1,800 are heavy (257 .. 316 targets hold their hash: above the cell list),
    light (three targets) or empty, in random order -- a workgroup's units lie a whole grid apart, so a pattern whose period
    divides the grid would hand every workgroup one kind only.  (h, off, bits, kinds)"""
    rng = np.random.default_rng(77)
    kinds = rng.integers(0, 4, size=QUEUES_ROWS)       # 0 heavy, 1 and 2 light, 3 empty
    pool, parts = Ascending(), [[] for _ in range(QUEUES_N)]
    for r in range(QUEUES_ROWS):
        if kinds[r] == 3:
            continue
        x = pool.take(1)
        parts[r].append(x)
        for t in range(QUEUES_T0, QUEUES_T0 + (257 + r % 60 if kinds[r] == 0 else 3)):
            parts[t].append(x)
    for g in range(QUEUES_ROWS, QUEUES_N):
        parts[g].append(pool.take(1))
    h, off = csr([np.concatenate(p) if p else np.zeros(0, dtype=np.uint32) for p in parts])
    for arr in (h, off, kinds):
        arr.setflags(write=False)
    return h, off, BITS, kinds


def queues_conditions(stage_hits, cap=256):
    """(workgroups of a launch with one pair per workgroup, padded to whole XCD chunks; the model's slice totals)"""
    h, off, _, kinds = queues_collection()
    n = len(off) - 1
    assert QUEUES_T0 % 8 != 0 and QUEUES_T0 + 316 <= n and n % 2 == 1
    for k in (0, 1, 3):
        assert np.count_nonzero(kinds == k) >= QUEUES_ROWS // 5
    sizes = np.diff(off).astype(np.int64)
    assert np.array_equal(sizes[:QUEUES_ROWS] == 0, kinds == 3)
    want = oracle_hits(("queues",), 1, LISTS_D)
    per_row = np.bincount(want["row"], minlength=n)[:QUEUES_ROWS]
    assert np.all(per_row[kinds == 0] > cap) and np.all(per_row[(kinds == 1) | (kinds == 2)] == 3)
    grid = ((n + 1) // 2 + 63) // 64 * 64
    assert len(want) > stage_hits * grid
    return grid, slice_totals(_model(("queues",))[0])


# ---- collection 5: relatives across band and tile boundaries (leg D) ---------------------------------------------------------
BANDS_D = 0.3


def bands_pairs(n, band_rows, tile_edges):
    """the pairs a plan's boundaries ask for.  band_rows: the first row of every band but the first; around each, pairs with one
    member in either band, both ways for the rows of a pair (2p in one band and the relative of 2p + 1 in the next).
    tile_edges: [(a row of the band, first column of a tile behind it)]: that row and its neighbour against the last column of
    one tile and the first of the next."""
    pairs = set()
    for b in band_rows:
        for i, j in ((b - 2, b + 1), (b - 1, b), (b - 1, b + 2), (b - 2, b), (b, b + 1), (b - 3, b - 1)):
            if 0 <= i < j < n:
                pairs.add((i, j))
    for r, c in tile_edges:
        for i in (r, r + 1):
            for j in (c - 1, c):
                if 0 <= i < j < n:
                    pairs.add((i, j))
    return sorted(pairs)


def bands_collection(n, pairs):
    """n genomes of two private hashes; every pair of `pairs` shares three hashes of its own.  (h, off, bits)"""
    pool, parts = Ascending(stride=2000), [[] for _ in range(n)]
    for g in range(n):
        parts[g].append(pool.take(2))
    for i, j in pairs:
        x = pool.take(3)
        parts[i].append(x)
        parts[j].append(x)
    h, off = csr([np.concatenate(p) for p in parts])
    return h, off, BITS


def dist_hits(h, off, bits, metric, D):
    postings, counts = ok.index_build32(h, off, bits)
    return ok.index_dist32(counts, bits, postings, np.diff(off).astype(np.uint32), h, off, 1, metric, K, D, threads=8)[0]


# ---- the oracle ------------------------------------------------------------------------------------------------------------
COLLECTIONS = {"forms": forms_collection, "lists": lists_collection, "width": width_collection, "queues": queues_collection}


def collection(key):
    """a collection by its key: ("forms", multiset), ("lists",), ("width", big, repeat)"""
    return COLLECTIONS[key[0]](*key[1:])


@functools.lru_cache(maxsize=None)
def _oracle_index(key):
    h, off, bits = collection(key)[:3]
    return ok.index_build32(h, off, bits)


@functools.lru_cache(maxsize=None)
def oracle_hits(key, metric, D):
    h, off, bits = collection(key)[:3]
    postings, counts = _oracle_index(key)
    want, _ = ok.index_dist32(counts, bits, postings, np.diff(off).astype(np.uint32), h, off, 1, metric, K, D, threads=8)
    want.setflags(write=False)
    return want


def hit_cells(hits):
    """{(row, col): common}"""
    return dict(zip(zip(hits["row"].tolist(), hits["col"].tolist()), hits["common"].tolist()))


# ---- the conditions the collections were built for: asserted on the CPU, and again by every GPU leg ------------------------
@functools.lru_cache(maxsize=None)
def _model(key):
    h, off = collection(key)[:2]
    return slices(h, off), np.diff(off).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _common(key):
    return common_matrix(*collection(key)[:2])


def _has(u, **want):
    """some slice of the unit with these properties (d_first / d_last: relative to the unit's base)"""
    m = np.ones(len(u), dtype=bool)
    for k, v in want.items():
        m &= u[k] == v
    return bool(m.any())


@functools.lru_cache(maxsize=None)
def forms_conditions(multiset, pair, threads):
    """the seams of legs A and B are present in forms_collection(multiset) for a kernel that walks pairs (`pair`) or single rows
    in batches of `threads` slices; returns the model's slice totals"""
    key = ("forms", multiset)
    s, sizes = _model(key)
    n = len(sizes)
    totals = slice_totals(s)
    assert s["sets"] == (not multiset) and (totals[1] == 0) == multiset and not (multiset and pair)
    assert n % 2 == 1 and ((n - 1) // 2) % 8 == 0            # a lone last row, the first unit of its XCD chunk
    assert sizes[EMPTY_FIRST] == 0 and sizes[EMPTY_SECOND] == 0 and EMPTY_FIRST % 2 == 0 and EMPTY_SECOND % 2 == 1
    ro = s["row_off"]
    assert ro[EMPTY_FIRST + 2] > ro[EMPTY_FIRST + 1] and ro[EMPTY_SECOND] > ro[EMPTY_SECOND - 1]     # their partners have slices
    u = unit_classes(s, HUB, pair, threads)
    assert len(u) >= HUB_SLICES > 1024
    base = HUB + 1
    rel = np.zeros(len(u), dtype=[("d_first", "<i8"), ("d_last", "<i8")])
    rel["d_first"], rel["d_last"] = u["first"] - base, u["last"] - base
    edge = {(0, 31): WINDOW, (1, 31): WINDOW, (30, 31): WINDOW, (31, 31): WINDOW, (1, 32): ROTATED, (30, 32): ROTATED,
            (31, 32): ROTATED, (0, 32): SHORT}
    for (f, l), form in edge.items():
        m = (rel["d_first"] == f) & (rel["d_last"] == l) & (u["n"] <= 2)
        assert m.any() and (multiset or np.all(u["form"][m] == form)), (f, l)
    ranges = u[u["form"] >= SHORT]
    assert set(RANGE_LENGTHS) <= set(ranges["n"].tolist())
    assert np.all((ranges["last"] - ranges["first"] > 31) | multiset)
    if not multiset:
        assert np.any((u["n"] == 32) & (u["form"] == WINDOW)) and np.any((u["n"] == 32) & (u["form"] == ROTATED))   # all 32 bits
        assert np.any((u["form"] == ROTATED) & (u["n"] == 2) & (u["last"] - u["first"] == 31))                       # bit 31 alone
        rot = u["form"] == ROTATED
        runs = [p for p in range(len(u) - 7) if rot[p:p + 8].all() and u["wave"][p] == u["wave"][p + 7] and np.all(u["n"][p:p + 8] >= 3)]
        assert runs and set((u["lane"][runs[0]:runs[0] + 8] & 7).tolist()) == set(range(8))    # every rotation, side by side
    per_wave = long_ranges_per_wave(u)
    assert any(len(v) == 4 and max(v) <= GROUP + 16 for v in per_wave.values())              # the four 16-lane rows, no more
    for where in ((0, 0), (0, threads // 64 - 1), (1, 0)):                                   # first wave, last wave, second batch
        v = per_wave.get(where, [])
        assert len(v) >= 6 and sum(GROUP < x <= GROUP + 16 for x in v) >= 4 and max(v) > GROUP + 16, (where, v)
    if pair:
        for form in (WINDOW, SHORT, MID, LONG):
            assert _has(u, shared=True, form=form), form
        p = unit_classes(s, PAIR_A, True, threads)
        assert _has(p, shared=True, form=WINDOW, n=1)                                        # held by the pair only: mask 1
        for nn, form in ((3, WINDOW), (8, SHORT), (9, MID), (24, MID), (25, LONG), (24 + 65, LONG)):
            assert _has(p, shared=True, form=form, n=nn), nn
        for form in (WINDOW, ROTATED, SHORT, MID, LONG):
            assert _has(p, in_b=True, form=form), form                                       # open slices of the partner
            assert _has(p, in_b=False, shared=False, form=form), form                        # the first row's alone
        rec = s["rec"]
        assert np.count_nonzero(rec["covered"] & (rec["g"] == PAIR_A + 1)) >= 9
        assert totals[2] < totals[0]
    return totals


@functools.lru_cache(maxsize=None)
def lists_conditions(cap, kind, tile_cols=512):
    """the seams of leg C are present in lists_collection() for a cell list of `cap` entries.  kind: "single" (per-unit list,
    runs of two rows), "pairs" (batch lists, runs of four pairs), "tiles" (single rows, column tiles of tile_cols)"""
    key = ("lists",)
    s, sizes = _model(key)
    want = oracle_hits(key, 1, LISTS_D)
    rows = lists_row_counts()
    designed = want[want["row"] < len(rows)]
    assert np.array_equal(np.bincount(designed["row"], minlength=len(rows)), rows)           # every designed cell is reported
    assert LISTS_T0 % 8 != 0 and (LISTS_T1 + 1) % 8 != 0 and LISTS_T0 < tile_cols <= LISTS_T1
    m = _common(key)
    if kind == "single":
        c = candidates(m, sizes, 1, LISTS_D)[:, 0]
        assert c[:len(rows)].tolist() == rows
        assert {cap - 1, cap, cap + 1, cap + 9} <= set(c.tolist()) and c.max() >= cap + cap // 2
        runs = run_events(c, cap, False, 2)
        assert any(r[0][0] == "overflow" and r[1][0] == "fits" and r[1][1] >= 1 for r in runs if len(r) == 2)   # the unit after an overflow
    elif kind == "pairs":
        c = candidates(m, sizes, 1, LISTS_D, unit_rows=2)[:, 0]
        assert {cap - 1, cap, cap + 1, cap + 9} <= set(c.tolist())
        ev = [e for r in run_events(c, cap, True, 4) for e in r]
        assert ("flush", cap // 2) in ev and ("flush", cap) in ev
        assert any(e[0] == "overflow" and e[1] == cap // 2 - 1 and e[1] + e[2] == cap + 1 for e in ev)
        assert any(e[0] == "overflow" and e[1] == 0 and e[2] > cap for e in ev)
        assert any(e[0] == "final" and e[1] > 0 for e in ev)
    else:
        c = candidates(m, sizes, 1, LISTS_D, tile_cols=tile_cols)
        assert c.shape[1] == 2 and np.any(c > cap)
        assert np.any((c.max(axis=1) > cap) & (c.min(axis=1) > 0))       # a row across the boundary that overflows the list in one tile
    return slice_totals(s)
