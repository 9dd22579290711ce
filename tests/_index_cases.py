"""Collections that put the index build (rk_index.hip and its .inc files) on each of its switches, one generator per case.

make(case, leg) returns (hashes, off, bits, env, expect): the sketches as a CSR (uint32 hashes, uint64 for more than 32 bits),
the hash bits, the environment the context and the build run under, and what the leg is ABOUT:
  expect["plan"]     words of rk_index_build_plan that must come out as stated (capi.PLAN_WORDS)
  expect["report"]   words of rk_index_build_report (capi.REPORT_WORDS)
  expect["products"] rk_index_products right after the build
The plan words are plan_build's / plan_attempt's arithmetic (rk_index_plan.h) evaluated by hand for the shape, see the comment of
each case.  A generator asserts its own preconditions -- exact sizes of the bucket or sub-bucket it is about, every other bucket
within the in-LDS sort, chunk boundaries where stated, an internal order that leaves them there -- on the CPU: a case that misses
its edge fails here, without a GPU.  Everything is cached: the GPU tests and the CPU tests share one copy."""
import functools

import numpy as np

from _order_ref import order_ref, parents_ref
from oracle import oracle as ok
from rabbitkssd_amd import synth

BUCKET_CAP = 4096        # kBucketCap: keys of a bucket the in-LDS sort holds
CROWDED_SUB = 768        # kCrowdedSub: a sub-bucket of more keys sends its bucket to k_bucket_heavy
PART_CHUNK = 65536       # kPartChunk: source elements per workgroup of the partition walk
STAGE_GENOMES = 1024     # kStageGenomes: genome bounds of a chunk staged in LDS
SUB_BITS = 10            # kSubBits
REC_REGIONS = 64         # kRecRegions
OVERFLOW = 1             # kFastOverflow


def tile_records_ref(postings, counts, order):
    """Tile records of an index, by the definition at the top of rk_index_tiles.inc: a run is the members of one posting list
    inside one block of 32 internal ids; a list of r runs writes one record per pair of its runs, r (r - 1) / 2, and one more
    for every run with at least two members.  postings: the .dict payload (lists back to back, caller's ids); counts: the
    list lengths in that order (zeros are skipped: the dense .index array will do); order: orig[] of the index."""
    postings = np.asarray(postings, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    counts = counts[counts > 0]
    assert counts.sum() == len(postings)
    inv = np.empty(len(order), dtype=np.int64)
    inv[np.asarray(order, dtype=np.int64)] = np.arange(len(order))
    n_blocks = (len(order) + 31) // 32
    lst = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    runs, members = np.unique(lst * n_blocks + inv[postings] // 32, return_counts=True)
    r = np.bincount(runs // n_blocks, minlength=len(counts))
    return int((r * (r - 1) // 2).sum() + (members >= 2).sum())


def region_records(hashes, off, bits, B, order):
    """tile records a one-pass build asks of each of its kRecRegions regions of unsorted records: the records of bucket b (the lists
    whose top B hash bits are b, counted as tile_records_ref counts them) go to region b % 64 -- an attempt whose fullest region
    exceeds rec_cap / 64 is repeated"""
    off = np.asarray(off, dtype=np.int64)
    inv = np.empty(len(order), dtype=np.int64)
    inv[np.asarray(order, dtype=np.int64)] = np.arange(len(order))
    n_blocks = (len(order) + 31) // 32
    block = inv[np.repeat(np.arange(len(off) - 1), np.diff(off))] // 32
    lists, lst = np.unique(np.asarray(hashes, dtype=np.uint64), return_inverse=True)
    runs, members = np.unique(lst.astype(np.int64) * n_blocks + block, return_counts=True)
    r = np.bincount(runs // n_blocks, minlength=len(lists))
    per_list = r * (r - 1) // 2 + np.bincount(runs // n_blocks, weights=members >= 2, minlength=len(lists)).astype(np.int64)
    region = (lists >> np.uint64(bits - B)).astype(np.int64) % REC_REGIONS
    return np.bincount(region, weights=per_list, minlength=REC_REGIONS).astype(np.int64)


# ---- building blocks -------------------------------------------------------------------------------------------------
def csr(parts, dtype=np.uint32):
    """sorted sets -> (hashes, off); asserts that they ARE sets (strictly ascending: what the bucket sort takes)"""
    parts = [np.asarray(p, dtype=dtype) for p in parts]
    for p in parts:
        assert len(p) < 2 or np.all(p[1:] > p[:-1])
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)).astype(dtype), off


def one_set(rng, m, space):
    """exactly m distinct uniform values below `space`, ascending (uint64)"""
    s = np.unique(rng.integers(0, space, size=m, dtype=np.uint64))
    while len(s) < m:
        s = np.unique(np.concatenate([s, rng.integers(0, space, size=m - len(s), dtype=np.uint64)]))
    return s


def uniform_parts(rng, sizes, space):
    return [one_set(rng, int(m), space) for m in sizes]


def buckets(hashes, bits, B):
    """keys per bucket of a one-pass build with B bucket bits"""
    return np.bincount((np.asarray(hashes, dtype=np.uint64) >> np.uint64(bits - B)).astype(np.int64), minlength=1 << B)


def bucket_bits(H_pass, eff_bits, target=1536):
    """plan_build: the smallest B >= 1 (at most the hash bits of a pass, at most 15) with ceil(H_pass / target) <= 2^B"""
    B = 1
    while B < eff_bits and B < 15 and (H_pass + target - 1) // target > (1 << B):
        B += 1
    return B


def bits_of(n):
    """genome_bits_of: the smallest b >= 1 with 2^b >= n"""
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def rec_cap_of(H, bits):
    """plan_attempt: room for unsorted tile records of a first attempt, rounded up to whole regions"""
    lam = H / float(1 << bits) if bits < 48 else 0.0
    cap = int(H * (0.5 + 0.6 * lam)) + 65536
    return (cap + REC_REGIONS - 1) // REC_REGIONS * REC_REGIONS


def built(attempts=1, **more):
    """report of a build that the bucket sort finished"""
    r = {"attempts": attempts, "key_retries": 0, "rec_retries": 0, "fell_back": 0, "general": 0, "flags": 0}
    r.update(more)
    return r


def assert_identity_order(h, off):
    """the chunk cases state where genomes lie in the element space the partition walks: the internal order must leave them there"""
    assert np.array_equal(order_ref(h, off), np.arange(len(off) - 1))


# ---- low_bits 0: 7-bit hashes, every hash value a bucket of its own (B 7 = the hash bits; sub-bucket count 1) ------------------
@functools.lru_cache(None)
def _low0():
    rng = np.random.default_rng(70)
    h, off = csr([np.sort(rng.choice(128, size=48, replace=False)) for _ in range(600)])
    b = buckets(h, 7, 7)
    assert len(h) == 600 * 48 and b.min() > 0 and b.max() < CROWDED_SUB    # (one sub-bucket per bucket: it must not count as crowded)
    return h, off


def low_bits_0(leg):
    # H 28,800, target 64: 450 buckets wanted, B stops at the 7 hash bits; low_bits 0; 7 >= 7 and 0 + 10 + 6 key bits: two-pass partition
    h, off = _low0()
    env = {"RK_INDEX_BUCKET_TARGET": "64"}
    tiles = leg == "tiles"
    if tiles:
        env["RK_INDEX_TILES"] = "1"
    plan = {"fast_ok": 1, "tiles_mode": int(tiles), "B": 7, "low_bits": 0, "gb": 10, "rb": 6, "part2": 1, "narrow": 1, "n_pass": 1}
    return h, off, 7, env, {"plan": plan, "report": built(heavy=0, passes=1), "products": 6 if tiles else 1}


# ---- low_bits 31 against 32: the widest low_mask of the partition against the refusal ------------------------------------------
@functools.lru_cache(None)
def _low31(leg):
    rng = np.random.default_rng(31)
    if leg == "bits32":
        parts = uniform_parts(rng, [200] * 12, 1 << 32)
        ends = np.array([0, 0xFFFFFFFF], dtype=np.uint64)                          # both ends of the hash space
        parts[3] = np.unique(np.concatenate([parts[3], ends]))
        parts[11] = np.unique(np.concatenate([parts[11], parts[3][:50], ends[1:]]))
        return csr(parts)
    n = 150 if leg == "bits36_low31" else 100
    parts = uniform_parts(rng, [200] * n, 1 << 36)
    top = np.array([(1 << 36) - 1], dtype=np.uint64)
    parts[n - 1] = np.unique(np.concatenate([parts[n - 1][:150], parts[0][:50], top]))   # relatives, and the top of the space
    parts[0] = np.unique(np.concatenate([parts[0], top]))
    return csr(parts, np.uint64)


def low_bits_31_32(leg):
    h, off = _low31(leg)
    H = len(h)
    if leg == "bits32":
        # 12 x ~200: ceil(H / 1536) = 2 buckets, B 1, low_bits 31; genome bits 4: (hash_low, genome) takes 35 bits, u64 keys
        assert (H + 1535) // 1536 == 2
        plan = {"fast_ok": 1, "tiles_mode": 0, "B": 1, "low_bits": 31, "gb": 4, "narrow": 0}
        return h, off, 32, {}, {"plan": plan, "report": built(heavy=0), "products": 1}
    if leg == "bits36_low31":
        # 150 x 200: 20 buckets wanted, B 5, low_bits 31: the bucket sort
        assert 16 < (H + 1535) // 1536 <= 32
        plan = {"fast_ok": 1, "tiles_mode": 0, "B": 5, "low_bits": 31, "gb": 8, "narrow": 0}
        return h, off, 36, {}, {"plan": plan, "report": built(heavy=0), "products": 1}
    # 100 x 200: 14 buckets wanted, B 4, low_bits 32: refused by the plan, the general path without an attempt
    assert 8 < (H + 1535) // 1536 <= 16
    plan = {"fast_ok": 0, "slices_ok": 0, "tiles_ok": 0, "B": 4, "low_bits": 32}
    return h, off, 36, {}, {"plan": plan, "report": built(attempts=0, general=1, heavy=0, passes=0), "products": 1}


# ---- narrow 32 against 33: u32 and u64 sort keys, in every instance of both emission kernels ------------------------------------
@functools.lru_cache(None)
def _narrow(n):
    rng = np.random.default_rng(n)
    # clades of 8: strain s keeps 16 of the ancestor's 20 hashes, so lists and tile records have more than one member
    parts = []
    for c in range((n + 7) // 8):
        anc = one_set(rng, 20, 1 << 26)
        for s in range(8):
            own = one_set(rng, 4, 1 << 26) if s else anc[:0]
            parts.append(np.unique(np.concatenate([anc[: 20 if not s else 16], own]))[:20])
    parts = parts[:n]
    assert all(len(p) == 20 for p in parts)
    return csr(parts)


def narrow_32_33(leg):
    # 26 bits, 20,480 (20,500) postings: 14 buckets wanted, B 4, low_bits 22; 1,024 genomes need 10 bits (32: u32 keys), 1,025 need 11
    side, prod, t = leg.split("-")
    n = 1024 if side == "narrow" else 1025
    h, off = _narrow(n)
    assert len(h) == 20 * n and bucket_bits(len(h), 26) == 4
    env = {"RK_INDEX_EMIT_T": t}
    if prod == "tiles":
        env["RK_INDEX_TILES"] = "1"
    plan = {"fast_ok": 1, "tiles_mode": int(prod == "tiles"), "B": 4, "low_bits": 22, "gb": bits_of(n), "narrow": int(n == 1024), "emit_t": int(t),
            "big_ok": int(prod == "tiles" and n == 1024)}
    return h, off, 26, env, {"plan": plan, "report": built(heavy=0, passes=1), "products": 6 if prod == "tiles" else 1}


# ---- a real key equal to the padding key 0xFFFFFFFF ------------------------------------------------------------------------------
@functools.lru_cache(None)
def _padding(everyone):
    rng = np.random.default_rng(99)
    ones = [np.uint64((b << 22) | 0x3FFFFF) for b in range(16)]            # per bucket the hash whose 22 low bits are all ones
    m = 8 if everyone else 20                                                  # (24,576 postings at most: B stays 4)
    parts = uniform_parts(rng, [m] * 1024, 1 << 26)
    for g in range(0 if everyone else 1024 - 40, 1024):
        parts[g] = np.unique(np.concatenate([parts[g], ones]))
        assert len(parts[g]) == m + 16
    return csr(parts)


def key_equals_padding(leg):
    # the narrow-32 shape: key = hash_low << 10 | internal genome; internal genome 1,023 holds the all-ones hash of bucket 15: 0xFFFFFFFF
    everyone = leg == "heavy"
    h, off = _padding(everyone)
    assert bucket_bits(len(h), 26) == 4 and buckets(h, 26, 4).max() <= BUCKET_CAP
    order = np.arange(1024) if leg == "relabel0" else order_ref(h, off)
    last = int(order[1023])
    assert 0x3FFFFFF in h[int(off[last]): int(off[last + 1])]                 # the key 0xFFFFFFFF exists
    sub = np.bincount((h & np.uint32(0x3FFFFF)) >> 12, minlength=1024)         # (per sub-bucket index over all buckets: an upper bound)
    env = {"relabel0": {"RK_INDEX_RELABEL": "0"}, "default": {}, "tiles": {"RK_INDEX_TILES": "1"}, "heavy": {"RK_INDEX_TILES": "1"}}[leg]
    tiles = leg in ("tiles", "heavy")
    # the list of 40 leaves every sub-bucket below kCrowdedSub; held by all 1,024 genomes it crowds the last sub-bucket of all 16 buckets
    heavy = 16 if everyone else 0
    assert (sub.max() >= 16 * 1024) if everyone else (sub.max() < CROWDED_SUB)
    plan = {"fast_ok": 1, "tiles_mode": int(tiles), "B": 4, "low_bits": 22, "gb": 10, "narrow": 1, "relabel": int(leg != "relabel0"), "big_ok": int(tiles)}
    return h, off, 26, env, {"plan": plan, "report": built(heavy=heavy, passes=1), "products": 6 if tiles else 1}


# ---- part2 at B 6 against 7: k_part_scatter against k_part_coarse + k_part_fine ---------------------------------------------------
@functools.lru_cache(None)
def _part2(n):
    names, h, off = synth.clade_sketches(n, 200, 26, seed=600 + n)
    return h, off


def part2_threshold(leg):
    # 26 bits, 450 x ~200: 59 buckets wanted, B 6: one scattering pass; 550 x ~200: 72, B 7: two passes, unless RK_INDEX_PART2=0
    n = 450 if leg == "b6" else 550
    h, off = _part2(n)
    B = 6 if n == 450 else 7
    assert bucket_bits(len(h), 26) == B
    env = {"RK_INDEX_PART2": "0"} if leg == "b7_one_pass" else {}
    plan = {"fast_ok": 1, "tiles_mode": 0, "B": B, "low_bits": 26 - B, "part2": int(leg == "b7")}
    return h, off, 26, env, {"plan": plan, "report": built(heavy=0, passes=1), "products": 1}


# ---- the coarse pass in four workgroups of 256 against one of 1,024 ---------------------------------------------------------------
@functools.lru_cache(None)
def _coarse(n, m):
    names, h, off = synth.clade_sketches(n, m, 26, seed=n + m)
    return h, off


def coarse_variants(leg):
    # 26 bits, target 64: 1,000 x 250 want 3,907 buckets (B 12: 64 coarse buckets, small workgroups); 2,200 x 250 want 8,594 (B 14: 256
    # coarse buckets, the 1,024-thread pass); 4,200 x 260 want 17,063 (B 15, the most there are).  4,200 genomes get tile records.
    n, m, B = {"b12": (1000, 250, 12), "b14": (2200, 250, 14), "b14_xcd0": (2200, 250, 14), "b15": (4200, 260, 15)}[leg]
    h, off = _coarse(n, m)
    assert bucket_bits(len(h), 26, 64) == B and len(h) <= 1_100_000
    env = {"RK_INDEX_BUCKET_TARGET": "64", "RK_INDEX_XCD": "0" if leg == "b14_xcd0" else "1"}
    tiles = n >= 4000
    plan = {"fast_ok": 1, "tiles_mode": int(tiles), "B": B, "low_bits": 26 - B, "part2": 1, "small_wgs": int(B <= 13)}
    return h, off, 26, env, {"plan": plan, "report": built(heavy=0, passes=1), "products": 6 if tiles else 1}


# ---- bucket capacity and the crowded sub-bucket ---------------------------------------------------------------------------------
CAP_BUCKET = 17          # the bucket the background avoids (of 32: B 5, low_bits 21)


@functools.lru_cache(None)
def _background():
    """1,000 genomes x 40 hashes of 26 bits, none in CAP_BUCKET"""
    rng = np.random.default_rng(4096)
    parts = uniform_parts(rng, [40] * 1000, 31 << 21)
    return [p + np.uint64(1 << 21) * (p >> np.uint64(21) >= CAP_BUCKET) for p in parts]


@functools.lru_cache(None)
def _capacity(keys):
    """... and exactly `keys` keys in CAP_BUCKET: lists of four neighbouring genomes (4 j .. 4 j + 3: one run, one tile record each, so that
    the bucket's region of unsorted records does not overflow and the build stays at one attempt), spread over the sub-buckets"""
    rng = np.random.default_rng(keys)
    pool = (keys + 3) // 4
    low = np.sort(rng.choice(1 << 21, size=pool, replace=False)).astype(np.uint64)
    extra = [[] for _ in range(1000)]
    for k in range(keys):
        q, r = divmod(k, pool)
        extra[4 * (r % 250) + q].append((CAP_BUCKET << 21) | int(low[r]))
    parts = [np.unique(np.concatenate([p, np.array(e, dtype=np.uint64)])) for p, e in zip(_background(), extra)]
    h, off = csr(parts)
    b = buckets(h, 26, 5)
    assert len(h) == 40000 + keys and bucket_bits(len(h), 26) == 5
    assert b[CAP_BUCKET] == keys and np.delete(b, CAP_BUCKET).max() <= BUCKET_CAP
    mine = h[(h >> 21) == CAP_BUCKET]
    assert np.bincount((mine & np.uint32((1 << 21) - 1)) >> 11, minlength=1024).max() < CROWDED_SUB
    asked = region_records(h, off, 26, 5, order_ref(h, off))
    assert keys // 4 <= asked[CAP_BUCKET] and asked.max() <= rec_cap_of(len(h), 26) // REC_REGIONS
    return h, off


def bucket_capacity(leg):
    # 26 bits, 40,000 + keys postings: 27 .. 29 buckets wanted, B 5, low_bits 21, genome bits 10: narrow
    prod, keys = leg.split("-")[0], int(leg.split("-")[1])
    h, off = _capacity(keys)
    env = {"slices": {}, "tiles": {"RK_INDEX_TILES": "1"}, "tiles_noheavy": {"RK_INDEX_TILES": "1", "RK_INDEX_NO_HEAVY": "1"}}[prod]
    over = keys > BUCKET_CAP
    plan = {"fast_ok": 1, "tiles_mode": int(prod != "slices"), "B": 5, "low_bits": 21, "gb": 10, "narrow": 1, "big_ok": int(prod == "tiles")}
    if over and prod != "tiles":     # the kernels raise the overflow flag: the general path after one attempt
        return h, off, 26, env, {"plan": plan, "report": built(general=1, flags=OVERFLOW, passes=1), "products": 1}
    return h, off, 26, env, {"plan": plan, "report": built(heavy=int(over), passes=1), "products": 1 if prod == "slices" else 6}


@functools.lru_cache(None)
def _crowded(members):
    rng = np.random.default_rng(members)
    crowd = np.uint64((CAP_BUCKET << 21) | (5 << 11) | 77)                       # sub-bucket 5 of CAP_BUCKET: nobody else's
    low = rng.choice(1 << 21, size=600, replace=False)
    low = low[(low >> 11) != 5][:500].astype(np.uint64)
    assert len(low) == 500
    parts = []
    for g, p in enumerate(_background()):
        add = ([crowd] if g < members else []) + ([np.uint64(CAP_BUCKET << 21) | low[g - 500]] if g >= 500 else [])
        parts.append(np.unique(np.concatenate([p, np.array(add, dtype=np.uint64)])))
    h, off = csr(parts)
    mine = h[(h >> 21) == CAP_BUCKET]
    sub = np.bincount((mine & np.uint32((1 << 21) - 1)) >> 11, minlength=1024)
    assert sub[5] == members == int((h == crowd).sum()) and np.delete(sub, 5).max() < CROWDED_SUB
    assert bucket_bits(len(h), 26) == 5 and buckets(h, 26, 5).max() <= BUCKET_CAP
    return h, off


def crowded_sub_bucket(leg):
    members = int(leg)
    h, off = _crowded(members)
    plan = {"fast_ok": 1, "tiles_mode": 1, "B": 5, "low_bits": 21, "gb": 10, "narrow": 1, "big_ok": 1}
    return h, off, 26, {"RK_INDEX_TILES": "1"}, {"plan": plan, "report": built(heavy=int(members > CROWDED_SUB), passes=1), "products": 6}


# ---- chunk geometry of the partition walk ------------------------------------------------------------------------------------
def sizes_to(rng, total, lo, hi):
    """random sketch sizes in [lo, hi) that add up to exactly `total`"""
    sizes = []
    while sum(sizes) < total:
        sizes.append(int(rng.integers(lo, hi)))
    sizes[-1] -= sum(sizes) - total
    if sizes[-1] == 0:
        sizes.pop()
    assert sum(sizes) == total and min(sizes) > 0
    return sizes


@functools.lru_cache(None)
def _chunks(shape):
    rng = np.random.default_rng(len(shape) * 1000 + sum(map(ord, shape)))
    space, dtype = (1 << 24, np.uint32)
    if shape in ("h131071", "h131072", "h131073"):
        sizes = sizes_to(rng, int(shape[1:]), 96, 160)
    elif shape == "aligned":      # genomes end exactly at elements 65,536 and 131,072
        sizes = sizes_to(rng, PART_CHUNK, 96, 160) + sizes_to(rng, PART_CHUNK, 96, 160) + sizes_to(rng, 20000, 96, 160)
    elif shape == "empties":      # empty sketches first, last, on both sides of the boundary at 65,536 and at the one at 131,072
        sizes = [0] + sizes_to(rng, PART_CHUNK - 6, 96, 160) + [0, 12, 0] + sizes_to(rng, PART_CHUNK - 6, 96, 160) + [0, 0] + sizes_to(rng, 9000, 96, 160) + [0]
    else:                         # exactly 1,024 (1,025) genomes have elements in chunk 0: sketches of 63 there, one of 2,000 across its end
        first = STAGE_GENOMES - 1 if shape == "stage1024" else STAGE_GENOMES
        sizes = [63] * first + [2000] + sizes_to(rng, 2 * PART_CHUNK + 500 - 63 * first - 2000, 96, 160)
        if shape == "stage1025_wide":
            space, dtype = (1 << 36, np.uint64)
    parts = uniform_parts(rng, sizes, space)
    # every seventh genome is a relative of the one before it (a tight self join has hits): it takes that one's largest hashes for half
    # of its own -- never one of its 16 smallest, which would move it in the internal order
    for g in range(7, len(parts), 7):
        if 60 <= len(parts[g]) < 160 and 60 <= len(parts[g - 1]) < 160:
            k = min(len(parts[g]), len(parts[g - 1])) // 2
            parts[g] = np.unique(np.concatenate([parts[g][:-k], parts[g - 1][-k:]]))
    assert [len(p) for p in parts] == sizes
    h, off = csr(parts, dtype)
    assert_identity_order(h, off)
    o = off.astype(np.int64)
    if shape == "aligned":
        assert PART_CHUNK in o and 2 * PART_CHUNK in o and len(h) > 2 * PART_CHUNK
    if shape == "empties":
        sz = np.diff(o)
        at = lambda e: np.flatnonzero((sz == 0) & (o[:-1] == e))     # noqa: E731
        assert sz[0] == 0 and sz[-1] == 0 and len(at(PART_CHUNK - 6)) == 1 and len(at(PART_CHUNK + 6)) == 1 and len(at(2 * PART_CHUNK)) == 2
    if shape.startswith("stage"):
        in_chunk0 = int(((o[:-1] < PART_CHUNK) & (np.diff(o) > 0)).sum())
        assert in_chunk0 == (STAGE_GENOMES if shape == "stage1024" else STAGE_GENOMES + 1) and o[in_chunk0] > PART_CHUNK
    return h, off


CHUNK_SHAPES = ("h131071", "h131072", "h131073", "aligned", "empties", "stage1024", "stage1025", "stage1025_wide")


def chunk_geometry(leg):
    # target 256, so that a pass of half the hashes still has 128 buckets and more (the two-pass partition, which the filter needs):
    # one pass of ~131,000 .. 151,000 keys wants 512 .. 590 buckets, B 9 or 10; a pass of half of them B 8 or 9
    shape, mode = leg.rsplit("-", 1)
    h, off = _chunks(shape)
    H, bits = len(h), 36 if shape.endswith("wide") else 24
    env = {"RK_INDEX_BUCKET_TARGET": "256"}
    if mode != "one":
        env["RK_INDEX_PASS_BITS"] = "1"
    if mode == "walk":
        env["RK_INDEX_FILTER"] = "0"
    if shape.startswith("h"):
        assert H == int(shape[1:])
    n_pass = 1 if mode == "one" else 2
    B = bucket_bits(H if mode == "one" else H >> 1, bits - (n_pass - 1), 256)
    assert B >= 7
    plan = {"fast_ok": 1, "tiles_mode": int(n_pass == 2), "n_pass": n_pass, "range_bits": n_pass - 1, "use_filter": int(mode == "filter"), "part2": 1, "B": B,
            "keys_cap": H if mode == "one" else min(H, (H >> 1) * 125 // 100 + (1 << 20))}
    return h, off, bits, env, {"plan": plan, "report": built(heavy=0, passes=n_pass), "products": 6 if n_pass == 2 else 1}


# ---- attempts that carry state ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _species():
    names, h, off = synth.clade_sketches(3000, 120, 26, strains_per_clade=3000, seed=3000)
    postings, counts = ok.index_build32(h, off, 26)
    return h, off, tile_records_ref(postings, counts, np.arange(3000))


def attempts(leg):
    # one species of 3,000 strains in the caller's order: its lists touch all 94 blocks, far more tile records than a first attempt
    # has room for (H / 2 + 64 K), within the budget of one retry (6 H + 2^22)
    h, off, records = _species()
    H = len(h)
    rec_cap = rec_cap_of(H, 26)
    assert rec_cap < records <= 6 * H + (1 << 22)
    env = {"RK_INDEX_RELABEL": "0", "RK_INDEX_TILES": "1"}
    plan = {"fast_ok": 1, "tiles_mode": 1, "slices_ok": 1, "relabel": 0, "rec_cap": rec_cap, "n_pass": 1}
    if leg == "records":           # (a) the records do not fit: once more with room for them
        return h, off, 26, env, {"plan": plan, "report": built(attempts=2, rec_retries=1, passes=1), "products": 6, "tile_records": records}
    if leg == "keys_then_records":  # (b) four range passes with buffers for 60 % of their keys: the keys first, then the records
        # (a pass of 90,000 keys wants 59 buckets of 1,536: B 6, the one-pass partition, which has no filter to count what a range
        # needs -- the build would go straight to the general path; buckets of 512 make it B 8)
        env.update({"RK_INDEX_PASS_BITS": "2", "RK_INDEX_KEYS_CAP_PCT": "60", "RK_INDEX_BUCKET_TARGET": "512"})
        top = np.bincount(h >> 24, minlength=4)
        cap = (H >> 2) * 60 // 100
        assert top.max() > cap and bucket_bits(H >> 2, 24, 512) == 8
        plan.update({"n_pass": 4, "slices_ok": 0, "keys_cap": cap, "use_filter": 1, "part2": 1, "B": 8})
        return h, off, 26, env, {"plan": plan, "report": built(attempts=3, key_retries=1, rec_retries=1, passes=4), "products": 6, "tile_records": records}
    # (c) no retry allowed (RK_TILE_REC_CAP): slice records after all.  With the default bucket target two of the species' lists of
    # ~2,000 share a bucket, which the slice-record emission cannot sort in LDS: the overflow flag, the general path.  (d) with
    # buckets of 64 every bucket fits, and the second attempt builds the slice records.
    env["RK_TILE_REC_CAP"] = "4096"
    plan["rec_cap"] = 4096
    if leg == "fall_back":
        assert buckets(h, 26, bucket_bits(H, 26)).max() > BUCKET_CAP
        return h, off, 26, env, {"plan": plan, "report": built(attempts=2, fell_back=1, general=1, flags=OVERFLOW, passes=1), "products": 1}
    env["RK_INDEX_BUCKET_TARGET"] = "64"
    B = bucket_bits(H, 26, 64)
    assert buckets(h, 26, B).max() <= BUCKET_CAP
    plan["B"] = B
    return h, off, 26, env, {"plan": plan, "report": built(attempts=2, fell_back=1, heavy=0, passes=1), "products": 1}


# ---- the internal order ----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _clades(n):
    names, h, off = synth.clade_sketches(n, 20, 24, seed=n)
    names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(n, "shuffled", seed=n))
    return h, off


@functools.lru_cache(None)
def _table_full():
    """64 unrelated genomes of exactly 16 hashes: 1,024 distinct values, as many as the renumbering's table has slots at RK_INDEX_TABLE_X=1"""
    rng = np.random.default_rng(64)
    all_h = one_set(rng, 1024, 1 << 24)
    rng.shuffle(all_h)
    h, off = csr([np.sort(all_h[16 * g: 16 * g + 16]) for g in range(64)])
    assert len(np.unique(h)) == 1024
    return h, off


def fold_partner(v):
    """another 36-bit hash with the same 32-bit fold h ^ (h >> 32)"""
    return v ^ np.uint64((1 << 32) | 1)


@functools.lru_cache(None)
def _fold36():
    rng = np.random.default_rng(36)
    parts = uniform_parts(rng, [20] * 200, 1 << 36)
    for c in range(5):                      # five clades of four around genomes 30, 34, ...
        for s in range(1, 4):
            parts[30 + 4 * c + s] = np.unique(np.concatenate([parts[30 + 4 * c][:12], parts[30 + 4 * c + s][:8]]))
    for g in range(10):                     # genome 100 + g shares no hash with genome g, but the folds of g's two smallest
        parts[100 + g] = np.unique(np.concatenate([fold_partner(parts[g][:2]), parts[100 + g][2:]]))
        assert len(np.intersect1d(parts[g], parts[100 + g])) == 0 and len(parts[100 + g]) == 20
    h, off = csr(parts, np.uint64)
    parent = parents_ref(h, off)
    assert all(parent[100 + g] == g for g in range(10)) and parent[33] == 30
    return h, off


@functools.lru_cache(None)
def _small_sketches():
    rng = np.random.default_rng(15)
    parts = uniform_parts(rng, [20] * 120, 1 << 24)
    parts[0] = parts[0][:0]                                        # empty, first
    parts[7] = parts[3][:1]                                        # one hash, shared: one vote attaches nothing
    parts[9] = parts[9][:1]                                        # one hash of its own
    parts[40] = np.unique(np.concatenate([parts[5][:2], parts[40][:13]]))      # 15 hashes, two of genome 5's smallest: attaches
    parts[41] = np.unique(np.concatenate([parts[5][:1], parts[41][:14]]))      # 15 hashes, one shared: does not
    parts[60] = parts[60][:0]
    parts[119] = np.unique(np.concatenate([parts[40][:15], parts[119][:3]]))   # follows 40 to 5
    h, off = csr(parts)
    parent = parents_ref(h, off)
    assert len(parts[40]) == 15 and parent[40] == 5 and parent[41] == 41 and parent[7] == 7 and parent[119] == 5
    return h, off


def order(leg):
    if leg.startswith("n"):
        n, _, mode = leg[1:].partition("-")
        n = int(n)
        h, off = _clades(n)
        env = {"": {}, "one_stream": {"RK_INDEX_ONE_STREAM": "1"}, "tiles1": {"RK_INDEX_TILES": "1"}, "tiles0": {"RK_INDEX_TILES": "0"}}[mode]
        tiles = n >= 2 and (mode == "tiles1" or (n >= 4000 and mode != "tiles0"))
        bits = 24
    else:
        h, off = {"table_full": _table_full, "fold36": _fold36, "small_sketches": _small_sketches}[leg]()
        # (fold36: 4,000 postings in 36 bits want 3 buckets of 1,536, low_bits 34: no bucket sort; buckets of 64 make it B 6, low_bits 30)
        env = {"table_full": {"RK_INDEX_TABLE_X": "1"}, "fold36": {"RK_INDEX_BUCKET_TARGET": "64"}, "small_sketches": {}}[leg]
        n, tiles, bits = len(off) - 1, False, 36 if leg == "fold36" else 24
    assert n <= 33000 and len(h) <= 1_100_000
    want = order_ref(h, off)
    if n > 64:
        assert not np.array_equal(want, np.arange(n))              # (the case is about an order that moves genomes)
    plan = {"fast_ok": 1, "tiles_mode": int(tiles), "relabel": int(n > 1), "two_streams": int(n > 1 and "RK_INDEX_ONE_STREAM" not in env)}
    return h, off, bits, env, {"plan": plan, "report": built(passes=1), "products": 6 if tiles else 1}


# ---- the table of cases ------------------------------------------------------------------------------------------------------
CASES = {
    "low_bits_0": (low_bits_0, ("slices", "tiles")),
    "low_bits_31_32": (low_bits_31_32, ("bits32", "bits36_low31", "bits36_low32")),
    "narrow_32_33": (narrow_32_33, tuple("%s-%s-%s" % (s, p, t) for s in ("narrow", "wide") for p in ("slices", "tiles") for t in ("256", "512", "1024"))),
    "key_equals_padding": (key_equals_padding, ("relabel0", "default", "tiles", "heavy")),
    "part2_threshold": (part2_threshold, ("b6", "b7", "b7_one_pass")),
    "coarse_variants": (coarse_variants, ("b12", "b14", "b14_xcd0", "b15")),
    "bucket_capacity": (bucket_capacity, ("slices-2048", "slices-2049", "slices-4095", "slices-4096", "slices-4097", "tiles-4096", "tiles-4097",
                                          "tiles_noheavy-4097")),
    "crowded_sub_bucket": (crowded_sub_bucket, ("768", "769")),
    "chunk_geometry": (chunk_geometry, tuple("%s-%s" % (s, m) for s in CHUNK_SHAPES for m in ("one", "filter", "walk"))),
    "attempts": (attempts, ("records", "keys_then_records", "fall_back", "fall_back_small_buckets")),
    "order": (order, ("n1", "n2", "n33", "n32768", "n32769", "n32768-one_stream", "n32769-one_stream", "n32768-tiles1", "n32769-tiles1", "n32768-tiles0",
                      "n32769-tiles0", "table_full", "fold36", "small_sketches")),
}


def all_legs():
    return [(case, leg) for case, (_, legs) in CASES.items() for leg in legs]


def make(case, leg):
    return CASES[case][0](leg)
