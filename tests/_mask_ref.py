"""The rule of rk_sketches_mask / rk_mask_lists in plain Python, twice and independently: from a collections.Counter over the references'
hashes (the definition of include/rabbitkssd.h: c(h) = how often the references hold h, a repeat inside a reference counted) and from
exported lists by bisect.  Integers only.  tests/test_mask_cpu.py checks the two against each other; everything else is checked
against them.

    refs, queries   lists of iterables of hashes; a reference that repeats a hash counts it twice, a query keeps its repeats and its order
    result          per query the list of its surviving hashes, in the query's order"""
import bisect
import collections
import itertools

import numpy as np

MAX = 0xFFFFFFFF   # UINT32_MAX: no upper bound
SUB, PRESENT = (0, 0), (1, MAX)


def from_counter(refs, queries, min_refs, max_refs):
    """the definition: c(h) from a Counter over every hash of every reference"""
    assert min_refs <= max_refs
    c = collections.Counter(int(h) for r in refs for h in r)
    return [[int(h) for h in q if min_refs <= c[int(h)] <= max_refs] for q in queries]


def exported(refs):
    """(list_hashes, counts) as rk_index_export_lists / rk_index_export64 return them: the distinct hashes ascending, the length of each
    one's posting list"""
    every = sorted(int(h) for r in refs for h in r)
    hashes = sorted(set(every))
    return hashes, [bisect.bisect_right(every, h) - bisect.bisect_left(every, h) for h in hashes]


def from_lists(list_hashes, counts, queries, min_refs, max_refs):
    """from exported lists: a binary search per query hash, the count of the list found or 0"""
    assert min_refs <= max_refs and len(list_hashes) == len(counts)
    out = []
    for q in queries:
        kept = []
        for h in q:
            at = bisect.bisect_left(list_hashes, int(h))
            c = counts[at] if at < len(list_hashes) and list_hashes[at] == int(h) else 0
            if min_refs <= c <= max_refs:
                kept.append(int(h))
        out.append(kept)
    return out


def fast(refs, queries, min_refs, max_refs):
    return from_lists(*exported(refs), queries, min_refs, max_refs)


def matched(refs, queries):
    """the query hashes that have a posting list, repeats counted"""
    held = set(int(h) for r in refs for h in r)
    return sum(int(h) in held for q in queries for h in q)


def emptied(queries, result):
    """non-empty queries that end empty"""
    return sum(len(q) > 0 and len(k) == 0 for q, k in zip(queries, result))


def as_arrays(result, dtype=np.uint32):
    """(hashes, off) of a result"""
    off = np.zeros(len(result) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(k) for k in result])
    return np.array([h for k in result for h in k], dtype=dtype), off


def parts_of(h, off):
    return [np.asarray(h[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


# ---- every small collection ------------------------------------------------------------------------------------------------------
SUBSETS = [[h + 3 for h in range(5) if m >> h & 1] for m in range(32)]   # every sketch over a universe of 5 hashes
BANDS = [(a, b) for a in range(4) for b in range(a, 4)]                  # every band with bounds in 0 .. 3


def small_collections(max_refs=3):
    """Every collection of up to max_refs references over 5 hashes, up to the ORDER of the references, which cannot matter: c(h) counts
    the holders of h and does not name them.  1 + 32 + 528 + 5,984 collections for max_refs = 3.  The queries that go with each are
    SUBSETS, all 32 at once: a query's survivors depend on its own hashes alone, so the 32 stand for every pair of them, and their
    offsets for every pair's."""
    for n in range(max_refs + 1):
        for refs in itertools.combinations_with_replacement(SUBSETS, n):
            yield list(refs)
