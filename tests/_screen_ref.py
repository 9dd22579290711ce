"""The rule of rk_screen_rows / rk_screen_lists in plain Python, twice and independently: from the hash sets (the definition of
include/rabbitkssd.h, containments as fractions.Fraction, every candidate scanned per hash) and from posting lists (the row's candidates
ranked once with a comparator, then the minimum rank per list).  Integers and exact fractions only.  tests/test_screen_cpu.py checks the
two against each other and against the facts that follow from the rule; everything else is checked against them.

    refs, queries   lists of iterables of hashes, taken as sets
    sizes           the size of every reference; None: the number of its distinct hashes
    result          per query (recs, matched, n_cand, claimed); a record is the tuple REC_FIELDS without the sizes: (query, ref, common, won)"""
import functools
from fractions import Fraction

import numpy as np

REC_FIELDS = ("query", "ref", "common", "won", "size_ref", "size_query")


def selected_rows(n_query, row_first=0, row_step=1, row_block=0):
    """the rows of a shard: blocks of row_block rows dealt round-robin, as rk_gather_opts"""
    rb, rs = max(1, row_block), max(1, row_step)
    return [r for r in range(n_query) if (r // rb) % rs == row_first % rs and (r // rb) >= row_first]


def sizes_of(refs, sizes=None):
    return [len(set(int(h) for h in r)) for r in refs] if sizes is None else [int(s) for s in sizes]


def tallies_from_sets(refs, queries, min_common=1, sizes=None):
    """the definition up to the choice of records: per query (common, won, candidates, matched) -- per matched hash, the best of its
    holders that are candidates: the larger containment (an exact fraction), then the larger size, then the smaller index"""
    assert min_common >= 1
    R = [set(int(h) for h in r) for r in refs]
    size = sizes_of(refs, sizes)
    indexed = set().union(*R) if R else set()
    out = []
    for s in queries:
        S = set(int(h) for h in s)
        common = [len(S & r) for r in R]
        cands = [r for r in range(len(R)) if common[r] >= min_common]
        key = {r: (Fraction(common[r], size[r]), size[r], -r) for r in cands}
        won = [0] * len(R)
        for h in S & indexed:
            holders = [r for r in cands if h in R[r]]
            if holders:
                won[max(holders, key=key.__getitem__)] += 1
        out.append((common, won, cands, len(S & indexed)))
    return out


def records(tallies, min_won=0):
    """the result of a statement from its tallies: the candidates that claim at least min_won hashes, by ascending index"""
    return [([(q, r, common[r], won[r]) for r in cands if won[r] >= min_won], matched, len(cands), sum(won))
            for q, (common, won, cands, matched) in enumerate(tallies)]


def from_sets(refs, queries, min_common=1, min_won=0, sizes=None):
    return records(tallies_from_sets(refs, queries, min_common, sizes), min_won)


def posting_lists(refs):
    """{hash: the references that hold it, ascending, each once}"""
    lists = {}
    for r, s in enumerate(refs):
        for h in sorted(set(int(x) for x in s)):
            lists.setdefault(h, []).append(r)
    return lists


def better(a, b):
    """-1 when candidate a = (common, size, index) is better than b, +1 when worse: integer products, no division"""
    if a[0] * b[1] != b[0] * a[1]:
        return -1 if a[0] * b[1] > b[0] * a[1] else 1
    if a[1] != b[1]:
        return -1 if a[1] > b[1] else 1
    return -1 if a[2] < b[2] else 1 if a[2] > b[2] else 0


def tallies_from_lists(lists, n_ref, queries, sizes, min_common=1):
    """from posting lists: the counters per reference, the row's candidates ranked once, a list goes to its member of the smallest rank"""
    assert min_common >= 1
    out = []
    for s in queries:
        live = [lists[h] for h in sorted(set(int(x) for x in s)) if h in lists]
        common = [0] * n_ref
        for l in live:
            for r in l:
                common[r] += 1
        cands = [r for r in range(n_ref) if common[r] >= min_common]
        order = sorted(((common[r], sizes[r], r) for r in cands), key=functools.cmp_to_key(better))
        rank = {k[2]: i for i, k in enumerate(order)}
        won = [0] * n_ref
        for l in live:
            ranks = [rank[r] for r in l if r in rank]
            if ranks:
                won[order[min(ranks)][2]] += 1
        out.append((common, won, cands, len(live)))
    return out


def from_lists(lists, n_ref, queries, sizes, min_common=1, min_won=0):
    return records(tallies_from_lists(lists, n_ref, queries, sizes, min_common), min_won)


def fast_tallies(refs, queries, min_common=1, sizes=None):
    return tallies_from_lists(posting_lists(refs), len(refs), queries, sizes_of(refs, sizes), min_common)


def fast(refs, queries, min_common=1, min_won=0, sizes=None):
    return from_lists(posting_lists(refs), len(refs), queries, sizes_of(refs, sizes), min_common, min_won)


def facts(refs, queries, result, min_common=1, min_won=0, sizes=None):
    """the facts that follow from the rule, by brute force over the sets; raises AssertionError"""
    R = [set(int(h) for h in r) for r in refs]
    size = sizes_of(refs, sizes)
    every = result if min_won == 0 else from_sets(refs, queries, min_common, 0, sizes)
    for q, (recs, matched, n_cand, claimed) in enumerate(result):
        S = set(int(h) for h in queries[q])
        allrecs = every[q][0]
        assert n_cand == len(allrecs) == sum(len(S & r) >= min_common for r in R)
        assert [t for t in allrecs if t[3] >= min_won] == recs and [t[1] for t in recs] == sorted(t[1] for t in recs)
        assert claimed == sum(t[3] for t in allrecs) <= matched
        if min_common == 1:
            assert claimed == matched
        for (_, r, common, won) in allrecs:
            assert common == len(S & R[r]) and won <= common
        if allrecs:
            key = {t[1]: (Fraction(t[2], size[t[1]]), size[t[1]], -t[1]) for t in allrecs}
            inside = {t[1]: S & R[t[1]] for t in allrecs}
            best = max(allrecs, key=lambda t: key[t[1]])
            assert best[3] == best[2]                       # the best candidate keeps everything it shares
            for t in allrecs:                               # within S a subset of a better candidate's hashes: nothing is left to claim
                if t[3]:
                    assert not any(key[u[1]] > key[t[1]] and inside[t[1]] <= inside[u[1]] for u in allrecs)


def as_arrays(result, refs, queries, rows=None, sizes=None):
    """(off, records as a list of REC_FIELDS tuples, matched, n_cand, claimed) over the selected rows, unselected rows empty and zero"""
    n = len(queries)
    rows = range(n) if rows is None else rows
    sel = set(rows)
    size = sizes_of(refs, sizes)
    off, recs = [0], []
    matched, n_cand, claimed = [0] * n, [0] * n, [0] * n
    for q in range(n):
        if q in sel:
            p, matched[q], n_cand[q], claimed[q] = result[q]
            recs += [t + (size[t[1]], len(set(int(h) for h in queries[q]))) for t in p]
        off.append(len(recs))
    return off, recs, matched, n_cand, claimed


def rec_tuples(recs):
    """a SCREEN_REC_DTYPE array as a list of REC_FIELDS tuples"""
    return [tuple(int(p[f]) for f in REC_FIELDS) for p in recs]


def parts_of(h, off):
    return [np.asarray(h[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def exported(refs, queries):
    """(postings, counts, q_off, q_lists) as rk_screen_lists takes them: the lists in ascending hash order"""
    lists = posting_lists(refs)
    hashes = sorted(lists)
    at = {h: i for i, h in enumerate(hashes)}
    postings = [r for h in hashes for r in lists[h]]
    counts = [len(lists[h]) for h in hashes]
    q_off, q_lists = [0], []
    for s in queries:
        q_lists += sorted(at[h] for h in set(int(x) for x in s) if h in at)
        q_off.append(len(q_lists))
    return postings, counts, q_off, q_lists
