"""The rule of rk_gather_rows / rk_gather_lists in plain Python, twice and independently: from the hash sets (the definition of
include/rabbitkssd.h, word for word) and from posting lists.  Integers only.  tests/test_gather_cpu.py checks the two against each
other and against what singles the result out; everything else is checked against them.

    refs, queries   lists of iterables of hashes, taken as sets
    result          per query (picks, matched, n_cand, covered); a pick is the tuple PICK_FIELDS without the sizes:
                    (query, ref, rank, common, fresh, left)"""
import numpy as np

PICK_FIELDS = ("query", "ref", "rank", "common", "fresh", "left", "size_ref", "size_query")


def selected_rows(n_query, row_first=0, row_step=1, row_block=0):
    """the rows of a shard: blocks of row_block rows dealt round-robin, as rk_dist_opts"""
    rb, rs = max(1, row_block), max(1, row_step)
    return [r for r in range(n_query) if (r // rb) % rs == row_first % rs and (r // rb) >= row_first]


def from_sets(refs, queries, min_new=1, max_picks=0):
    """the definition: M shrinks by the picked reference's hashes, rem is recomputed from the sets in every round"""
    assert min_new >= 1
    R = [set(int(h) for h in r) for r in refs]
    indexed = set().union(*R) if R else set()
    out = []
    for q, s in enumerate(queries):
        S = set(int(h) for h in s)
        M = S & indexed
        matched = len(M)
        common = [len(S & r) for r in R]
        n_cand = sum(c >= min_new for c in common)
        picked, picks = set(), []
        while not max_picks or len(picks) < max_picks:
            rem = [(len(M & R[r]), -r) for r in range(len(R)) if r not in picked]
            if not rem or max(rem)[0] < min_new:
                break
            fresh, r = max(rem)[0], -max(rem)[1]
            M = M - R[r]
            picked.add(r)
            picks.append((q, r, len(picks), common[r], fresh, len(M)))
        out.append((picks, matched, n_cand, sum(p[4] for p in picks)))
    return out


def posting_lists(refs):
    """{hash: the references that hold it, ascending, each once}"""
    lists = {}
    for r, s in enumerate(refs):
        for h in sorted(set(int(x) for x in s)):
            lists.setdefault(h, []).append(r)
    return lists


def from_lists(lists, n_ref, queries, min_new=1, max_picks=0):
    """from posting lists: counters per reference, a list dies when the pick is on it and takes one off every reference it names"""
    assert min_new >= 1
    out = []
    for q, s in enumerate(queries):
        live = [lists[h] for h in sorted(set(int(x) for x in s)) if h in lists]
        matched = len(live)
        rem = [0] * n_ref
        for l in live:
            for r in l:
                rem[r] += 1
        common = list(rem)
        n_cand = sum(c >= min_new for c in common)
        picks, left = [], matched
        while not max_picks or len(picks) < max_picks:
            best = max(range(n_ref), key=lambda r: (rem[r], -r)) if n_ref else None
            if best is None or rem[best] < min_new:
                break
            fresh = rem[best]
            dying = [l for l in live if best in l]
            live = [l for l in live if best not in l]
            for l in dying:
                for r in l:
                    rem[r] -= 1
            assert rem[best] == 0 and len(dying) == fresh
            left -= fresh
            picks.append((q, best, len(picks), common[best], fresh, left))
        out.append((picks, matched, n_cand, sum(p[4] for p in picks)))
    return out


def fast(refs, queries, min_new=1, max_picks=0):
    return from_lists(posting_lists(refs), len(refs), queries, min_new, max_picks)


def singled_out(refs, queries, result, min_new=1, max_picks=0):
    """what singles the result out, checked pick by pick by brute force over the sets; raises AssertionError"""
    R = [set(int(h) for h in r) for r in refs]
    indexed = set().union(*R) if R else set()
    for q, (picks, matched, n_cand, covered) in enumerate(result):
        S = set(int(h) for h in queries[q])
        M = S & indexed
        assert matched == len(M) and n_cand == sum(len(S & r) >= min_new for r in R)
        seen = set()
        for t, (qq, r, rank, common, fresh, left) in enumerate(picks):
            assert qq == q and rank == t and r not in seen and common == len(S & R[r])
            rems = [len(M & R[x]) if x not in seen else -1 for x in range(len(R))]
            assert fresh == max(rems) >= min_new                    # the brute-force maximum of the remaining intersections
            assert r == rems.index(max(rems))                       # ties go to the smaller index
            M = M - R[r]
            seen.add(r)
            assert left == len(M)                                   # left telescopes:
            assert left == (picks[t - 1][5] if t else matched) - fresh
        assert covered == sum(p[4] for p in picks) == matched - len(M)
        assert not max_picks or len(picks) <= max_picks
        stopped_by_limit = max_picks and len(picks) == max_picks
        rest = [len(M & R[x]) for x in range(len(R)) if x not in seen]
        assert stopped_by_limit or not rest or max(rest) < min_new   # nothing worth a pick is left
        if min_new == 1 and not max_picks:
            assert covered == matched


def as_arrays(result, refs, queries, rows=None):
    """(off, picks as a list of PICK_FIELDS tuples, matched, n_cand, covered) over the selected rows, unselected rows empty and zero"""
    n = len(queries)
    rows = range(n) if rows is None else rows
    sel = set(rows)
    off, picks = [0], []
    matched, n_cand, covered = [0] * n, [0] * n, [0] * n
    for q in range(n):
        if q in sel:
            p, matched[q], n_cand[q], covered[q] = result[q]
            picks += [t + (len(set(int(h) for h in refs[t[1]])), len(set(int(h) for h in queries[q]))) for t in p]
        off.append(len(picks))
    return off, picks, matched, n_cand, covered


def pick_tuples(picks):
    """a GATHER_PICK_DTYPE array as a list of PICK_FIELDS tuples"""
    return [tuple(int(p[f]) for f in PICK_FIELDS) for p in picks]


def parts_of(h, off):
    return [np.asarray(h[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
