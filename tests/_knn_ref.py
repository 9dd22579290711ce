"""Reference of the kNN tests: per genome the first k incident records of a hit list with exact rational ratios, a checker of the
properties that single that result out (written independently: integer cross-multiplication, no sort), and a step-by-step model of
the selection wave of rk_knn.hip.  Imports nothing of the package under test.

A hit is (row, col, common, size0, size1) with row < col, one per pair.  A record is incident to its row and to its col; the neighbour
of genome v in it is the other endpoint.  Order of v's records: the ratio common / u descending -- u = size0 + size1 - common for
metric 0, min(size0, size1) for metric 1 --, then the neighbour's index ascending; a record without a ratio (u <= 0 or common < 0)
behind every record that has one (include/rabbitkssd.h, k nearest neighbours)."""
from fractions import Fraction

DEAD = (1 << 64) - 1
LANES = 64


def terms(hit, metric):
    _, _, common, size0, size1 = hit
    return common, (size0 + size1 - common if metric == 0 else min(size0, size1))


def other(hit, v):
    assert v in (hit[0], hit[1])
    return hit[1] if hit[0] == v else hit[0]


def place(hit, v, metric):
    """the sort key of a record in the list of genome v"""
    c, u = terms(hit, metric)
    if u > 0 and c >= 0:
        return (0, -Fraction(c, u), other(hit, v))
    return (1, 0, other(hit, v))


def knn(hits, n, k, metric):
    """lists[v] = the first min(k, degree(v)) records incident to v, nearest first"""
    hits = [tuple(int(x) for x in h) for h in hits]
    incident = [[] for _ in range(n)]
    for h in hits:
        assert h[0] < h[1] < n
        incident[h[0]].append(h)
        incident[h[1]].append(h)
    return [sorted(incident[v], key=lambda h: place(h, v, metric))[:k] for v in range(n)]


def offsets(lists):
    off = [0]
    for one in lists:
        off.append(off[-1] + len(one))
    return off


def flat(lists):
    return [h for one in lists for h in one]


def precedes(a, b, v, metric):
    """a comes strictly before b in the list of v: integers only"""
    (ca, ua), (cb, ub) = terms(a, metric), terms(b, metric)
    va, vb = ua > 0 and ca >= 0, ub > 0 and cb >= 0
    if va != vb:
        return va
    if va and ca * ub != cb * ua:
        return ca * ub > cb * ua
    return other(a, v) < other(b, v)


def check_properties(hits, n, k, metric, lists):
    """what singles the result out: every record of a list is incident to its genome, the list ascends strictly, holds min(k, degree)
    records, and no incident record outside it precedes its last entry"""
    hits = [tuple(int(x) for x in h) for h in hits]
    known = set(hits)
    assert len(known) == len(hits) and len(lists) == n
    for v in range(n):
        mine = [tuple(h) for h in lists[v]]
        incident = [h for h in hits if v in (h[0], h[1])]
        assert len(mine) == min(k, len(incident)), "the list of %d holds %d of %d records" % (v, len(mine), len(incident))
        for h in mine:
            assert h in known and v in (h[0], h[1]), "the list of %d holds %r" % (v, h)
        for a, b in zip(mine, mine[1:]):
            assert precedes(a, b, v, metric), "the list of %d does not ascend strictly at %r" % (v, b)
        inside = set(mine)
        for h in incident:
            if h not in inside:
                assert not precedes(h, mine[-1], v, metric), "genome %d has a nearer neighbour %d" % (v, other(h, v))


# ---- the device's view ------------------------------------------------------------------------------------------------------
def entry(hit, v, e, metric):
    """the 16-byte entry of record number e in the segment of genome v: (~floor(common * 2^62 / u), neighbour << 32 | e)"""
    c, u = terms(hit, metric)
    assert 0 < c <= u < (1 << 31) and e < (1 << 31)
    return (DEAD - ((c << 62) // u), (other(hit, v) << 32) | e)


def select_model(entries, k):
    """k_knn_select, one wave over one segment: lane l holds the l-th best entry so far or (DEAD, DEAD); the segment streams in chunks of
    64; a ballot keeps the candidates that beat the current k-th (lane k - 1); each survivor, lowest lane first, is broadcast, tested
    again against the k-th, ranked by the number of lanes that precede it and inserted with one shuffle up.  Returns the lanes that are
    written out: the first min(k, len(entries))."""
    assert 1 <= k <= LANES
    dead = (DEAD, DEAD)
    best = [dead] * LANES
    for at in range(0, len(entries), LANES):
        chunk = list(entries[at: at + LANES])
        chunk += [dead] * (LANES - len(chunk))
        kth = best[k - 1]
        mask = [chunk[lane] < kth for lane in range(LANES)]
        for src in range(LANES):
            if not mask[src]:
                continue
            s = chunk[src]
            if not s < best[k - 1]:
                continue
            rank = sum(b < s for b in best)
            assert rank < k
            up = [best[0]] + best[:-1]   # (a shuffle up leaves lane 0 its own value)
            for lane in range(LANES):
                if lane < k and lane >= rank:
                    best[lane] = s if lane == rank else up[lane]
    assert all(b == dead for b in best[k:])   # lanes >= k stay dead
    return best[: min(k, len(entries))]


def hit_tuples(rec):
    """a structured array with the fields of rk_hit as a list of hits"""
    return list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["common"].tolist(), rec["size0"].tolist(), rec["size1"].tolist()))
