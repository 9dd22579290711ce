"""Reference of the placement tests: the rule of include/rabbitkssd.h (placement of query genomes into a labelled collection) from a hit
list with Python integers and exact rational ratios (group by row, sort), and a checker of the properties that single its result out,
written independently (integer cross-multiplication, every record of a query looked at).  Imports nothing of the package under test.

A hit is (row, col, common, size0, size1): row a query below n_query, col a reference below n_ref, one per pair.  labels[r] < n_ref names
reference r's cluster, NONE leaves r unlabelled.  u = size0 + size1 - common for metric 0, min(size0, size1) for metric 1.  Per query:
n_within (its hits), n_labelled (those to a labelled reference), nearest (its hit to a labelled reference of the largest ratio, ties to
the smaller reference), label (that reference's label, NONE without one: novel), n_same (its hits to references of that label),
runner_up (its nearest hit, same order, to a reference labelled otherwise).

    python tests/_assign_ref.py [max_ref]    the reference against the checker on EVERY bipartite hit pattern of up to 2 queries x
                                             max_ref (default 4) references under every labelling over {0, 1, NONE}; the suite runs a
                                             fixed part of that"""
from fractions import Fraction

NONE = 0xFFFFFFFF


def terms(hit, metric):
    _, _, common, size0, size1 = hit[:5]
    return common, (size0 + size1 - common if metric == 0 else min(size0, size1))


def ratio(hit, metric):
    c, u = terms(hit, metric)
    assert 0 < c <= u
    return Fraction(c, u)


def assign(hits, n_query, n_ref, labels, metric):
    """(label, n_within, n_labelled, n_same, nearest, runner_up): lists of n_query; the last two hold hits or None"""
    hits = [tuple(int(x) for x in h) for h in hits]
    assert len(labels) == n_ref and all(l == NONE or 0 <= l < n_ref for l in labels)
    assert len({h[:2] for h in hits}) == len(hits) and all(h[0] < n_query and h[1] < n_ref for h in hits)
    rows = [[] for _ in range(n_query)]
    for h in hits:
        rows[h[0]].append(h)
    label, n_within, n_labelled, n_same, nearest, runner_up = [], [], [], [], [], []
    for mine in rows:
        mine = sorted(mine, key=lambda h: (-ratio(h, metric), h[1]))
        anchored = [h for h in mine if labels[h[1]] != NONE]
        l = labels[anchored[0][1]] if anchored else NONE
        others = [h for h in anchored if labels[h[1]] != l]
        label.append(l)
        n_within.append(len(mine))
        n_labelled.append(len(anchored))
        n_same.append(len(anchored) - len(others))
        nearest.append(anchored[0] if anchored else None)
        runner_up.append(others[0] if others else None)
    return label, n_within, n_labelled, n_same, nearest, runner_up


# ---- the checker: integers only, every record looked at --------------------------------------------------------------------
def cross(a, b, metric):
    """the sign of ratio(a) - ratio(b)"""
    (ca, ua), (cb, ub) = terms(a, metric), terms(b, metric)
    return (ca * ub > cb * ua) - (ca * ub < cb * ua)


def check_properties(hits, n_query, n_ref, labels, metric, result):
    hits = [tuple(int(x) for x in h) for h in hits]
    label, n_within, n_labelled, n_same, nearest, runner_up = result
    assert all(len(x) == n_query for x in result)
    for q in range(n_query):
        mine = [h for h in hits if h[0] == q]
        assert n_within[q] == len(mine), "n_within of %d" % q
        assert n_labelled[q] == sum(labels[h[1]] != NONE for h in mine), "n_labelled of %d" % q
        best = nearest[q]
        if not n_labelled[q]:
            assert best is None and runner_up[q] is None and label[q] == NONE and n_same[q] == 0, "novel query %d" % q
            continue
        assert best in mine and labels[best[1]] != NONE and label[q] == labels[best[1]], "nearest of %d" % q
        for h in mine:
            if h != best and labels[h[1]] != NONE:
                s = cross(h, best, metric)
                assert s < 0 or (s == 0 and best[1] < h[1]), "nearest of %d: %r beats %r" % (q, h, best)
        assert n_same[q] == sum(labels[h[1]] == label[q] for h in mine) >= 1, "n_same of %d" % q
        rest = [h for h in mine if labels[h[1]] not in (NONE, label[q])]
        second = runner_up[q]
        if not rest:
            assert second is None, "runner_up of %d" % q
            continue
        assert second in rest, "runner_up of %d is not a record of another label" % q
        for h in rest:
            if h != second:
                s = cross(h, second, metric)
                assert s < 0 or (s == 0 and second[1] < h[1]), "runner_up of %d: %r beats %r" % (q, h, second)


# ---- every bipartite pattern of a few queries and references ---------------------------------------------------------------
# (common, size0, size1): 20/60 and 25/75 tie under metric 0 (u = size0 + size1 - common), 20/40 and 25/50 under metric 1 (u = min)
TRIPLES = [(20, 40, 40), (25, 50, 50), (40, 60, 60), (60, 70, 70)]
VALUES = (0, 1, NONE)


def pattern_of(n_query, n_ref, mask):
    """the hits whose (query, reference) cells are the set bits of mask; the weights a fixed function of (mask, cell), from TRIPLES"""
    hits = []
    for k in range(n_query * n_ref):
        if mask >> k & 1:
            hits.append((k // n_ref, k % n_ref) + TRIPLES[(mask * 2654435761 + k * 40503 >> 5) % len(TRIPLES)])
    return hits


def exhaustive(n_query, n_ref, stride=1, first=0):
    """the reference against the checker on the cases first, first + stride, ... of the (patterns of n_query x n_ref cells) x (labellings
    of the references over {0, 1, NONE}; 1 only from two references on), the metric alternating; returns (cases, queries whose nearest or
    runner-up a tie decided, queries with a runner-up, novel queries that have records)"""
    values = [v for v in VALUES if v == NONE or v < n_ref]
    n_masks = 1 << (n_query * n_ref)
    cases = ties = seconds = unanchored = 0
    for case in range(first, n_masks * len(values) ** n_ref, stride):
        mask, code = case % n_masks, case // n_masks
        labels = []
        for _ in range(n_ref):
            labels.append(values[code % len(values)])
            code //= len(values)
        hits = pattern_of(n_query, n_ref, mask)
        metric = mask & 1
        result = assign(hits, n_query, n_ref, labels, metric)
        check_properties(hits, n_query, n_ref, labels, metric, result)
        for q in range(n_query):
            for best, same in ((result[4][q], True), (result[5][q], False)):
                if best is not None:
                    ties += sum(h[0] == q and labels[h[1]] != NONE and (labels[h[1]] == result[0][q]) == same and cross(h, best, metric) == 0 for h in hits) > 1
            seconds += result[5][q] is not None
            unanchored += result[0][q] == NONE and result[1][q] > 0
        cases += 1
    return cases, ties, seconds, unanchored


def render(query_names, ref_names, labels, result, values):
    """the text of `rabbit_kssd assign -o`; values[(row, col)] = (jorc, dist) of a pair as dist prints them"""
    label, n_within, n_labelled, n_same, nearest, runner_up = result
    out = ""
    for q, name in enumerate(query_names):
        h, s = nearest[q], runner_up[q]
        if h is None:
            out += "%s\t-\t-\t-\t-\t-\t%d\t%d\t%d\t-\t-\n" % (name, n_same[q], n_labelled[q], n_within[q])
            continue
        second = "-\t-" if s is None else "%s\t%f" % (ref_names[labels[s[1]]], values[s[:2]][1])
        out += "%s\t%s\t%s\t%d|%d|%d\t%f\t%f\t%d\t%d\t%d\t%s\n" % ((name, ref_names[label[q]], ref_names[h[1]]) + h[2:5] + tuple(values[h[:2]]) +
                                                                  (n_same[q], n_labelled[q], n_within[q], second))
    return out


def novel(query_names, result):
    """the text of `rabbit_kssd assign --novel`"""
    return "".join("%s\n" % name for q, name in enumerate(query_names) if result[0][q] == NONE)


def hit_tuples(rec):
    """a structured array with the fields of rk_hit as a list of hits"""
    return list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["common"].tolist(), rec["size0"].tolist(), rec["size1"].tolist()))


def record_tuples(rec):
    """a record array of the library (row = col = NONE: absent) as a list of hits or None"""
    return [None if h[0] == NONE else h for h in hit_tuples(rec)]


if __name__ == "__main__":
    import sys
    for n_q in (1, 2):
        for n_r in range(1, (int(sys.argv[1]) if len(sys.argv) > 1 else 4) + 1):
            print("%d x %d: %d cases, %d records decided by a tie, %d runner-ups, %d novel queries with records" % ((n_q, n_r) + exhaustive(n_q, n_r)),
                  flush=True)
