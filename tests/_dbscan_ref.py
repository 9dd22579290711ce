"""Reference of the DBSCAN tests: the rule of include/rabbitkssd.h (density-based clusters) from a hit list with exact rational
ratios -- adjacency sets, a breadth-first search over the core genomes --, and a checker of the properties that single its result out,
written independently (integer cross-multiplication, a transitive closure, no search).  Imports nothing of the package under test.

A hit is (row, col, common, size0, size1) with row < col, one per pair.  deg(v) = the hits incident to v; v is core iff deg(v) + 1 >=
min_pts; clusters are the components of the subgraph induced by the core genomes, labelled by their smallest core index; a non-core
genome with a core neighbour is border and takes the label of its nearest core neighbour -- the ratio common / u descending (u = size0
+ size1 - common for metric 0, min(size0, size1) for metric 1), then the neighbour's index ascending; a record without a ratio (u <= 0
or common < 0) behind every record that has one --; every other genome is noise, label = via = NOISE.

    python tests/_dbscan_ref.py [max_n]     the reference against the checker on EVERY graph of up to max_n (default 7) vertices, at
                                            every min_pts; minutes at 7 (2^21 graphs), which is why the suite runs 7 thinned out"""
import itertools
from collections import deque
from fractions import Fraction

NOISE = 0xFFFFFFFF
KIND_NOISE, KIND_BORDER, KIND_CORE = 0, 1, 2
KIND_NAMES = ("noise", "border", "core")


def terms(hit, metric):
    _, _, common, size0, size1 = hit
    return common, (size0 + size1 - common if metric == 0 else min(size0, size1))


def nearness(hit, other, metric):
    """the sort key of a record among those incident to one genome: `other` is the neighbour"""
    c, u = terms(hit, metric)
    if u > 0 and c >= 0:
        return (0, -Fraction(c, u), other)
    return (1, 0, other)


def dbscan(hits, n, min_pts, metric):
    """(labels, kind, via, degree), lists of n"""
    assert min_pts >= 1
    hits = [tuple(int(x) for x in h) for h in hits]
    nbrs = [set() for _ in range(n)]
    record = {}
    for h in hits:
        assert h[0] < h[1] < n and (h[0], h[1]) not in record
        record[(h[0], h[1])] = h
        nbrs[h[0]].add(h[1])
        nbrs[h[1]].add(h[0])
    degree = [len(s) for s in nbrs]
    core = [degree[v] + 1 >= min_pts for v in range(n)]
    labels, kind, via = [NOISE] * n, [KIND_NOISE] * n, [NOISE] * n
    for s in range(n):   # ascending: the first core genome that reaches a cluster is its smallest
        if not core[s] or labels[s] != NOISE:
            continue
        labels[s] = s
        queue = deque([s])
        while queue:
            v = queue.popleft()
            kind[v] = KIND_CORE
            for x in nbrs[v]:
                if core[x] and labels[x] == NOISE:
                    labels[x] = s
                    queue.append(x)
    for v in range(n):
        if core[v]:
            continue
        near = [x for x in nbrs[v] if core[x]]
        if near:
            via[v] = min(near, key=lambda x: nearness(record[(min(v, x), max(v, x))], x, metric))
            labels[v] = labels[via[v]]
            kind[v] = KIND_BORDER
    return labels, kind, via, degree


def nearer(a, xa, b, xb, metric):
    """record a (neighbour xa) comes strictly before record b (neighbour xb): integers only"""
    (ca, ua), (cb, ub) = terms(a, metric), terms(b, metric)
    va, vb = ua > 0 and ca >= 0, ub > 0 and cb >= 0
    if va != vb:
        return va
    if va and ca * ub != cb * ua:
        return ca * ub > cb * ua
    return xa < xb


def check_properties(hits, n, min_pts, metric, labels, kind, via, degree):
    """what singles the result out: the kind matches the degree; two core genomes share a label iff a path of core genomes joins them;
    the label is the smallest core index; a border genome's via is core, adjacent, and no adjacent core genome is nearer or equally
    near with a smaller index; noise has no core neighbour"""
    hits = [tuple(int(x) for x in h) for h in hits]
    labels, kind, via, degree = [[int(x) for x in a] for a in (labels, kind, via, degree)]
    assert len(labels) == len(kind) == len(via) == len(degree) == n
    record = {}
    for h in hits:
        record[(h[0], h[1])] = record[(h[1], h[0])] = h
    assert len(record) == 2 * len(hits)
    for v in range(n):
        assert degree[v] == sum(v in h[:2] for h in hits), "degree of %d" % v
        assert (kind[v] == KIND_CORE) == (degree[v] + 1 >= min_pts), "genome %d of degree %d is of kind %d" % (v, degree[v], kind[v])
    core = [kind[v] == KIND_CORE for v in range(n)]
    # reach[a][b]: a path of core genomes joins the core genomes a and b (Warshall)
    reach = [[a == b or (core[a] and core[b] and (a, b) in record) for b in range(n)] for a in range(n)]
    for m in range(n):
        if core[m]:
            for a in range(n):
                if reach[a][m]:
                    for b in range(n):
                        if reach[m][b]:
                            reach[a][b] = True
    for a in range(n):
        if not core[a]:
            continue
        assert via[a] == NOISE, "core genome %d has a via" % a
        assert labels[a] == min(b for b in range(n) if core[b] and reach[a][b]), "label of core genome %d" % a
        for b in range(n):
            if core[b]:
                assert (labels[a] == labels[b]) == reach[a][b], "core genomes %d and %d" % (a, b)
    for v in range(n):
        if core[v]:
            continue
        near = [x for x in range(n) if core[x] and (v, x) in record]
        if kind[v] == KIND_NOISE:
            assert not near and labels[v] == NOISE and via[v] == NOISE, "noise genome %d" % v
            continue
        assert kind[v] == KIND_BORDER and via[v] in near, "border genome %d came in through %d" % (v, via[v])
        assert labels[v] == labels[via[v]], "label of border genome %d" % v
        for x in near:
            if x != via[v]:
                assert nearer(record[(v, via[v])], via[v], record[(v, x)], x, metric), "border genome %d has a nearer core neighbour %d" % (v, x)


# ---- every graph of a few vertices ----------------------------------------------------------------------------------------
# (common, size0, size1): 20/60 and 25/75 tie under metric 0 (u = size0 + size1 - common), 20/40 and 25/50 under metric 1 (u = min)
TRIPLES = [(20, 50, 50), (40, 60, 60), (60, 70, 70), (20, 40, 40), (25, 50, 50)]


def graph_of(n, mask):
    """the graph over n vertices whose pairs (in itertools.combinations order) are the set bits of mask; the weights a fixed function
    of (mask, pair), from TRIPLES"""
    hits = []
    for k, (a, b) in enumerate(itertools.combinations(range(n), 2)):
        if mask >> k & 1:
            hits.append((a, b) + TRIPLES[(mask * 2654435761 + k * 40503 >> 7) % len(TRIPLES)])
    return hits


def exhaustive(n, stride=1, first=0):
    """the reference against the checker on the graphs first, first + stride, ... of the 2^(n (n - 1) / 2) over n vertices, at every
    min_pts 1 .. n + 1, the metric alternating; returns (graphs, border genomes seen, border genomes decided by a tie)"""
    graphs = borders = ties = 0
    for mask in range(first, 1 << (n * (n - 1) // 2), stride):
        hits = graph_of(n, mask)
        metric = mask & 1
        for min_pts in range(1, n + 2):
            labels, kind, via, degree = dbscan(hits, n, min_pts, metric)
            check_properties(hits, n, min_pts, metric, labels, kind, via, degree)
            for v in range(n):
                if kind[v] == KIND_BORDER:
                    borders += 1
                    mine = nearness(next(h for h in hits if set(h[:2]) == {v, via[v]}), 0, metric)[:2]
                    ties += sum(kind[h[0] + h[1] - v] == KIND_CORE and nearness(h, 0, metric)[:2] == mine for h in hits if v in h[:2]) > 1
        graphs += 1
    return graphs, borders, ties


def render(names, labels, kind, via, degree):
    """the text of `rabbit_kssd dbscan`: clusters in order of their label, numbered from 1, core genomes first, then border genomes,
    each by index; then the noise as cluster 0 of size 0"""
    n = len(names)
    size = {}
    for v in range(n):
        if kind[v] != KIND_NOISE:
            size[labels[v]] = size.get(labels[v], 0) + 1
    number = {l: k + 1 for k, l in enumerate(sorted(size))}
    order = sorted((v for v in range(n) if kind[v] != KIND_NOISE), key=lambda v: (labels[v], -kind[v], v)) + [v for v in range(n) if kind[v] == KIND_NOISE]
    text = ""
    for v in order:
        noise = kind[v] == KIND_NOISE
        text += "%d\t%d\t%s\t%s\t%d\t%s\n" % (0 if noise else number[labels[v]], 0 if noise else size[labels[v]], KIND_NAMES[kind[v]], names[v], degree[v],
                                              names[via[v]] if kind[v] == KIND_BORDER else "-")
    return text


def hit_tuples(rec):
    """a structured array with the fields of rk_hit as a list of hits"""
    return list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["common"].tolist(), rec["size0"].tolist(), rec["size1"].tolist()))


if __name__ == "__main__":
    import sys
    for size in range(1, (int(sys.argv[1]) if len(sys.argv) > 1 else 7) + 1):
        print("%d vertices: %d graphs, %d border genomes, %d of them decided by a tie" % ((size,) + exhaustive(size)), flush=True)
