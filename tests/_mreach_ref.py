"""Reference of the mutual-reachability tests: the rule of include/rabbitkssd.h (mutual-reachability forest) from a hit list with exact
rational ratios -- per genome a sorted adjacency, then Kruskal by (the largest of three negated ratios, row, col) --, and a checker of
the properties that single its result out, written independently (integer cross-multiplication, paths in the forest, no sort of edges).
Imports nothing of the package under test.

A hit is (row, col, common, size0, size1) with row < col, one per pair.  With k = min_pts - 1 the core record of v is the k-th of the hits
incident to v in the order (ratio common / u descending, the neighbour's index ascending) -- u = size0 + size1 - common for metric 0,
min(size0, size1) for metric 1; none when v has fewer than k hits (no edge then touches v); no record and weight 0 for k = 0.  The weight
of a hit is the largest of its own and its two endpoints' core records' weights, a weight being the negated ratio; the forest is what
Kruskal accepts in the order (weight, row, col).

    python tests/_mreach_ref.py [max_n]     the reference against the checker on EVERY labelled graph of up to max_n (default 6)
                                            vertices, at every min_pts from 1 to n + 1"""
import itertools
import random
from fractions import Fraction

NONE = 0xFFFFFFFF
NOISE = 0xFFFFFFFF


def ratio(hit, metric):
    _, _, common, size0, size1 = hit
    return Fraction(common, size0 + size1 - common if metric == 0 else min(size0, size1))


def mreach(hits, n, min_pts, metric):
    """(core, edges): core[v] = (the core record of v, the neighbour in it) or None; edges = the forest's hits in order"""
    assert min_pts >= 1
    k = min_pts - 1
    hits = [tuple(int(x) for x in h) for h in hits]
    incident = [[] for _ in range(n)]
    for h in hits:
        assert h[0] < h[1] < n
        incident[h[0]].append((-ratio(h, metric), h[1], h))
        incident[h[1]].append((-ratio(h, metric), h[0], h))
    core, core_w = [None] * n, [Fraction(-1) if k == 0 else None] * n   # (-1: below the weight of every hit, whose ratio is <= 1)
    if k:
        for v in range(n):
            if len(incident[v]) >= k:
                w, other, h = sorted(incident[v])[k - 1]
                core[v], core_w[v] = (h, other), w
    finite = [h for h in hits if core_w[h[0]] is not None and core_w[h[1]] is not None]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    edges = []
    for h in sorted(finite, key=lambda h: (max(-ratio(h, metric), core_w[h[0]], core_w[h[1]]), h[0], h[1])):
        a, b = find(h[0]), find(h[1])
        if a != b:
            parent[a] = b
            edges.append(h)
    return core, edges


def cut(edges, core, n, min_pts, metric, t_ratio):
    """labels of the forest cut where a weight links iff its ratio lies strictly ABOVE t_ratio (the distance strictly below the
    threshold of that ratio): the smallest index of each component of the genomes core at that level, NOISE elsewhere"""
    k = min_pts - 1
    is_core = [k == 0 or (core[v] is not None and ratio(core[v][0], metric) > t_ratio) for v in range(n)]
    label = [v if is_core[v] else NOISE for v in range(n)]
    for h in edges:
        if ratio(h, metric) > t_ratio and is_core[h[0]] and is_core[h[1]]:
            a, b = label[h[0]], label[h[1]]
            if a != b:
                label = [min(a, b) if l in (a, b) else l for l in label]
    return label


# ---- the checker: integers only ---------------------------------------------------------------------------------------------
def terms(hit, metric):
    _, _, common, size0, size1 = hit
    return common, (size0 + size1 - common if metric == 0 else min(size0, size1))


def heavier(a, b):
    """the weight of the ratio terms a = (c, u) lies strictly above that of b: the smaller ratio"""
    return a[0] * b[1] < b[0] * a[1]


def check_properties(hits, n, min_pts, metric, core, edges):
    """what singles the result out: the core record of v is incident to v and exactly k - 1 records incident to v come strictly before
    it (none: fewer than k are incident); the forest's edges are hits with finite weight, strictly ascending in the order, and they span
    exactly the components of the graph of the finite-weight hits; for every finite-weight hit outside the forest, every forest edge on
    the path between its ends comes before it in the order (so no exchange gives a forest that Kruskal would have preferred)"""
    k = min_pts - 1
    hits = [tuple(int(x) for x in h) for h in hits]
    edges = [tuple(int(x) for x in h) for h in edges]
    assert len(core) == n
    # the core records
    core_t = [None] * n
    for v in range(n):
        mine = [h for h in hits if v in h[:2]]
        if k == 0 or len(mine) < k:
            assert core[v] is None, "genome %d of degree %d has a core record" % (v, len(mine))
            continue
        assert core[v] is not None, "genome %d of degree %d has no core record" % (v, len(mine))
        rec, other = tuple(int(x) for x in core[v][0]), int(core[v][1])
        assert rec in mine and {v, other} == set(rec[:2]), "core record of %d" % v
        before = 0
        for h in mine:
            x = h[0] + h[1] - v
            before += heavier(terms(rec, metric), terms(h, metric)) or (not heavier(terms(h, metric), terms(rec, metric)) and x < other)
        assert before == k - 1, "%d records precede the core record of %d, k = %d" % (before, v, k)
        core_t[v] = terms(rec, metric)

    def weight(h):   # the heaviest of three ratio terms; None: infinite
        if k == 0:
            return terms(h, metric)
        if core_t[h[0]] is None or core_t[h[1]] is None:
            return None
        w = terms(h, metric)
        for c in (core_t[h[0]], core_t[h[1]]):
            if heavier(c, w):
                w = c
        return w

    def precedes(e, f):
        we, wf = weight(e), weight(f)
        if heavier(wf, we):
            return True
        return not heavier(we, wf) and e[:2] < f[:2]
    finite = [h for h in hits if weight(h) is not None]
    assert len(set(edges)) == len(edges) and all(e in finite for e in edges), "a forest edge is no finite-weight hit"
    for a, b in zip(edges, edges[1:]):
        assert precedes(a, b), "the forest is not in order at %r, %r" % (a, b)
    # spanning: the same components, and no cycle
    def components(es):
        label = list(range(n))
        for h in es:
            a, b = label[h[0]], label[h[1]]
            if a != b:
                label = [a if l == b else l for l in label]
        return [[label[x] == label[y] for y in range(n)] for x in range(n)]
    assert components(edges) == components(finite), "the forest does not span the components of the finite-weight graph"
    assert len(edges) == n - len({min(y for y in range(n) if row[y]) for row in components(edges)}), "the forest holds a cycle"
    # the cycle property
    nbrs = [[] for _ in range(n)]
    for e in edges:
        nbrs[e[0]].append((e[1], e))
        nbrs[e[1]].append((e[0], e))

    def path(a, b):
        stack = [(a, None, [])]
        while stack:
            x, came, way = stack.pop()
            if x == b:
                return way
            stack += [(y, x, way + [e]) for y, e in nbrs[x] if y != came]
        raise AssertionError("no path between %d and %d" % (a, b))
    in_forest = set(edges)
    for f in finite:
        if f not in in_forest:
            for e in path(f[0], f[1]):
                assert precedes(e, f), "forest edge %r on the path of %r comes behind it" % (e, f)


# ---- every labelled graph of a few vertices ---------------------------------------------------------------------------------
# (common, size0, size1): 20/60 and 25/75 tie under metric 0 (u = size0 + size1 - common), 20/40 and 25/50 under metric 1 (u = min)
TRIPLES = [(20, 50, 50), (40, 60, 60), (60, 70, 70), (20, 40, 40), (25, 50, 50)]


def graph_of(n, mask, rng):
    """the graph over n vertices whose pairs (in itertools.combinations order) are the set bits of mask, the counts drawn from TRIPLES"""
    return [(a, b) + TRIPLES[rng.randrange(len(TRIPLES))] for k, (a, b) in enumerate(itertools.combinations(range(n), 2)) if mask >> k & 1]


def exhaustive(n, seed=5):
    """the reference against the checker on every labelled graph over n vertices at every min_pts 1 .. n + 1, the metric alternating;
    returns (graphs, forest edges seen, of which with the weight of their predecessor, genomes without a core record)"""
    rng = random.Random(seed * 1000 + n)
    graphs = seen = tied = bare = 0
    for mask in range(1 << (n * (n - 1) // 2)):
        hits = graph_of(n, mask, rng)
        metric = mask & 1
        for min_pts in range(1, n + 2):
            core, edges = mreach(hits, n, min_pts, metric)
            check_properties(hits, n, min_pts, metric, core, edges)
            w = [max([ratio(e, metric)] + [ratio(core[v][0], metric) for v in e[:2] if core[v]], key=lambda r: -r) for e in edges]
            seen += len(edges)
            tied += sum(a == b for a, b in zip(w, w[1:]))
            bare += sum(c is None for c in core) if min_pts > 1 else 0
        graphs += 1
    return graphs, seen, tied, bare


# ---- the texts of `rabbit_kssd mreach` --------------------------------------------------------------------------------------
def render_edges(names, edges, mw):
    """-o: one alldist line per edge (the names as alldist orders them: col first), then the mutual-reachability distance.  edges: records
    with the fields of rk_hit"""
    return "".join("%s\t%s\t%d|%d|%d\t%f\t%f\t%f\n" % (names[e["col"]], names[e["row"]], e["common"], e["size0"], e["size1"], e["jorc"], e["dist"], m)
                   for e, m in zip(edges, mw))


def render_core(names, core_dist, core_nb):
    """--core: name, core distance (- when none), the neighbour's name (- when none)"""
    return "".join("%s\t%s\t%s\n" % (names[v], "-" if d == float("inf") else "%f" % d, "-" if x == NONE else names[x])
                   for v, (d, x) in enumerate(zip(core_dist, core_nb)))


def render_labels(names, labels):
    """--labels: the layout of `cluster` (cluster number, size, name; clusters by their label, members by index), clusters numbered
    from 1 and the noise last as cluster 0 of size 0"""
    n = len(names)
    size = {}
    for v in range(n):
        if labels[v] != NOISE:
            size[labels[v]] = size.get(labels[v], 0) + 1
    number = {l: i + 1 for i, l in enumerate(sorted(size))}
    order = sorted((v for v in range(n) if labels[v] != NOISE), key=lambda v: (labels[v], v)) + [v for v in range(n) if labels[v] == NOISE]
    return "".join("%d\t%d\t%s\n" % (((number[labels[v]], size[labels[v]]) if labels[v] != NOISE else (0, 0)) + (names[v],)) for v in order)


def hit_tuples(rec):
    """a structured array with the fields of rk_hit as a list of hits"""
    return list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["common"].tolist(), rec["size0"].tolist(), rec["size1"].tolist()))


if __name__ == "__main__":
    import sys
    for size in range(1, (int(sys.argv[1]) if len(sys.argv) > 1 else 6) + 1):
        print("%d vertices: %d graphs, %d forest edges, %d of them tied with their predecessor, %d genomes without a core record"
              % ((size,) + exhaustive(size)), flush=True)
