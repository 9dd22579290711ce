"""Reference of the medoid tests: the rule of include/rabbitkssd.h (medoids and census of a clustering) from a hit list with Python
integers and exact rational ratios, and a checker of the properties that single its result out, written independently (integer
cross-multiplication, every record of a cluster looked at, no per-genome shortcut).  Imports nothing of the package under test.

A hit is (row, col, common, size0, size1) with row < col, one per pair.  labels[v] < n names v's cluster, NONE leaves v unlabelled.  A hit
is INSIDE iff its two labels are equal and not NONE, else LEAVING for both ends.  q = floor(common * 2^32 / u), u = size0 + size1 - common
for metric 0, min(size0, size1) for metric 1.  Per genome: in_deg, out_deg, central = the sum of q over its inside hits, far_in = its
inside hit of the smallest ratio, near_out = its leaving hit of the largest ratio, ties to the smaller neighbour.  Per non-empty cluster,
by ascending label: size, in_edges, medoid (the largest central, ties to the smaller index), weakest_in (over the members' far_in the
smallest ratio, ties to the smaller (row, col)), nearest_out (over the members' near_out the largest ratio, ties to the smaller (row, col)).

    python tests/_medoid_ref.py [max_n]     the reference against the checker on EVERY graph of up to max_n (default 5) vertices under
                                            every assignment of labels, NONE included; the suite runs a fixed part of that"""
import itertools
from fractions import Fraction

NONE = 0xFFFFFFFF


def terms(hit, metric):
    _, _, common, size0, size1 = hit[:5]
    return common, (size0 + size1 - common if metric == 0 else min(size0, size1))


def ratio(hit, metric):
    c, u = terms(hit, metric)
    assert 0 < c <= u
    return Fraction(c, u)


def q_of(hit, metric):
    c, u = terms(hit, metric)
    return (c << 32) // u


def other(hit, v):
    return hit[1] if hit[0] == v else hit[0]


def inside(hit, labels):
    return labels[hit[0]] == labels[hit[1]] != NONE


def genomes(hits, n, labels, metric):
    """(in_deg, out_deg, central, far_in, near_out): lists of n; the last two hold hits or None"""
    hits = [tuple(int(x) for x in h) for h in hits]
    assert len(labels) == n and all(l == NONE or 0 <= l < n for l in labels)
    assert len({h[:2] for h in hits}) == len(hits) and all(h[0] < h[1] < n for h in hits)
    ins = [[] for _ in range(n)]
    outs = [[] for _ in range(n)]
    for h in hits:
        for v in h[:2]:
            (ins if inside(h, labels) else outs)[v].append(h)
    in_deg = [len(x) for x in ins]
    out_deg = [len(x) for x in outs]
    central = [sum(q_of(h, metric) for h in x) for x in ins]
    far_in = [min(x, key=lambda h: (ratio(h, metric), other(h, v))) if x else None for v, x in enumerate(ins)]
    near_out = [min(x, key=lambda h: (-ratio(h, metric), other(h, v))) if x else None for v, x in enumerate(outs)]
    return in_deg, out_deg, central, far_in, near_out


def pick(labels, g, metric):
    """the clusters by ascending label: dicts of label, size, medoid, in_edges, central, weakest_in, nearest_out (hits or None)"""
    in_deg, out_deg, central, far_in, near_out = g
    out = []
    for l in sorted({x for x in labels if x != NONE}):
        members = [v for v in range(len(labels)) if labels[v] == l]
        medoid = min(members, key=lambda v: (-central[v], v))
        far = [far_in[v] for v in members if far_in[v] is not None]
        near = [near_out[v] for v in members if near_out[v] is not None]
        out.append({"label": l, "size": len(members), "medoid": medoid, "in_edges": sum(in_deg[v] for v in members) // 2, "central": central[medoid],
                    "weakest_in": min(far, key=lambda h: (ratio(h, metric), h[0], h[1])) if far else None,
                    "nearest_out": min(near, key=lambda h: (-ratio(h, metric), h[0], h[1])) if near else None})
    return out


def merge(a, b, metric):
    """the fold of the results of two disjoint hit lists"""
    n = len(a[0])
    far, near = [], []
    for v in range(n):
        x = [h for h in (a[3][v], b[3][v]) if h is not None]
        far.append(min(x, key=lambda h: (ratio(h, metric), other(h, v))) if x else None)
        x = [h for h in (a[4][v], b[4][v]) if h is not None]
        near.append(min(x, key=lambda h: (-ratio(h, metric), other(h, v))) if x else None)
    return [p + r for p, r in zip(a[0], b[0])], [p + r for p, r in zip(a[1], b[1])], [p + r for p, r in zip(a[2], b[2])], far, near


# ---- the checker: integers only, every record looked at --------------------------------------------------------------------
def cross(a, b, metric):
    """the sign of ratio(a) - ratio(b)"""
    (ca, ua), (cb, ub) = terms(a, metric), terms(b, metric)
    return (ca * ub > cb * ua) - (ca * ub < cb * ua)


def check_properties(hits, n, labels, metric, g, clusters):
    hits = [tuple(int(x) for x in h) for h in hits]
    in_deg, out_deg, central, far_in, near_out = g
    assert all(len(x) == n for x in g)
    same = {h: labels[h[0]] != NONE and labels[h[0]] == labels[h[1]] for h in hits}
    for v in range(n):
        mine_in = [h for h in hits if v in h[:2] and same[h]]
        mine_out = [h for h in hits if v in h[:2] and not same[h]]
        assert in_deg[v] == len(mine_in) and out_deg[v] == len(mine_out), "degrees of %d" % v
        total = 0
        for h in mine_in:
            c, u = terms(h, metric)
            total += c * 2 ** 32 // u
        assert central[v] == total < 2 ** 63, "central of %d" % v
        assert labels[v] != NONE or not mine_in
        for mine, best, sign, what in ((mine_in, far_in[v], 1, "far_in"), (mine_out, near_out[v], -1, "near_out")):
            if not mine:
                assert best is None, "%s of %d" % (what, v)
                continue
            assert best in mine, "%s of %d is not one of its records" % (what, v)
            for h in mine:
                if h != best:
                    s = sign * cross(best, h, metric)
                    assert s < 0 or (s == 0 and other(best, v) < other(h, v)), "%s of %d: %r beats %r" % (what, v, h, best)
    used = sorted({l for l in labels if l != NONE})
    assert [c["label"] for c in clusters] == used
    for c in clusters:
        l = c["label"]
        members = [v for v in range(n) if labels[v] == l]
        assert c["size"] == len(members) > 0
        all_in = [h for h in hits if labels[h[0]] == l and labels[h[1]] == l]
        all_out = [h for h in hits if (labels[h[0]] == l) != (labels[h[1]] == l)]
        assert c["in_edges"] == len(all_in)
        m = c["medoid"]
        assert m in members and c["central"] == central[m]
        for v in members:
            assert central[v] < central[m] or (central[v] == central[m] and v >= m), "medoid of cluster %d" % l
        for every, best, sign, what in ((all_in, c["weakest_in"], 1, "weakest_in"), (all_out, c["nearest_out"], -1, "nearest_out")):
            if not every:
                assert best is None, "%s of cluster %d" % (what, l)
                continue
            assert best in every, "%s of cluster %d is not one of its records" % (what, l)
            for h in every:
                if h != best:
                    s = sign * cross(best, h, metric)
                    assert s < 0 or (s == 0 and best[:2] < h[:2]), "%s of cluster %d: %r beats %r" % (what, l, h, best)


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
    """the reference against the checker on the cases first, first + stride, ... of the (graphs over n vertices) x (assignments of a
    label below n or NONE to every vertex), the metric alternating; returns (cases, genomes whose far_in or near_out a tie decided,
    clusters whose medoid is not the smallest member)"""
    values = list(range(n)) + [NONE]
    cases = ties = moved = 0
    n_graphs = 1 << (n * (n - 1) // 2)
    for case in range(first, n_graphs * len(values) ** n, stride):
        mask, code = case % n_graphs, case // n_graphs
        labels = []
        for _ in range(n):
            labels.append(values[code % len(values)])
            code //= len(values)
        hits = graph_of(n, mask)
        metric = mask & 1
        g = genomes(hits, n, labels, metric)
        clusters = pick(labels, g, metric)
        check_properties(hits, n, labels, metric, g, clusters)
        for v in range(n):
            for best, group in ((g[3][v], True), (g[4][v], False)):
                if best is not None:
                    ties += sum(v in h[:2] and inside(h, labels) == group and cross(h, best, metric) == 0 for h in hits) > 1
        moved += sum(c["medoid"] != min(v for v in range(n) if labels[v] == c["label"]) for c in clusters)
        cases += 1
    return cases, ties, moved


def render(names, labels, g, clusters, dist_of):
    """(out, census): the two texts of `rabbit_kssd medoid`; dist_of[(row, col)] = the distance of a pair as alldist prints it"""
    in_deg, out_deg, central, far_in, near_out = g
    n = len(names)

    def pair(h):
        return "-\t-\t-" if h is None else "%s\t%s\t%f" % (names[h[0]], names[h[1]], dist_of[h[:2]])

    def line(number, size, role, v):
        mean = central[v] / 4294967296.0 / (size - 1) if size > 1 else 0.0
        h = near_out[v]
        near = "-\t-" if h is None else "%s\t%f" % (names[other(h, v)], dist_of[h[:2]])
        return "%d\t%d\t%s\t%s\t%d\t%d\t%.6f\t%s\n" % (number, size, role, names[v], in_deg[v], out_deg[v], mean, near)
    out = census = ""
    for k, c in enumerate(clusters):
        out += line(k + 1, c["size"], "medoid", c["medoid"])
        for v in range(n):
            if labels[v] == c["label"] and v != c["medoid"]:
                out += line(k + 1, c["size"], "member", v)
        census += "%d\t%d\t%s\t%d\t%d\t%s\t%s\n" % (k + 1, c["size"], names[c["medoid"]], c["in_edges"], c["size"] * (c["size"] - 1) // 2,
                                                  pair(c["weakest_in"]), pair(c["nearest_out"]))
    for v in range(n):
        if labels[v] == NONE:
            out += line(0, 0, "none", v)
    return out, census


def hit_tuples(rec):
    """a structured array with the fields of rk_hit as a list of hits"""
    return list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["common"].tolist(), rec["size0"].tolist(), rec["size1"].tolist()))


if __name__ == "__main__":
    import sys
    for size in range(1, (int(sys.argv[1]) if len(sys.argv) > 1 else 5) + 1):
        print("%d vertices: %d cases, %d extremes decided by a tie, %d medoids that are not the smallest member" % ((size,) + exhaustive(size)), flush=True)
