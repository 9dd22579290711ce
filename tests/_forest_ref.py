"""Reference of the forest tests: Kruskal over a hit list with exact rational weights.  Imports nothing of the package under test.

A hit is (row, col, common, size0, size1) with row < col.  Order of edges (include/rabbitkssd.h): the ratio common / u descending
-- u = size0 + size1 - common for metric 0, min(size0, size1) for metric 1 --, then row ascending, then col ascending.  The order
is strict, so the minimum spanning forest is unique: the edges Kruskal accepts in this order."""
import math
from fractions import Fraction


def ratio(hit, metric):
    _, _, common, size0, size1 = hit
    return Fraction(common, size0 + size1 - common if metric == 0 else min(size0, size1))


def edge_key(hit, metric):
    return (-ratio(hit, metric), hit[0], hit[1])


def distance(hit, metric, kmer_size):
    """(jorc, dist) with the expression of the reference (src/dist.cpp:218-231) in doubles: math.log is the C library's log"""
    _, _, common, size0, size1 = hit
    denom = size0 + size1 - common if metric == 0 else min(size0, size1)
    j = 0.0 if size0 == 0 or size1 == 0 else float(common) / float(denom)
    if j == 1.0:
        return j, 0.0
    if j == 0.0:
        return j, 1.0
    return j, (-1.0 / float(kmer_size)) * math.log((2 * j) / (1.0 + j) if metric == 0 else j)


class UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a, b):
        """False when a and b were connected already"""
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)
        return a != b

    def labels(self):
        """labels[i] = the smallest member of i's component"""
        return [self.find(i) for i in range(len(self.parent))]


def kruskal(hits, n, metric):
    """the minimum spanning forest of the hits over n genomes, as a list of hits in forest order"""
    uf = UnionFind(n)
    return [h for h in sorted((tuple(int(x) for x in h) for h in hits), key=lambda h: edge_key(h, metric)) if uf.union(h[0], h[1])]


def components(pairs, n):
    uf = UnionFind(n)
    for a, b in pairs:
        uf.union(a, b)
    return uf.labels()


def hit_tuples(rec):
    """a structured array with the fields of rk_hit as a list of hits"""
    return list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["common"].tolist(), rec["size0"].tolist(), rec["size1"].tolist()))
