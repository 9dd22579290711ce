"""What the suites of the self join's consumers share (test_gpu_cluster, test_gpu_forest, test_gpu_greedy, test_gpu_knn,
test_gpu_dbscan, test_gpu_mreach, test_gpu_medoid, and test_gpu_selfjoin_refusals for all seven calls): the oracle's side of a collection, the device's index of
it, and the collections that put a call at the stage's edges.  Everything here is built from fixed seeds, the named collections once per session, and nothing a test gets from here is changed by it."""
import os

import numpy as np

from conftest import ROOT
from oracle import oracle as ok
from rabbitkssd_amd import synth

TOOL = os.path.join(ROOT, "rabbitkssd_amd", "rabbit_kssd")
KMER = 20


def csr(parts, dtype=np.uint32):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return (np.concatenate(parts).astype(dtype) if len(parts) else np.zeros(0, dtype=dtype)), off


def permuted(parts, seed, keep_last=0):
    """the sketches in a fixed random caller order (the last keep_last stay where they are)"""
    n = len(parts)
    order = np.concatenate([np.random.default_rng(seed).permutation(n - keep_last), np.arange(n - keep_last, n)]).astype(np.int64)
    return [parts[i] for i in order]


def labels_of(pairs, n):
    """labels[i] = the smallest member of i's component of the graph with these edges"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.uint32)


class Oracle:
    """the oracle's index of one collection, built once; its hit list of a threshold (cached, read-only) and the single-linkage
    labels that list gives"""
    def __init__(self, h, off, bits, wide=False):
        self.h, self.off, self.bits, self.wide = h, off, bits, wide
        self.n = len(off) - 1
        self.sizes = np.diff(off).astype(np.uint32)
        self.built = ok.index_build64(h, off) if wide else ok.index_build32(h, off, bits)
        self._hits = {}

    def hits(self, metric, D, kmer=KMER):
        key = (metric, D, kmer)
        if key not in self._hits:
            if self.wide:
                uhash, ucount, postings = self.built
                got = ok.index_dist64(uhash, ucount, postings, self.sizes, self.h, self.off, 1, metric, kmer, D, threads=4)[0]
            else:
                postings, counts = self.built
                got = ok.index_dist32(counts, self.bits, postings, self.sizes, self.h, self.off, 1, metric, kmer, D, threads=4)[0]
            got.setflags(write=False)
            self._hits[key] = got
        return self._hits[key]

    def labels(self, metric, D, kmer=KMER):
        hits = self.hits(metric, D, kmer)
        return labels_of(zip(hits["row"].tolist(), hits["col"].tolist()), self.n), len(hits)


def device_index(ctx, h, off, bits, wide=False):
    sk = ctx.sketches_from_host64(h, off) if wide else ctx.sketches_from_host(h, off)
    return ctx.index_build(sk, bits)


# ---- one ratio from different counts --------------------------------------------------------------------------------------
def tie_collection(seed):
    """Six triangles, one per assignment of the roles to ascending caller indices: A and B of 50 hashes share 25, C of 30 hashes
    shares 20 with each (10 of them with both) -- jaccard 25/75 = 20/60 = 20/60 -- and six pairs at 26/75 (50 and 51 hashes)."""
    import itertools
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 24, size=4000))
    rng.shuffle(pool)
    take = iter(range(0, len(pool), 1)).__next__

    def fresh(k):
        return np.array([pool[take()] for _ in range(k)], dtype=np.uint32)
    parts = []
    for roles in itertools.permutations(range(3)):
        abc, ab, ac, bc, a_own, b_own = fresh(10), fresh(15), fresh(10), fresh(10), fresh(15), fresh(15)
        tri = [np.concatenate([abc, ab, ac, a_own]), np.concatenate([abc, ab, bc, b_own]), np.concatenate([abc, ac, bc])]
        parts += [np.sort(tri[r]) for r in roles]
        both, p_own, q_own = fresh(26), fresh(24), fresh(25)
        parts += [np.sort(np.concatenate([both, p_own])), np.sort(np.concatenate([both, q_own]))]
    return csr(parts)


def trio(seed, sizes, shares, roles):
    """Three sketches by role: two representatives of sizes[0] and sizes[1] hashes that share shares[0] and shares[1] hashes with
    the member of sizes[2] -- and with each other only what the member forces (shares[0] + shares[1] - sizes[2]).  roles[k] = the
    role at caller index k."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 24, size=600))
    rng.shuffle(pool)
    member = pool[:sizes[2]]
    both = shares[0] + shares[1] - sizes[2]
    assert 0 <= both <= min(shares)
    rest = pool[sizes[2]:]
    a = np.concatenate([member[:shares[0]], rest[:sizes[0] - shares[0]]])
    b = np.concatenate([member[shares[0] - both: shares[0] - both + shares[1]], rest[200: 200 + sizes[1] - shares[1]]])
    made = [np.sort(a), np.sort(b), np.sort(member)]
    assert [len(np.unique(p)) for p in made] == list(sizes)
    return csr([made[r] for r in roles])


# ---- a bridge between two cliques -----------------------------------------------------------------------------------------
def bridge_collection(clique, seed):
    """two cliques of identical sketches (A: 100 hashes, B: 100 others); a keeps 70 of A's hashes, b 70 of B's, and the two share 30
    others: a-A and b-B at d = -ln(0.7)/20 = 0.0178, a-b at -ln(0.3)/20 = 0.0602 under both metrics, every other pair across the
    cliques at 1.0.  a and b are the LAST two genomes; the rest in a fixed random order."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 24, size=400))
    rng.shuffle(pool)
    A, B, X = np.sort(pool[:100]), np.sort(pool[100:200]), pool[200:230]
    a = np.sort(np.concatenate([A[:70], X]))
    b = np.sort(np.concatenate([B[:70], X]))
    return csr(permuted([A] * (clique - 1) + [B] * (clique - 1), seed + 1) + [a, b])


# ---- overflows ------------------------------------------------------------------------------------------------------------
def identical(count, seed, others=0):
    """`count` copies of one sketch of 100 hashes, then `others` unrelated sketches of 100"""
    rng = np.random.default_rng(seed)
    one = np.unique(rng.integers(0, 1 << 24, size=130))[:100]
    return [one] * count + [np.unique(rng.integers(0, 1 << 24, size=130))[:100] for _ in range(others)]


def hit_overflow_collection():
    """400 copies of one sketch (79,800 pairs at distance 0: more than the first hit capacity) and three unrelated sketches"""
    return csr(permuted(identical(400, 4, others=3), 14))


def borderline_overflow_collection():
    """300 pairs that share 80 of their 100 hashes and nothing with anyone else: 300 records on one threshold"""
    rng = np.random.default_rng(6)
    pool = np.unique(rng.integers(0, 1 << 24, size=300 * 130))
    rng.shuffle(pool)
    parts = []
    for p in range(300):   # a pair shares 80 of 100
        mine = pool[120 * p: 120 * p + 120]
        parts += [np.sort(mine[:100]), np.sort(mine[20:120])]
    return csr(permuted(parts, 16))


def both_overflows_collection():
    """400 copies of one sketch of 100 hashes (79,800 pairs at distance 0: more than the first hit capacity of 65,536) and 10 pairs
    that share 80 of their 100 hashes, in a fixed random caller order; shared with the cluster and the greedy suites"""
    rng = np.random.default_rng(21)
    pool = np.unique(rng.integers(0, 1 << 24, size=2000))
    rng.shuffle(pool)
    assert len(pool) >= 100 + 10 * 120
    parts = [np.sort(pool[:100])] * 400
    for p in range(10):
        mine = pool[100 + 120 * p: 220 + 120 * p]
        parts += [np.sort(mine[:100]), np.sort(mine[20:120])]
    return csr(permuted(parts, 17))


def both_overflows_thresholds():
    """(D, the oracle's hits, borderline records kept) one ulp above the distance of the ten pairs, and on it (strict <)"""
    _, d0 = ok.distance(80, 100, 100, 0, KMER)
    return ((float(np.nextafter(d0, 1.0)), 79810, 10), (d0, 79800, 0))


# ---- every kernel of the join, 36-bit hashes ------------------------------------------------------------------------------
_collections = {}


def collection(which):
    """(names, h, off, bits, wide, Oracle) of the named collection, built once per session and never changed"""
    if which not in _collections:
        wide, bits = False, 24
        if which == "tiles":     # more than 4,000 genomes: tile records come with the build
            names, h, off = synth.clade_sketches(4200, 120, 24, strains_per_clade=10, seed=31, tiny=20)
        elif which == "near":    # below 4,000 genomes, clades inside the window: the near-window kernel
            names, h, off = synth.clade_sketches(1200, 120, 24, strains_per_clade=10, seed=32)
        elif which == "repeat":  # one sketch lists a hash twice: no sets, rk_dist_kernel
            names, h, off = synth.clade_sketches(64, 200, 24, strains_per_clade=10, seed=33)
            h = np.concatenate([h[:1], h])
            off = off.copy()
            off[1:] += np.uint64(1)
        elif which == "wide":    # 36-bit hashes, the 64-bit layout
            names, h, off = synth.clade_sketches(1500, 150, 36, kmer_size=24, seed=15, wide=True)
            wide, bits = True, 36
        else:
            raise KeyError(which)
        if which != "repeat":
            names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=len(names)))
        _collections[which] = (names, h, off, bits, wide, Oracle(h, off, bits, wide))
    return _collections[which]
