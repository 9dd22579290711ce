"""Reference of the index build's internal genome order, in numpy, written from the rule (rk_index.hip, "internal genome
order") and not from its kernels:

  * of every genome take its first min(size, 16) hashes (the sketches are ascending: its smallest), 64-bit ones folded to
    32 bits as h ^ (h >> 32);
  * owner[h] is the smallest genome that lists h among those;
  * parent[g] is the smallest owner that at least two of g's (up to) 16 hashes agree on, if that owner is below g; else g;
  * the root of g is found by following the parents; the internal order is by (root, caller's index).

order_ref returns orig[] as rk_index_order does: orig[i] = caller's index of internal genome i."""
import numpy as np

MIN_K = 16


def fold32(h):
    h = np.asarray(h)
    if h.dtype == np.uint64:
        return ((h ^ (h >> np.uint64(32))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return h.astype(np.uint32)


def parents_ref(hashes, off):
    """parent[g] of every genome (int64[N])"""
    off = np.asarray(off, dtype=np.int64)
    n = len(off) - 1
    cnt = np.minimum(np.diff(off), MIN_K)
    g_of = np.repeat(np.arange(n, dtype=np.int64), cnt)                   # genome of every signature element
    pos = np.arange(len(g_of), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    sig = fold32(np.asarray(hashes)[off[g_of] + pos]).astype(np.int64)
    # owner of a hash value: the smallest genome among those that list it
    by = np.lexsort((g_of, sig))
    first = np.ones(len(by), dtype=bool)
    first[1:] = sig[by][1:] != sig[by][:-1]
    run = np.cumsum(first) - 1
    owner_of_run = g_of[by][first]
    owner = np.empty(len(by), dtype=np.int64)
    owner[by] = owner_of_run[run]
    # the owners of a genome's hashes side by side; an unused place holds a value no owner has
    mat = np.full((n, MIN_K), -1, dtype=np.int64)
    mat[g_of, pos] = owner
    parent = np.arange(n, dtype=np.int64)
    for lo in range(0, n, 4096):                                          # (in slabs: n x 16 x 16 comparisons)
        m = mat[lo:lo + 4096]
        votes = ((m[:, :, None] == m[:, None, :]) & (m[:, None, :] >= 0)).sum(axis=2)
        g = np.arange(lo, lo + len(m), dtype=np.int64)[:, None]
        cand = np.where((votes >= 2) & (m >= 0) & (m < g), m, g)
        parent[lo:lo + len(m)] = cand.min(axis=1)
    return parent


def roots_ref(parent):
    root = np.asarray(parent, dtype=np.int64).copy()
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            return root
        root = nxt


def order_ref(hashes, off):
    """orig[i] = caller's index of internal genome i (uint32[N])"""
    n = len(off) - 1
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    root = roots_ref(parents_ref(hashes, off))
    return np.lexsort((np.arange(n), root)).astype(np.uint32)
