"""The rule of rk_group_sketches / rk_group_lists in plain Python, twice and independently: from the genomes' hash sets (the definition
of include/rabbitkssd.h, word for word) and from posting lists.  Integers only.  tests/test_group_cpu.py checks the two against each
other on every small labelling; everything else is checked against them.

    sketches   a list of N iterables of hashes (a sketch may repeat a hash: it counts once)
    labels     N entries: below N names the cluster, NONE leaves the genome unlabelled
    rule       (share_num, share_den, min_count, only)
    result     (group_label, group_size, kept): the labels in use ascending, their member counts, per group its hashes ascending"""
import functools

import numpy as np

NONE = 0xFFFFFFFF
RULES = {"pan": (0, 1, 1, 0), "core": (1, 1, 1, 0), "majority": (1, 2, 1, 0), "markers": (0, 1, 1, 1), "min2": (0, 1, 2, 0)}


@functools.lru_cache(maxsize=4096)
def _groups_of(labels):
    n = len(labels)
    assert all(l == NONE or 0 <= l < n for l in labels)
    used = sorted({int(l) for l in labels if l != NONE})
    return used, [sum(1 for l in labels if l == u) for u in used]


def groups_of(labels):
    """(group_label, group_size): the labels in use by ascending label and the genomes that carry each (empty sketches count)"""
    used, sizes = _groups_of(tuple(int(l) for l in labels))
    return list(used), list(sizes)


def holds(c, t, m, rule):
    num, den, min_count, only = rule
    assert den >= 1 and 0 <= num <= den and min_count >= 1 and only in (0, 1)
    return c >= min_count and c * den >= num * m and (not only or c == t)


def from_sets(sketches, labels, rule):
    """the definition: c_l(h) = the distinct genomes labelled l whose sketch holds h, t(h) = the distinct genomes that hold h"""
    sets = [set(int(h) for h in s) for s in sketches]
    group_label, group_size = groups_of(labels)
    every = sorted(set().union(*sets)) if sets else []
    t = {h: sum(1 for s in sets if h in s) for h in every}
    kept = []
    for l, m in zip(group_label, group_size):
        members = [sets[v] for v in range(len(sets)) if labels[v] == l]
        kept.append([h for h in every if holds(sum(1 for s in members if h in s), t[h], m, rule)])
    return group_label, group_size, kept


def posting_lists(sketches):
    """{hash: the genomes that list it, one entry per occurrence} -- a genome that repeats a hash appears twice"""
    lists = {}
    for v, s in enumerate(sketches):
        for h in s:
            lists.setdefault(int(h), []).append(v)
    return lists


def from_lists(lists, labels, rule):
    """from posting lists ({hash: genomes, any order, repeats allowed}): one pass over the lists, a counter per label"""
    group_label, group_size = groups_of(labels)
    place = {l: g for g, l in enumerate(group_label)}
    kept = [[] for _ in group_label]
    for h in sorted(lists):
        distinct = set(lists[h])
        count = {}
        for v in distinct:
            if labels[v] != NONE:
                count[labels[v]] = count.get(labels[v], 0) + 1
        for l, c in count.items():
            if holds(c, len(distinct), group_size[place[l]], rule):
                kept[place[l]].append(h)
    return group_label, group_size, kept


def fast(sketches, labels, rule):
    """from_lists for collections of thousands of genomes (the same formulation with the lists made here)"""
    return from_lists(posting_lists(sketches), labels, rule)


def csr(kept, dtype=np.uint32):
    """(hashes, off) of a result's kept lists, as Sketches.download returns them"""
    off = np.zeros(len(kept) + 1, dtype=np.uint64)
    if kept:
        off[1:] = np.cumsum([len(k) for k in kept])
    flat = [h for k in kept for h in k]
    return np.array(flat, dtype=dtype), off


def parts_of(h, off):
    """the sketches of a CSR pair as a list of arrays"""
    return [h[int(off[g]):int(off[g + 1])] for g in range(len(off) - 1)]


def collections_of(n, hashes, literal):
    """collections of n genomes over `hashes` hashes, as tuples of holder masks (hash k is held by the genomes of mask[k]).  literal:
    every multiset of `hashes` masks.  Otherwise the 2^n masks dealt over collections of `hashes` hashes: whether a hash is kept
    depends on its own posting list alone, so every (labelling, holder set) is met although not every combination of holder sets --
    the literal enumeration of 5 genomes x 4 hashes has 4 * 10^8 cases per rule."""
    import itertools
    masks = list(range(1 << n))
    if literal:
        return list(itertools.combinations_with_replacement(masks, hashes))
    return [tuple(masks[i:i + hashes]) for i in range(0, len(masks), hashes)]


def exhaustive(n, hashes, literal, rule_names=("pan", "core", "majority", "markers", "min2")):
    """every labelling of n genomes (labels of every form: 0 .. n - 1, a member of the cluster or not, and NONE) x collections_of(n,
    hashes, literal), below 5 genomes each also with every genome listing its first hash twice: the two formulations agree; returns the
    cases seen"""
    import itertools
    seen = 0
    alphabet = list(range(n)) + [NONE]
    cols = collections_of(n, hashes, literal)
    for labels in itertools.product(alphabet, repeat=n):
        labels = list(labels)
        for holders in cols:
            sketches = [[k for k in range(len(holders)) if holders[k] >> v & 1] for v in range(n)]
            for repeat in ((False, True) if n < 5 else (False,)):
                if repeat:
                    sketches = [s + s[:1] for s in sketches]
                lists = posting_lists(sketches)
                for name in rule_names:
                    assert from_sets(sketches, labels, RULES[name]) == from_lists(lists, labels, RULES[name]), (labels, holders, name)
                seen += 1
    return seen


if __name__ == "__main__":
    for n_, k_, lit_ in ((1, 4, True), (2, 4, True), (3, 3, True), (3, 4, False), (4, 4, False), (5, 4, False)):
        print(n_, k_, lit_, exhaustive(n_, k_, lit_))
