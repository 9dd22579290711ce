"""Reference of the greedy tests: the sequential rule over a hit list with exact rational ratios, and a checker of the properties
that characterise its result.  Imports nothing of the package under test.

A hit is (row, col, common, size0, size1) with row < col, one per pair.  Genome a PRECEDES b iff (priority[a], a) < (priority[b], b);
without a priority the larger sketch first: (-size[a], a).  Walking the genomes in this order, a genome is a representative iff no
representative that precedes it is adjacent to it; otherwise it is a member of the nearest adjacent representative that precedes it:
the largest ratio common / u -- u = size0 + size1 - common for metric 0, min(size0, size1) for metric 1 --, ties to the smallest
index (include/rabbitkssd.h, greedy representatives)."""
from fractions import Fraction


def ratio(hit, metric):
    _, _, common, size0, size1 = hit
    return Fraction(common, size0 + size1 - common if metric == 0 else min(size0, size1))


def sizes_of(hits, n):
    """the sizes the records name (triangle 1: size0 = |S_row|, size1 = |S_col|); 0 for a genome without a record"""
    size = [None] * n
    for row, col, _, size0, size1 in hits:
        for g, s in ((row, size0), (col, size1)):
            assert size[g] in (None, s), "records disagree about the size of genome %d" % g
            size[g] = s
    return [0 if s is None else s for s in size]


def order_of(n, priority=None, sizes=None):
    """the genomes in priority order"""
    if priority is not None:
        return sorted(range(n), key=lambda a: (int(priority[a]), a))
    return sorted(range(n), key=lambda a: (-int(sizes[a]), a))


def greedy(hits, n, metric, priority=None, sizes=None):
    """(rep, links): rep[i] = i's representative, links = {member: its hit to the representative}.  Without a priority the order
    comes from `sizes` (default: the sizes the records name)."""
    hits = [tuple(int(x) for x in h) for h in hits]
    if priority is None and sizes is None:
        sizes = sizes_of(hits, n)
    order = order_of(n, priority, sizes)
    adjacent = [[] for _ in range(n)]
    for h in hits:
        assert h[0] < h[1] < n
        adjacent[h[0]].append((h[1], h))
        adjacent[h[1]].append((h[0], h))
    rep, links, is_rep = [None] * n, {}, [False] * n
    for v in order:   # (a genome later in the order is not a representative yet: `is_rep` alone says "precedes")
        near = [(-ratio(h, metric), other, h) for other, h in adjacent[v] if is_rep[other]]
        if not near:
            is_rep[v] = True
            rep[v] = v
        else:
            _, r, h = min(near)
            rep[v] = r
            links[v] = h
    return rep, links


def rounds(hits, n, priority=None, sizes=None):
    """(is_rep, rounds): the parallel decision rounds of the device path (include/rabbitkssd.h), modelled step by step.  Per round an
    edge pass over the live records -- hi the endpoint that precedes lo: hi a representative covers lo, hi a member drops the record,
    both undecided blocks lo for this round -- then a vertex pass: covered -> member, neither covered nor blocked -> representative.
    The rounds end with the first that leaves no genome undecided; without a record there is none."""
    hits = [tuple(int(x) for x in h) for h in hits]
    if priority is None and sizes is None:
        sizes = sizes_of(hits, n)
    place = {g: k for k, g in enumerate(order_of(n, priority, sizes))}
    live = [(h[0], h[1]) if place[h[0]] < place[h[1]] else (h[1], h[0]) for h in hits]
    undecided, rep, member = 0, 1, 2
    state, covered, count = [undecided] * n, [False] * n, 0
    if not hits:
        return [True] * n, 0
    while True:
        count += 1
        blocked, still = set(), []
        for hi, lo in live:
            if state[hi] == rep:
                covered[lo] = True
            elif state[hi] == undecided:
                if state[lo] == undecided:
                    blocked.add(lo)
                still.append((hi, lo))
        live = still
        left = 0
        for v in range(n):
            if state[v] == undecided:
                if covered[v]:
                    state[v] = member
                elif v not in blocked:
                    state[v] = rep
                else:
                    left += 1
        if not left:
            return [s == rep for s in state], count
        assert count <= n, "the rounds do not end"


def check_properties(hits, n, metric, rep, links, priority=None, sizes=None):
    """the four properties that single the result out (by induction over the order: they fix every genome's fate in turn)"""
    hits = [tuple(int(x) for x in h) for h in hits]
    if priority is None and sizes is None:
        sizes = sizes_of(hits, n)
    place = {g: k for k, g in enumerate(order_of(n, priority, sizes))}
    is_rep = [rep[i] == i for i in range(n)]
    known = set(hits)
    adjacent = [[] for _ in range(n)]
    for h in hits:
        adjacent[h[0]].append((h[1], h))
        adjacent[h[1]].append((h[0], h))
        assert not (is_rep[h[0]] and is_rep[h[1]]), "a hit joins two representatives: %r" % (h,)
    assert sorted(links) == [i for i in range(n) if not is_rep[i]]
    for m, h in links.items():
        r = rep[m]
        assert h in known and {h[0], h[1]} == {m, r} and is_rep[r] and place[r] < place[m], "the link of %d" % m
        for other, g in adjacent[m]:   # no adjacent preceding representative is nearer in the strict order
            if is_rep[other] and place[other] < place[m] and other != r:
                assert (-ratio(g, metric), other) > (-ratio(h, metric), r), "genome %d has a nearer representative %d" % (m, other)
    for v in range(n):
        if is_rep[v]:
            assert not any(is_rep[other] and place[other] < place[v] for other, _ in adjacent[v]), "representative %d" % v


def hit_tuples(rec):
    """a structured array with the fields of rk_hit as a list of hits"""
    return list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["common"].tolist(), rec["size0"].tolist(), rec["size1"].tolist()))
