"""The rule of rk_lca_rows / rk_lca_lists / rk_lca_call in plain Python, stated twice.

A taxonomy is a list `parent`: parent[t] == t marks the one root.  taxa[v] is the node of reference v or NONE.  For a hash h with
holders, lca(h) is the lowest common ancestor of the taxa of its labelled holders (undefined when none is labelled).  A query is a list
of hashes; every ELEMENT counts.  A row is (records, matched, unlabelled): records = sorted (taxon, direct) with direct > 0.

  from_sets    from the references' hash sets: the LCA as the deepest node common to the holders' root paths;
  from_lists   from exported posting lists (bisect): a pairwise fold of a two-node LCA (by ancestor sets).

call() is rk_lca_call from the definition: clade and score by scanning every node.  Nothing here is shared with the library."""
import bisect
import itertools

import numpy as np

NONE = 0xFFFFFFFF


# ---- taxonomies -------------------------------------------------------------------------------------------------------------------------
def root_path(parent, t):
    """t, its parent, .. the root"""
    path = [t]
    while parent[path[-1]] != path[-1]:
        path.append(parent[path[-1]])
        assert len(path) <= len(parent), "a cycle"
    return path


def is_taxonomy(parent):
    """exactly one root, every node reaches it"""
    T = len(parent)
    if T == 0 or any(not 0 <= p < T for p in parent) or sum(parent[t] == t for t in range(T)) != 1:
        return False
    for t in range(T):
        at, steps = t, 0
        while parent[at] != at:
            at, steps = parent[at], steps + 1
            if steps > T:
                return False
    return True


def taxonomies(max_nodes=4):
    """every parent array of 1 .. max_nodes nodes with one root and no cycle: T ** (T - 1) of T nodes"""
    for T in range(1, max_nodes + 1):
        for parent in itertools.product(range(T), repeat=T):
            if is_taxonomy(parent):
                yield list(parent)


def root_of(parent):
    return next(t for t in range(len(parent)) if parent[t] == t)


def lca_by_paths(parent, nodes):
    """the deepest node common to the root paths of `nodes` (non-empty)"""
    common = None
    for t in nodes:
        s = set(root_path(parent, t))
        common = s if common is None else common & s
    return max(common, key=lambda t: len(root_path(parent, t)))


def lca_of_two(parent, a, b):
    """walk b upwards until it meets an ancestor of a"""
    above = set(root_path(parent, a))
    while b not in above:
        b = parent[b]
    return b


def is_ancestor(parent, a, t):
    """a is t or above it"""
    return a in root_path(parent, t)


def children(parent, t):
    return [c for c in range(len(parent)) if parent[c] == t and c != t]


def star(leaves):
    """node 0 the root, 1 .. leaves its children"""
    return [0] * (leaves + 1)


def path(n):
    """0 - 1 - .. - n-1, node 0 the root"""
    return [max(0, t - 1) for t in range(n)]


def caterpillar(spine):
    """a spine 0 .. spine-1 (0 the root) with one leaf spine + i under every spine node i"""
    return path(spine) + list(range(spine))


def balanced_binary(leaves):
    """(parent, leaf nodes): a heap-shaped binary tree over `leaves` >= 1 leaves; the leaves are its last `leaves` nodes in order"""
    T = 2 * leaves - 1
    return [0] + [(t - 1) // 2 for t in range(1, T)], list(range(leaves - 1, T))


def renumbered(parent, taxa, perm):
    """the same taxonomy with node t called perm[t]: (parent', taxa')"""
    out = [0] * len(parent)
    for t, p in enumerate(parent):
        out[perm[t]] = perm[p]
    return out, [NONE if x == NONE else perm[x] for x in taxa]


# ---- the tally, twice -----------------------------------------------------------------------------------------------------------------
def tally(lcas):
    """(records, matched, unlabelled) of the per-element lcas of one query: None = no posting list, NONE = no labelled holder"""
    hit = [x for x in lcas if x is not None]
    direct = {}
    for x in hit:
        if x != NONE:
            direct[x] = direct.get(x, 0) + 1
    return sorted(direct.items()), len(hit), sum(x == NONE for x in hit)


def from_sets(refs, taxa, parent, queries, hash_bits=64):
    """refs: lists of hashes (repeats allowed, they change nothing here); one row per query"""
    sets = [set(r) for r in refs]
    rows = []
    for q in queries:
        lcas = []
        for h in q:
            holders = [v for v in range(len(refs)) if h in sets[v]] if h < (1 << hash_bits) else []
            labelled = [taxa[v] for v in holders if taxa[v] != NONE]
            lcas.append(None if not holders else NONE if not labelled else lca_by_paths(parent, labelled))
        rows.append(tally(lcas))
    return rows


def exported(refs):
    """(list hashes ascending, postings back to back, counts) as rk_index_export_lists returns them: a genome that repeats a hash
    appears as often in its list"""
    held = {}
    for v, r in enumerate(refs):
        for h in r:
            held.setdefault(h, []).append(v)
    hashes = sorted(held)
    return hashes, [v for h in hashes for v in sorted(held[h])], [len(held[h]) for h in hashes]


def q_lists(list_hashes, queries, rows=None):
    """(q_off, q_lists): per query the indices of the lists its elements hit, ascending, one per matched element (rows: only those)"""
    off, out = [0], []
    for i, q in enumerate(queries):
        mine = []
        if rows is None or i in rows:
            for h in q:
                k = bisect.bisect_left(list_hashes, h)
                if k < len(list_hashes) and list_hashes[k] == h:
                    mine.append(k)
        out += sorted(mine)
        off.append(len(out))
    return off, out


def from_lists(list_hashes, postings, counts, taxa, parent, queries):
    starts = [0]
    for c in counts:
        starts.append(starts[-1] + c)
    list_lca = []
    for u in range(len(counts)):
        l = NONE
        for v in postings[starts[u]:starts[u + 1]]:
            if taxa[v] != NONE:
                l = taxa[v] if l == NONE else lca_of_two(parent, l, taxa[v])
        list_lca.append(l)
    rows = []
    for q in queries:
        lcas = []
        for h in q:
            k = bisect.bisect_left(list_hashes, h)
            lcas.append(list_lca[k] if k < len(list_hashes) and list_hashes[k] == h else None)
        rows.append(tally(lcas))
    return rows


def selected_rows(n, row_first=0, row_step=1, row_block=0):
    rb, rs = max(1, row_block), max(1, row_step)
    return [r for r in range(n) if r // rb >= row_first and (r // rb - row_first) % rs == 0]


def flat(rows, selected=None):
    """(off, records, matched, unlabelled) as the library returns them; rows outside `selected` are empty, their counts None"""
    off, recs, matched, unl = [0], [], [], []
    for i, (r, m, u) in enumerate(rows):
        on = selected is None or i in selected
        recs += r if on else []
        off.append(len(recs))
        matched.append(m if on else None)
        unl.append(u if on else None)
    return off, recs, matched, unl


# ---- the exhaustive small cases ---------------------------------------------------------------------------------------------------------
UNIVERSE = [0, 1, 2, 3]
SUBSETS = [[h for h in UNIVERSE if m >> h & 1] for m in range(16)]
QUERIES = SUBSETS + [[0, 0, 3, 3, 3], [3, 2, 2, 9, 1]]    # the 16 sets, a multiset, and one in its own order with a hash nobody holds
# per number of references the collections: between them every set of holders occurs as a posting list (hash 3 of the second collection
# of three is held by nobody); in the last one reference 0 repeats hash 3
COLLECTIONS = {
    0: [[]],
    1: [[[0]]],
    2: [[[0, 2], [1, 2]]],
    3: [[[0, 3, 3], [1, 3], [2, 3]], [[0, 1], [0, 2], [1, 2]]],
}


def small_cases(max_nodes=4):
    """(parent, refs, taxa): every taxonomy of up to max_nodes nodes, under each every labelling (NONE included) of the collections above"""
    for parent in taxonomies(max_nodes):
        T = len(parent)
        for n, colls in COLLECTIONS.items():
            for taxa in itertools.product(list(range(T)) + [NONE], repeat=n):
                for refs in colls:
                    yield parent, refs, list(taxa)


N_SMALL_CASES = 23 + 134 + 1341 + 17984    # per T: T ** (T - 1) * (1 + (T + 1) + (T + 1) ** 2 + 2 * (T + 1) ** 3)


# ---- the call -----------------------------------------------------------------------------------------------------------------------------
def call(records, parent, rule, size=0):
    """rk_lca_call on one tally: ({taxon, candidate, clade, score, retained, n_taxa}, clade of every record) from the definition"""
    min_count, num, den, denom = rule
    T, root = len(parent), root_of(parent)
    kept = {t: d for t, d in records if d >= min_count}
    retained = sum(kept.values())
    clade = [sum(d for t, d in kept.items() if is_ancestor(parent, a, t)) for a in range(T)]
    score = [sum(d for t, d in kept.items() if is_ancestor(parent, t, a)) for a in range(T)]
    out = dict(taxon=NONE, candidate=NONE, clade=0, score=0, retained=retained, n_taxa=len(kept))
    if kept:
        best = max(score[t] for t in kept)
        cand = lca_by_paths(parent, [t for t in kept if score[t] == best])
        D = size if denom else retained
        out.update(candidate=cand, score=best, clade=clade[root])
        for t in root_path(parent, cand):
            if clade[t] * den >= num * D:
                out.update(taxon=t, clade=clade[t])
                break
    return out, [clade[t] for t, _ in records]


def small_tallies(max_nodes=4):
    """(parent, tallies): under every taxonomy of up to max_nodes nodes every tally with direct in 0 .. 3 per node (0 .. 2 with 4 nodes)"""
    for parent in taxonomies(max_nodes):
        T = len(parent)
        yield parent, [[(t, d) for t, d in enumerate(ds) if d] for ds in itertools.product(range(4 if T < 4 else 3), repeat=T)]


N_SMALL_TALLIES = 4 + 2 * 16 + 9 * 64 + 64 * 81
RULES = [(m, n, d, w) for m in (1, 2) for n, d in ((0, 1), (1, 2), (2, 3), (1, 1)) for w in (0, 1)]


# ---- arrays ---------------------------------------------------------------------------------------------------------------------------------
def as_arrays(parts, dtype=np.uint32):
    """(hashes back to back, offsets) of a list of sketches"""
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    flat_ = [h for p in parts for h in p]
    return np.array(flat_, dtype=dtype), off


def records_of(counts):
    """[(taxon, direct)] of a LCA_COUNT_DTYPE array"""
    return [(int(t), int(d)) for t, d in zip(counts["taxon"], counts["direct"])]
