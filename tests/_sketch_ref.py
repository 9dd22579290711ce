"""CPU reference of the sketcher's candidate STREAM (tests/test_gpu_sketch_edges.py, tests/test_sketch_ref_cpu.py).

The oracle returns a genome's hash set and its window count.  The dedup and capacity edges of the sketch kernels depend on
the candidate multiset -- one dr_tuple per valid selected window, repeats included -- and the seam tests on where each such
window ends.  `candidates` restates the per-window arithmetic that rk_sketch.hip cites (src/sketch.cpp:491-530: valid
windows per record, canonical k-mer :508, inner-base index :509, selection by the .shuf value :341/:516, dr_tuple
:519-524) over whole arrays of 64-bit integers; tests/test_sketch_ref_cpu.py holds it equal to the oracle.  Nothing here
knows about chunks, lanes or queues.

Positions are those of the PACKED layout of a genome (rk_pack_genomes): its records back to back with one separator byte
between two of them, so position p lies in 1 KiB block p >> 10 and in lane (p >> 4) & 63 of it."""
import functools

import numpy as np

from oracle import oracle as ok

U = np.uint64
_CODE = np.full(256, -1, dtype=np.int8)   # BaseMap: A 0, C 1, G 2, T 3, either case; anything else is no base
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_c] = _v
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


class ParamSet:
    """a parameter set with everything the model and the tests need; the fields come from the oracle's init_param"""

    def __init__(self, half_k, half_subk, drlevel):
        self.ksl = (half_k, half_subk, drlevel)
        self.param = ok.init_param(half_k, half_subk, drlevel)
        self.table = ok.shuffle_table(half_k, half_subk, drlevel)
        self.k = int(self.param.kmer_size)            # bases of a window
        self.out = int(self.param.half_outctx_len)    # outer context bases on either side
        self.inner = 2 * half_subk                    # inner bases, the index into the .shuf table
        self.hash_bits = 4 * (half_k - drlevel)
        self.selected = np.nonzero((self.table >= self.param.dim_start) & (self.table < self.param.dim_end))[0]


@functools.lru_cache(maxsize=None)
def param_set(half_k, half_subk, drlevel):
    """one ParamSet per process and parameter set: a .shuf table of 16^7 entries takes the oracle many seconds to shuffle"""
    return ParamSet(half_k, half_subk, drlevel)


def packed(seq, rec_off, qual=None, least_qual=0):
    """one genome in the packed layout: (bytes with 0x00 between records, the same as base codes with -1 for no base)"""
    seq = np.asarray(seq, dtype=np.uint8)
    rec_off = [int(x) for x in rec_off]
    n_rec = len(rec_off) - 1
    if n_rec <= 0:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int8)
    out = np.zeros(rec_off[-1] - rec_off[0] + n_rec - 1, dtype=np.uint8)
    at = 0
    for r in range(n_rec):
        part = seq[rec_off[r]:rec_off[r + 1]].copy()
        if qual is not None:   # the FASTQ gate (src/sketch.cpp:785): a base below least_qual is no base
            part[np.asarray(qual[rec_off[r]:rec_off[r + 1]], dtype=np.uint8).view(np.int8) < least_qual] = 0
        out[at:at + len(part)] = part
        at += len(part) + 1
    return out, _CODE[out]


def candidates(ps, seq, rec_off, qual=None, least_qual=0):
    """(dr_tuples uint64 in stream order, packed position of each one's last base int64, number of valid windows)"""
    _, code = packed(seq, rec_off, qual, least_qual)
    k, out = ps.k, ps.out
    valid = code >= 0
    # bases since the last non-base, this one included (src/sketch.cpp:488,:503: base = 1 again)
    idx = np.arange(len(code), dtype=np.int64)
    last_bad = np.maximum.accumulate(np.where(valid, -1, idx)) if len(code) else idx
    end = np.nonzero(idx - last_bad >= k)[0]   # last bases of the valid windows (:506)
    if not len(end):
        return np.zeros(0, dtype=U), np.zeros(0, dtype=np.int64), 0
    c = code.astype(U)
    fwd = np.zeros(len(end), dtype=U)
    rvs = np.zeros(len(end), dtype=U)
    for j in range(k):   # base j of the window, oldest first
        b = c[end - (k - 1) + j]
        fwd |= b << U(2 * (k - 1 - j))        # :498, the newest base in the low bits
        rvs |= (b ^ U(3)) << U(2 * j)         # :499, the complement with the newest base on top
    uni = np.minimum(fwd, rvs)                                                   # :508
    dim = ((uni & U(ps.param.domask)) >> U(2 * out)).astype(np.int64)            # :509
    v = ps.table[dim].astype(np.int64)
    sel = (v >= ps.param.dim_start) & (v < ps.param.dim_end)                     # :341, :516
    uni, v = uni[sel], v[sel]
    pf = (v - ps.param.dim_start).astype(U)                                      # :519-521
    dr = (((uni & U(ps.param.undomask0)) | ((uni & U(ps.param.undomask1)) << U(2 * k - 4 * out)))
          >> U(4 * ps.param.drlevel)) | pf                                       # :524
    return dr, end[sel], len(end)


def kept(dr, min_count=1):
    """the sketch of a candidate stream: distinct dr_tuples that occur at least min_count times, ascending (:526-529, :828-845)"""
    u, n = np.unique(dr, return_counts=True)
    return u[n >= min_count]


def planted_kmers(ps, rng, n, dims=None):
    """n k-mers (n x k array of ASCII bases) whose canonical inner bases are selected entries of the .shuf table: the inner bases
    spell an entry of `dims` (default: any selected one), the first base is A and the last one is not T, so that the forward
    strand is the canonical one whatever lies between.  Needs an outer context (half_k > half_subk)."""
    assert ps.out >= 1
    dims = ps.selected if dims is None else np.asarray(dims)
    d = dims[rng.integers(0, len(dims), n)].astype(U)
    shifts = (2 * (ps.inner - 1 - np.arange(ps.inner))).astype(U)   # first inner base in the high bits
    inner = ((d[:, None] >> shifts[None, :]) & U(3)).astype(np.uint8)
    left = rng.integers(0, 4, (n, ps.out), dtype=np.uint8)
    right = rng.integers(0, 4, (n, ps.out), dtype=np.uint8)
    left[:, 0] = 0
    right[:, -1] = rng.integers(0, 3, n, dtype=np.uint8)
    return LUT[np.concatenate([left, inner, right], axis=1)]


def plant(ps, rng, length, ends, filler="random", dims=None):
    """a sequence of `length` bases with a planted k-mer ending at every position of `ends` (positions of last bases, at least k
    apart from each other and >= k - 1); the rest is random ACGT or N.  What came out is for `candidates` to say."""
    seq = LUT[rng.integers(0, 4, length)] if filler == "random" else np.full(length, ord(filler), dtype=np.uint8)
    ends = np.asarray(sorted(set(int(e) for e in ends)), dtype=np.int64)
    assert len(ends) == 0 or (ends[0] >= ps.k - 1 and ends[-1] < length and (len(ends) < 2 or np.diff(ends).min() >= ps.k))
    km = planted_kmers(ps, rng, len(ends), dims)
    for e, w in zip(ends, km):
        seq[e - ps.k + 1:e + 1] = w
    return seq


def dense(ps, rng, n_kmers, dims=None):
    """planted k-mers back to back: every k-th window is selected by construction, 50x and more the density of a random genome"""
    return planted_kmers(ps, rng, n_kmers, dims).reshape(-1)


def with_candidates(ps, seq, n, filler=ord("N")):
    """`seq` cut where the model counts exactly n candidates (its n-th candidate's last base is the last base kept), then filled
    up to its old length with N: a single-record genome of the same length -- the same region capacity -- with n candidates"""
    dr, pos, _ = candidates(ps, seq, [0, len(seq)])
    assert len(dr) >= n, "the sequence carries %d candidates, %d wanted" % (len(dr), n)
    out = seq.copy()
    out[(int(pos[n - 1]) + 1 if n else 0):] = filler
    return out
