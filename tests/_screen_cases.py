"""What the screen tests share: the argument types of the two calls, indexes built and imported from hash sets, the golden pairs with the
real reference's intersection counts and the random clades.  No test lives here."""
import ctypes as C
import os

import numpy as np

import _screen_ref as sr
from _selfjoin_cases import csr, device_index
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

LISTS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(capi.ScreenOpts),
                  C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p]
ROWS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.ScreenOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p,
                 C.c_void_p, C.c_void_p, C.POINTER(capi.ScreenStats)]


def queries_of(ctx, parts, wide=False):
    h, off = csr(parts, np.uint64 if wide else np.uint32)
    return ctx.sketches_from_host64(h, off) if wide else ctx.sketches_from_host(h, off)


def index_of(ctx, parts, wide=False, bits=24):
    h, off = csr(parts, np.uint64 if wide else np.uint32)
    return device_index(ctx, h, off, bits, wide)


def imported_index(ctx, parts, wide, bits):
    """the same collection through the oracle's .dict / .index arrays: no sketches, identity genome order, the sizes the caller's"""
    h, off = csr(parts, np.uint64 if wide else np.uint32)
    sizes = np.diff(off).astype(np.uint32)
    if wide:
        uhash, ucount, postings = ok.index_build64(h, off)
        return ctx.index_import64(postings, uhash, ucount, bits, sizes)
    postings, counts = ok.index_build32(h, off, bits)
    return ctx.index_import(postings, counts, bits, sizes)


def golden_pair(tag):
    """(reference names, reference sketches, query names, query sketches, {(query, reference): (common, size, size)}) of tests/golden/dist
    ("32") or dist64 ("64"): the triples are the real reference's"""
    read = ok.read_sketches64 if tag == "64" else ok.read_sketches32
    d, s = ("dist64", "64") if tag == "64" else ("dist", "")
    _, rnames, rh, roff = read(os.path.join(GOLDEN, d, "ref%s.sketch" % s))
    _, qnames, qh, qoff = read(os.path.join(GOLDEN, d, "qry%s.sketch" % s))
    triples = {}
    for line in open(os.path.join(GOLDEN, d, "dist%s_M0_D1_N0.ref.txt" % s)):
        f = line.rstrip("\n").split("\t")
        triples[(f[0], f[1])] = tuple(int(x) for x in f[2].split("|"))
    return rnames, sr.parts_of(rh, roff), qnames, sr.parts_of(qh, qoff), triples


_clades = {}


def clades(wide):
    """(refs, queries, bits): 1,000 genomes in clades of 10, sketches of about 40 hashes, in a shuffled caller order; 40 queries that
    are unions of 1 .. 6 genomes plus foreign hashes, one empty query and one of foreign hashes only"""
    if wide not in _clades:
        bits, kmer = (36, 24) if wide else (24, 20)
        names, h, off = synth.clade_sketches(1000, 40, bits, kmer_size=kmer, strains_per_clade=10, seed=91 + wide, wide=wide)
        names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=6))
        refs = sr.parts_of(h, off)
        rng = np.random.default_rng(17 + wide)
        dtype = np.uint64 if wide else np.uint32
        queries = []
        for k in range(40):
            members = rng.choice(len(refs), size=1 + k % 6, replace=False)
            if k % 3 == 0:   # relatives: strains of one clade hold each other's hashes, so most of them win nothing
                members = np.concatenate([members, [int(np.argmax([len(np.intersect1d(refs[members[0]], r)) if i != members[0] else 0 for i, r in enumerate(refs)]))]])
            foreign = rng.integers(0, 1 << bits, size=int(rng.integers(0, 30)), dtype=np.uint64)
            queries.append(np.unique(np.concatenate([refs[m].astype(np.uint64) for m in members] + [foreign])).astype(dtype))
        indexed = np.unique(h)
        queries.append(np.zeros(0, dtype=dtype))
        queries.append(np.setdiff1d(rng.integers(0, 1 << bits, size=50, dtype=np.uint64), indexed.astype(np.uint64)).astype(dtype))
        _clades[wide] = (refs, queries, bits)
    return _clades[wide]
