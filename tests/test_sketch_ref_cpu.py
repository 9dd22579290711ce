"""The numpy model of the sketcher's candidate stream (tests/_sketch_ref.py) against the oracle, on the CPU: its distinct
dr_tuples are the oracle's hash set, its valid windows the oracle's count, and with an occurrence threshold it is the
oracle's FASTQ sketch -- on every family of genomes tests/test_gpu_sketch_edges.py builds, at small size, and on the golden
sketch fixtures."""
import json
import os

import numpy as np
import pytest

import _sketch_ref as sr
from conftest import GOLDEN
from oracle import oracle as ok

# (one set with 28 inner bits: its .shuf table has 2^28 entries and takes the oracle a good while to shuffle)
SETS = [(10, 6, 3), (8, 5, 2), (7, 4, 1), (16, 6, 3), (16, 4, 1), (11, 7, 4), (11, 6, 2)]


def agree(ps, seq, rec_off):
    rec_off = np.asarray(rec_off, dtype=np.uint64)
    dr, pos, windows = sr.candidates(ps, seq, rec_off)
    assert np.array_equal(np.unique(dr), ok.sketch_records(ps.param, ps.table, seq, rec_off))
    assert windows == ok.count_windows(ps.param, seq, rec_off)
    assert len(pos) == len(dr) and (len(pos) < 2 or np.all(np.diff(pos) > 0))
    return dr, pos


def families(ps, rng):
    """(seq, rec_off) of every kind of genome the GPU tests use, a few thousand bases each"""
    k = ps.k
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTacgtNnRYKMSWBDHV-", dtype=np.uint8)
    yield np.zeros(0, dtype=np.uint8), [0]
    yield np.zeros(0, dtype=np.uint8), [0, 0]
    for n in (1, k - 1, k, k + 1, 1023, 1024, 1025, 3000):
        yield sr.LUT[rng.integers(0, 4, n)], [0, n]
    yield alphabet[rng.integers(0, len(alphabet), 5000)], [0, 700, 700, 701, 4000, 5000]
    d = sr.dense(ps, rng, 120)
    yield d, [0, len(d)]
    yield d, [0, k, 2 * k + 3, len(d) // 2, len(d)]                       # records that end inside planted k-mers
    yield sr.plant(ps, rng, 4096, [k - 1, 1023, 1024 + k, 2047, 3000, 4095]), [0, 4096]
    yield sr.plant(ps, rng, 4096, [k - 1, 1023, 2048, 4095], filler="N"), [0, 4096]
    yield sr.with_candidates(ps, d, 17), [0, len(d)]
    yield np.tile(sr.planted_kmers(ps, rng, 1)[0], 60), [0, 60 * k]        # one k-mer over and over
    g = sr.LUT[rng.integers(0, 4, 3000)].copy()
    g[1024 - 3] = ord("N")
    yield g, [0, 3000]
    yield g, [0, 1023, 2047, 3000]


@pytest.mark.parametrize("ksl", SETS)
def test_model_equals_oracle_on_every_family(ksl):
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(sum(ksl))
    total = 0
    for seq, rec_off in families(ps, rng):
        dr, _ = agree(ps, seq, rec_off)
        total += len(dr)
    assert total > 300   # the planted families do carry candidates


@pytest.mark.parametrize("ksl", SETS)
def test_planted_kmers_are_selected_where_they_were_put(ksl):
    """the generator against the model: every planted k-mer is a candidate ending where it was put, N filler yields no other
    window, and cutting at a candidate count meets it exactly"""
    ps = sr.param_set(*ksl)
    rng = np.random.default_rng(5 + sum(ksl))
    ends = [ps.k - 1, 500, 1023, 1024 + ps.k, 2047, 2048 + 2 * ps.k, 4000]
    seq = sr.plant(ps, rng, 4001, ends, filler="N")
    dr, pos = agree(ps, seq, [0, len(seq)])
    assert pos.tolist() == ends
    d = sr.dense(ps, rng, 300)
    dr, pos = agree(ps, d, [0, len(d)])
    assert set(range(ps.k - 1, len(d), ps.k)) <= set(pos.tolist())
    for n in (0, 1, 2, 100, len(dr)):
        cut = sr.with_candidates(ps, d, n)
        assert len(cut) == len(d) and len(agree(ps, cut, [0, len(cut)])[0]) == n
    # disjoint sets of .shuf entries give disjoint planted hashes (the drain test relies on it)
    a = sr.candidates(ps, sr.plant(ps, rng, 2000, range(ps.k - 1, 2000, ps.k + 5), "N", ps.selected[0::2]), [0, 2000])[0]
    b = sr.candidates(ps, sr.plant(ps, rng, 2000, range(ps.k - 1, 2000, ps.k + 5), "N", ps.selected[1::2]), [0, 2000])[0]
    assert len(a) and len(b) and not set(a.tolist()) & set(b.tolist())


def test_model_equals_oracle_on_the_golden_fixtures():
    d = os.path.join(GOLDEN, "sketch")
    exp = json.load(open(os.path.join(d, "expected.json")))
    ps = sr.param_set(exp["half_k"], exp["half_subk"], exp["drlevel"])
    for fn, e in sorted(exp["files"].items()):
        seq, off = ok.read_fasta(os.path.join(d, fn))
        dr, _ = agree(ps, seq, off)
        assert np.unique(dr).tolist() == e["hashes"], fn
    d = os.path.join(GOLDEN, "sketch_ref")
    n = 0
    for case in json.load(open(os.path.join(d, "expected.json")))["cases"]:
        ps = sr.param_set(case["half_k"], case["half_subk"], case["drlevel"])
        for fn, want in case["files"].items():
            path = os.path.join(d, "inputs", fn)
            if case["kind"] == "fasta":
                seq, off = ok.read_fasta(path)
                assert np.unique(agree(ps, seq, off)[0]).tolist() == want, fn
            else:
                sq, ql, off = ok.parse_fastq_bytes(open(path, "rb").read())
                dr, _, _ = sr.candidates(ps, sq, off, ql, case["least_qual"])
                assert sr.kept(dr, case["least_num"]).tolist() == want, (fn, case["least_qual"], case["least_num"])
            n += len(want)
    assert n > 3000


@pytest.mark.parametrize("least_qual,least_num", [(0, 1), (0, 2), (0, 3), (50, 2), (127, 1)])
def test_model_with_an_occurrence_threshold_equals_the_fastq_oracle(least_qual, least_num):
    ps = sr.param_set(8, 5, 2)
    rng = np.random.default_rng(11)
    pool = sr.planted_kmers(ps, rng, 40)
    reads = [pool[rng.integers(0, 40, 6)].reshape(-1) for _ in range(60)]   # the same k-mers in many reads: counts 1..20
    seq = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    qual = rng.integers(33, 74, len(seq)).astype(np.uint8)
    dr, _, _ = sr.candidates(ps, seq, off, qual, least_qual)
    want = ok.sketch_records_fastq(ps.param, ps.table, seq, qual, off, least_qual, least_num)
    assert np.array_equal(sr.kept(dr, least_num), want)
    if least_qual == 0:
        counts = np.unique(dr, return_counts=True)[1]
        assert (counts < least_num).any() or least_num == 1
        assert (counts >= least_num).any()
    if least_qual == 127:
        assert len(dr) == 0
