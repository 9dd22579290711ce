"""The host side of the per-cluster sketches (rk_group_lists), the refusals of rk_group_sketches that need no context and the sizes of
its structures -- against tests/_group_ref.py: the rule twice in plain Python, the two formulations checked against each other first;
and the tie to the reference's own `union` and `sub` outputs (tests/golden/f4)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import _group_ref as gr
from conftest import GOLDEN, ROOT
from oracle import oracle as ok
from rabbitkssd_amd import capi
from test_assign_cpu import random_labels   # labels of every form: below n without being a member, NONE, few clusters or many

RK_ERR_ARG = -1
NONE = gr.NONE
RULE_NAMES = ("pan", "core", "majority", "markers", "min2")
LISTS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(capi.GroupRule), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                  C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
SKETCHES_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.GroupRule), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                     C.POINTER(C.c_uint32), C.POINTER(capi.GroupStats)]


def exported(sketches, rng=None):
    """(postings, counts, hashes) of a collection as rk_index_export_lists returns them: the lists by ascending hash, a genome once per
    occurrence; with rng every list is shuffled"""
    lists = gr.posting_lists(sketches)
    hashes = sorted(lists)
    if rng is not None:
        lists = {h: [v[i] for i in rng.permutation(len(v))] for h, v in lists.items()}
    postings = np.array([v for h in hashes for v in lists[h]], dtype=np.uint32)
    return postings, np.array([len(lists[h]) for h in hashes], dtype=np.uint32), hashes


def library(sketches, labels, rule, rng=None):
    """rk_group_lists over the exported lists, in the reference's form"""
    postings, counts, hashes = exported(sketches, rng)
    off, kept, gl, gs = capi.group_lists(postings, counts, len(sketches), labels, rule)
    assert off.dtype == kept.dtype == np.uint64 and gl.dtype == gs.dtype == np.uint32
    assert len(off) == len(gl) + 1 == len(gs) + 1 and off[0] == 0 and off[-1] == len(kept)
    per = [kept[int(off[g]):int(off[g + 1])].tolist() for g in range(len(gl))]
    assert all(all(a < b for a, b in zip(k, k[1:])) for k in per)   # indices ascending
    return gl.tolist(), gs.tolist(), [[hashes[i] for i in k] for k in per]


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_the_two_formulations_agree_on_every_small_labelling():
    """every labelling of up to 5 genomes: literally every collection of 1 and 2 genomes over 4 hashes and of 3 genomes over 3; for 3, 4
    and 5 genomes every holder set in collections of 4 hashes (_group_ref.collections_of says why that loses nothing)"""
    seen = sum(gr.exhaustive(n, k, lit) for n, k, lit in ((1, 4, True), (2, 4, True), (3, 3, True), (3, 4, False), (4, 4, False), (5, 4, False)))
    assert seen == 2 * (2 * 5 + 9 * 35 + 64 * 120 + 64 * 2 + 625 * 4) + 7776 * 8


def test_reference_on_a_case_worked_by_hand():
    # hash 1: genomes 0 1 2 (labels 3 3 1); hash 2: genome 0 twice and genome 3 (unlabelled); hash 5: genomes 1 and 2; hash 9: genome 4 alone
    sketches = [[1, 2, 2], [1, 5], [1, 5], [2], [9]]
    labels = [3, 3, 1, NONE, 1]
    assert gr.groups_of(labels) == ([1, 3], [2, 2])
    for f in (gr.from_sets, gr.fast):
        assert f(sketches, labels, gr.RULES["pan"]) == ([1, 3], [2, 2], [[1, 5, 9], [1, 2, 5]])
        assert f(sketches, labels, gr.RULES["core"]) == ([1, 3], [2, 2], [[], [1]])
        assert f(sketches, labels, gr.RULES["majority"]) == ([1, 3], [2, 2], [[1, 5, 9], [1, 2, 5]])
        assert f(sketches, labels, gr.RULES["markers"]) == ([1, 3], [2, 2], [[9], []])   # (hash 2: the unlabelled holder defeats it)
        assert f(sketches, labels, gr.RULES["min2"]) == ([1, 3], [2, 2], [[], [1]])      # (hash 2 twice in genome 0 counts once)


# ---- rk_group_lists ---------------------------------------------------------------------------------------------------------
def test_group_lists_equals_the_reference_on_every_small_labelling():
    seen = 0
    for n in (1, 2, 3, 4):
        for labels in itertools.product(list(range(n)) + [NONE], repeat=n):
            for holders in gr.collections_of(n, 4, False):
                sketches = [[k + 7 for k in range(len(holders)) if holders[k] >> v & 1] for v in range(n)]
                for name in RULE_NAMES:
                    assert library(sketches, list(labels), gr.RULES[name]) == gr.from_sets(sketches, list(labels), gr.RULES[name]), (labels, holders, name)
                seen += 1
    assert seen > 2500


def test_group_lists_equals_the_reference_on_random_collections():
    rng = np.random.default_rng(211)
    empties = strangers = repeats = 0
    for case in range(200):
        n = int(rng.integers(1, 13))
        sketches = [rng.integers(0, 24, size=int(rng.integers(0, 9))).tolist() for _ in range(n)]   # repeats happen, empty sketches too
        labels = random_labels(rng, n)
        rule = gr.RULES[RULE_NAMES[case % 5]] if case % 7 else (int(rng.integers(0, 4)), 3, int(rng.integers(1, 4)), int(rng.integers(2)))
        want = gr.from_sets(sketches, labels, rule)
        assert want == gr.fast(sketches, labels, rule)
        assert library(sketches, labels, rule) == want
        assert library(sketches, labels, rule, rng) == want   # the order inside a list does not matter
        empties += sum(not k for k in want[2])
        strangers += any(l != NONE and labels[l] != l for l in labels)
        repeats += any(len(set(s)) < len(s) for s in sketches)
    assert empties > 50 and strangers > 50 and repeats > 50


def test_a_repeated_genome_counts_once():
    # genome 0 lists hash 4 three times: core of {0, 1} holds 4 only if 1 holds it too; markers of group 0 keeps it (c = t = 1)
    sketches = [[4, 4, 4], [6]]
    assert library(sketches, [0, 0], "core") == ([0], [2], [[]])
    assert library(sketches, [0, 1], "markers") == ([0, 1], [1, 1], [[4], [6]])
    assert library(sketches, [0, 0], (0, 1, 2, 0)) == ([0], [2], [[]])   # min_count 2: three occurrences are one genome


def test_need_beyond_the_members_gives_an_empty_group_that_is_still_listed():
    sketches = [[1, 2], [1, 2], [2]]
    assert library(sketches, [0, 0, 2], (0, 1, 3, 0)) == ([0, 2], [2, 1], [[], []])
    assert library(sketches, [0, 0, 2], (1, 1, 2, 0)) == ([0, 2], [2, 1], [[1, 2], []])
    assert library([[], [], [5]], [1, 1, NONE], "pan") == ([1], [2], [[]])   # members with empty sketches count towards m


def test_all_unlabelled_gives_no_group():
    off, kept, gl, gs = capi.group_lists(*exported([[1, 2], [2]])[:2], 2, [NONE, NONE])
    assert off.tolist() == [0] and len(kept) == len(gl) == len(gs) == 0
    off, kept, gl, gs = capi.group_lists(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, [])
    assert off.tolist() == [0] and len(kept) == len(gl) == len(gs) == 0


def marked():
    out = [C.c_void_p(0x1234) for _ in range(4)]
    return out, C.c_uint32(0xABABABAB)


def untouched(out, k):
    return all(o.value == 0x1234 for o in out) and k.value == 0xABABABAB


def test_group_lists_refusals_write_nothing():
    L = capi.lib()
    L.rk_group_lists.argtypes = LISTS_ARGTYPES
    postings = np.array([0, 1, 1], dtype=np.uint32)
    counts = np.array([2, 1], dtype=np.uint32)
    labels = np.array([0, NONE], dtype=np.uint32)
    out, k = marked()

    def call(p=postings, c=counts, n_lists=2, n=2, lab=labels, rule=(0, 1, 1, 0), outs=None, kk=None):
        r = capi.GroupRule(*rule) if rule is not None else None
        o = outs if outs is not None else [C.byref(x) for x in out]
        return L.rk_group_lists(p.ctypes.data if p is not None else None, c.ctypes.data if c is not None else None, n_lists, n,
                                lab.ctypes.data if lab is not None else None, C.byref(r) if r is not None else None, o[0], o[1], o[2], o[3],
                                C.byref(k) if kk is None else kk)
    assert call(p=np.array([0, 2, 1], dtype=np.uint32)) == RK_ERR_ARG            # a posting beyond the genomes
    assert call(lab=np.array([0, 2], dtype=np.uint32)) == RK_ERR_ARG             # a label that names nothing
    assert call(lab=np.array([0, NONE - 1], dtype=np.uint32)) == RK_ERR_ARG
    for rule in ((0, 0, 1, 0), (2, 1, 1, 0), (0, 1, 0, 0), (0, 1, 1, 2)):       # den 0, num > den, min_count 0, only 2
        assert call(rule=rule) == RK_ERR_ARG
    assert call(rule=None) == RK_ERR_ARG
    assert call(p=None) == RK_ERR_ARG and call(c=None) == RK_ERR_ARG and call(lab=None) == RK_ERR_ARG
    for miss in range(4):
        o = [C.byref(x) for x in out]
        o[miss] = None
        assert call(outs=o) == RK_ERR_ARG
    assert L.rk_group_lists(postings.ctypes.data, counts.ctypes.data, 2, 2, labels.ctypes.data, C.byref(capi.GroupRule(0, 1, 1, 0)),
                            *[C.byref(x) for x in out], None) == RK_ERR_ARG
    assert untouched(out, k)
    with pytest.raises(capi.RkError) as e:
        capi.group_lists(postings, counts, 2, [0, 5])
    assert e.value.code == RK_ERR_ARG
    assert call() == 0 and k.value == 1   # and the good call writes
    for o in out:
        L.rk_free_host(o)


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_group_sketches_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_group_sketches.argtypes = SKETCHES_ARGTYPES
    out, k = marked()
    rule, st = capi.GroupRule(0, 1, 1, 0), capi.GroupStats()
    labels = np.zeros(4, dtype=np.uint32)
    assert L.rk_group_sketches(None, None, labels.ctypes.data, C.byref(rule), C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(k), C.byref(st)) == RK_ERR_ARG
    assert L.rk_group_sketches(None, None, None, None, None, None, None, None, None) == RK_ERR_ARG
    assert untouched(out, k)


def test_group_symbols_and_constants():
    L = capi.lib()
    for name in ("rk_group_sketches", "rk_group_lists"):
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert callable(capi.Context.group_sketches) and callable(capi.group_lists)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_GROUP 13\b", hdr) and capi.MS_GROUP == 13
    assert re.search(r"#define RK_GROUP_NONE 0xFFFFFFFFu\b", hdr) and capi.GROUP_NONE == NONE == capi.DBSCAN_NOISE
    assert {k: capi.GROUP_RULES[k] for k in capi.GROUP_RULES} == {k: gr.RULES[k] for k in ("pan", "core", "majority", "markers")}


def test_group_structures_have_the_headers_sizes():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    width = {"uint64_t": 8, "uint32_t": 4}

    def fields(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for t, names in re.findall(r"\b(uint64_t|uint32_t)\s+([\w\s,]+);", body):
            out += [(t, x.strip()) for x in names.split(",")]
        return out
    st = fields("rk_group_stats")
    assert [x for _, x in st] == [x for x, _ in capi.GroupStats._fields_]
    assert C.sizeof(capi.GroupStats) == sum(width[t] for t, _ in st) == 88
    rl = fields("rk_group_rule")
    assert [x for _, x in rl] == [x for x, _ in capi.GroupRule._fields_] == ["share_num", "share_den", "min_count", "only"]
    assert C.sizeof(capi.GroupRule) == 16


# ---- the reference's own union and sub ----------------------------------------------------------------------------------------
def golden(tag):
    """(ref parts, qry parts, union parts, sub parts) of the committed fixtures: tag "32" or "64" """
    read = ok.read_sketches64 if tag == "64" else ok.read_sketches32
    d, s = ("dist64", "64") if tag == "64" else ("dist", "")
    out = []
    for path in (os.path.join(d, "ref%s.sketch" % s), os.path.join(d, "qry%s.sketch" % s), os.path.join("f4", "union%s.sketch" % tag),
                 os.path.join("f4", "sub%s.sketch" % tag)):
        _, _, h, off = read(os.path.join(GOLDEN, path))
        out.append(gr.parts_of(h, off))
    return out


@pytest.mark.parametrize("tag", ["32", "64"])
def test_pan_is_the_references_union_and_markers_its_sub(tag):
    ref, qry, union, sub = golden(tag)
    assert len(union) == 1 and len(sub) == len(qry) and any(len(p) == 0 for p in ref)   # (an empty sketch rides along)
    if tag == "32":
        assert len(ref) == 45 and len(qry) == 14 and len(union[0]) == 1870
    got = library(ref, [0] * len(ref), "pan")
    assert got == ([0], [len(ref)], [union[0].tolist()])
    for q, want in zip(qry, sub):
        gl, gs, kept = library(ref + [q], [0] * len(ref) + [len(ref)], "markers")
        assert gl == [0, len(ref)] and gs == [len(ref), 1]
        assert kept[1] == sorted(int(h) for h in want)   # (the reference writes `sub` in input order)
