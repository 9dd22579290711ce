"""The host side of the screen with abundances (rk_screen_abund_lists), the refusals of rk_screen_abund_rows that need no context and the
sizes of its structures -- against tests/_screen_abund_ref.py: the rule twice in plain Python, the two statements checked against each
other and against the facts that follow from the rule first."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _screen_abund_ref as ar
import _screen_ref as sr
from conftest import ROOT
from rabbitkssd_amd import capi

RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OPTIONS = [(c, w) for c in (1, 2) for w in (0, 1)]
LISTS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.POINTER(capi.ScreenOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p]


def in_reference_form(off, recs, abund, matched, n_cand, claimed, occ):
    assert off.dtype == np.uint64 and recs.dtype == capi.SCREEN_REC_DTYPE and abund.dtype == capi.SCREEN_ABUND_DTYPE and occ.dtype == np.uint64
    return off.tolist(), sr.rec_tuples(recs), ar.abund_tuples(abund), matched.tolist(), n_cand.tolist(), claimed.tolist(), occ.tolist()


def library(refs, queries, min_common=1, min_won=0, sizes=None, **rows):
    p, c, q_off, q_lists, q_counts, occ = ar.exported(refs, queries)
    qs = [len(m) for m in queries]
    return capi.screen_abund_lists(p, c, q_off, q_lists, q_counts, len(refs), sr.sizes_of(refs, sizes), qs, occ, min_common, min_won, **rows)


def wanted(refs, queries, min_common=1, min_won=0, sizes=None, rows=None):
    return ar.as_arrays(ar.fast(refs, queries, min_common, min_won, sizes), refs, queries, rows, sizes)


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_the_two_statements_agree_and_the_facts_hold_on_every_small_collection():
    seen = 0
    for refs, queries in ar.small_collections():
        seen += 1
        for min_common, min_won in OPTIONS:
            a = ar.from_dicts(refs, queries, min_common, min_won)
            assert a == ar.fast(refs, queries, min_common, min_won), (refs, queries, min_common, min_won)
            ar.facts(refs, queries, a, min_common, min_won)
    assert seen > 25000


def test_reference_on_a_case_worked_by_hand():
    """tests/test_screen_cpu.py's case: A (10 hashes, all in the query) claims its 10, B (6 shared with A, hash 10 its own) hash 10, C its
    3, D nothing.  The count of hash h is h + 1, of 20 .. 22 it is 7, 7, 9."""
    A, B, C_, D = list(range(0, 10)), list(range(4, 11)), [20, 21, 22, 23], [5]
    query = {h: h + 1 for h in range(0, 11)}
    query.update({20: 7, 21: 7, 22: 9, 99: 1000})
    for f in (ar.from_dicts, ar.fast):
        recs, abund, matched, n_cand, claimed, occ = f([A, B, C_, D], [query])[0]
        assert recs == [(0, 0, 10, 10), (0, 1, 7, 1), (0, 2, 3, 3), (0, 3, 1, 0)]
        assert abund == [(55, 55, 5, 5), (5 + 6 + 7 + 8 + 9 + 10 + 11, 11, 8, 11), (23, 23, 7, 7), (6, 0, 6, 0)]
        assert (matched, n_cand, claimed, occ) == (14, 4, 14, (66 + 23 + 1000, 66 + 23, 66 + 23))
        recs, abund, matched, n_cand, claimed, occ = f([A, B, C_, D], [query], 4)[0]   # C and D are no candidates: 20 .. 22 unclaimed
        assert abund == [(55, 55, 5, 5), (56, 11, 8, 11)] and occ == (1089, 89, 66)
        assert f([A], [{}, {77: 3}]) == [([], [], 0, 0, 0, (0, 0, 0)), ([], [], 0, 0, 0, (3, 0, 0))]
    # the lower median: two values; all equal; two distinct values half and half
    for counts, med in (((4, 9), 4), ((9, 4), 4), ((6, 6, 6, 6), 6), ((2, 8, 8, 2), 2), ((8, 2, 2, 8, 2, 8), 2)):
        query = dict(zip(range(len(counts)), counts))
        for f in (ar.from_dicts, ar.fast):
            assert f([list(range(len(counts)))], [query])[0][1] == [(sum(counts), sum(counts), med, med)]


# ---- rk_screen_abund_lists ------------------------------------------------------------------------------------------------------
def check_together(cases):
    """rk_screen_abund_lists on several small collections in ONE call per option, as tests/test_screen_cpu.py: collection i keeps its
    hashes to itself (+ 1000 i), its references and queries follow those of the collections before it"""
    refs_all, queries_all, first = [], [], []
    for i, (refs, queries) in enumerate(cases):
        first.append((len(refs_all), len(queries_all)))
        refs_all += [[h + 1000 * i for h in r] for r in refs]
        queries_all += [{h + 1000 * i: c for h, c in m.items()} for m in queries]
    p, c, q_off, q_lists, q_counts, q_occ = ar.exported(refs_all, queries_all)
    rs, qs = sr.sizes_of(refs_all), [len(m) for m in queries_all]
    for min_common, min_won in OPTIONS:
        off, recs, abund, matched, n_cand, claimed, occ = [0], [], [], [], [], [], []
        for (r0, q0), (refs, queries) in zip(first, cases):
            for mine, ab, m, k, w, o in ar.fast(refs, queries, min_common, min_won):
                recs += [(q + q0, r + r0, common, won, rs[r + r0], qs[q + q0]) for q, r, common, won in mine]
                abund += ab
                off.append(len(recs))
                matched.append(m)
                n_cand.append(k)
                claimed.append(w)
                occ.append(list(o))
        got = capi.screen_abund_lists(p, c, q_off, q_lists, q_counts, len(refs_all), rs, qs, q_occ, min_common, min_won)
        assert in_reference_form(*got) == (off, recs, abund, matched, n_cand, claimed, occ), (cases, min_common, min_won)
        plain = capi.screen_lists(p, c, q_off, q_lists, len(refs_all), rs, qs, min_common, min_won)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((got[0], got[1]) + got[3:6], plain))   # the records: byte for byte the screen's


def test_screen_abund_lists_equals_the_reference_on_every_small_collection():
    together = []
    for refs, queries in ar.small_collections():
        together.append((refs, queries))
        if len(together) == 64:
            check_together(together)
            together = []
    check_together(together)


def random_clades(rng, n_ref, n_query, universe):
    """clades of related references of mixed sizes, queries that are unions of a few of them plus foreign hashes, with counts"""
    refs = []
    while len(refs) < n_ref:
        core = rng.choice(universe, size=int(rng.integers(5, 40)), replace=False)
        for _ in range(int(rng.integers(1, 6))):
            keep = core[rng.random(len(core)) < rng.uniform(0.4, 1.0)]
            own = rng.choice(universe, size=int(rng.integers(0, 8)), replace=False)
            refs.append(np.unique(np.concatenate([keep, own])).tolist())
    refs = refs[:n_ref]
    queries = []
    for k in range(n_query):
        members = rng.choice(n_ref, size=1 + k % 4, replace=False)
        parts = [np.array(refs[m], dtype=np.int64)[rng.random(len(refs[m])) < 0.8] for m in members]
        queries.append(np.unique(np.concatenate(parts + [rng.integers(universe, 2 * universe, size=int(rng.integers(0, 6)))])).tolist())
    return refs, ar.with_counts(queries + [[], [2 * universe + 1]], rng)


def test_screen_abund_lists_equals_the_reference_on_random_clades():
    rng = np.random.default_rng(37)
    for trial in range(10):
        refs, queries = random_clades(rng, 60, 10, 400)
        for min_common, min_won in ((1, 0), (2, 1), (3, 2)):
            got = in_reference_form(*library(refs, queries, min_common, min_won))
            assert got == wanted(refs, queries, min_common, min_won)
            assert len(got[1]) > 5
        if trial < 3:
            a = ar.from_dicts(refs, queries)
            assert a == ar.fast(refs, queries)
            ar.facts(refs, queries, a)


def test_row_shards_concatenate_and_leave_the_rest_alone():
    rng = np.random.default_rng(6)
    refs, queries = random_clades(rng, 50, 21, 300)
    whole = in_reference_form(*library(refs, queries, 2, 1))
    for step, block in ((2, 1), (3, 4)):
        recs, abund = [], []
        for first in range(step):
            rows = sr.selected_rows(len(queries), first, step, block)
            got = in_reference_form(*library(refs, queries, 2, 1, row_first=first, row_step=step, row_block=block))
            assert got == wanted(refs, queries, 2, 1, rows=rows)
            recs += got[1]
            abund += got[2]
        order = sorted(range(len(recs)), key=recs.__getitem__)
        assert [recs[i] for i in order] == whole[1] and [abund[i] for i in order] == whole[2]


def test_counts_at_the_top_of_32_bits_and_sums_beyond():
    top = 2 ** 32 - 1
    refs = [[1, 2, 3, 4], [4, 5]]
    queries = [{1: top, 2: top, 3: top, 4: top - 1, 5: 1}]
    got = in_reference_form(*library(refs, queries))
    assert got == wanted(refs, queries)
    assert got[2] == [(4 * top - 1, 4 * top - 1, top, top), (top, 1, 1, 1)] and got[6] == [[4 * top, 4 * top, 4 * top]]
    assert got[2][0][0] > 2 ** 32


def test_refusals_write_nothing():
    L = capi.lib()
    L.rk_screen_abund_lists.argtypes = LISTS_ARGTYPES
    u32, u64 = (lambda x: np.array(x, dtype=np.uint32)), (lambda x: np.array(x, dtype=np.uint64))
    postings, counts, q_off, ql, qc, rs, qsz, qocc = u32([0, 1, 1]), u32([2, 1]), u64([0, 2, 3]), u64([0, 1, 1]), u32([2, 1, 5]), u32([1, 2]), u32([2, 1]), u64([4, 5])
    off = np.full(3, 0x77, dtype=np.uint64)
    outs = [np.full(2, 0x77, dtype=np.uint32) for _ in range(3)]
    occ = np.full(6, 0x77, dtype=np.uint64)
    recs, abund, n = C.c_void_p(0x1234), C.c_void_p(0x4321), C.c_uint64(0x77)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

    def call(p=postings, c=counts, qo=q_off, l=ql, qcnt=qc, nq=2, n_ref=2, s=rs, z=qsz, qoc=qocc, opts=(1, 0, 0, 0, 0), o=off, r=C.byref(recs), ab=C.byref(abund),
             nn=C.byref(n), m=outs[0], k=outs[1], w=outs[2], oc=occ):
        op = capi.ScreenOpts(*opts) if opts is not None else None
        return L.rk_screen_abund_lists(ptr(p), ptr(c), 2, ptr(qo), ptr(l), ptr(qcnt), nq, n_ref, ptr(s), ptr(z), ptr(qoc), C.byref(op) if op is not None else None,
                                       ptr(o), r, ab, nn, ptr(m), ptr(k), ptr(w), ptr(oc))
    for null in ("p", "c", "qo", "l", "qcnt", "s", "z", "qoc", "o", "r", "ab", "nn", "m", "k", "w", "oc"):   # a null array
        assert call(**{null: None}) == RK_ERR_ARG, null
    assert call(qcnt=u32([2, 0, 5])) == RK_ERR_ARG and call(qcnt=u32([0, 1, 5])) == RK_ERR_ARG            # a zero count
    assert call(opts=None) == RK_ERR_ARG and call(opts=(0, 0, 0, 0, 0)) == RK_ERR_ARG                     # what rk_screen_lists refuses
    assert call(qo=u64([1, 2, 3])) == RK_ERR_ARG and call(qo=u64([0, 3, 2])) == RK_ERR_ARG
    assert call(l=u64([0, 2, 1])) == RK_ERR_ARG and call(l=u64([1, 0, 1])) == RK_ERR_ARG and call(l=u64([0, 0, 1])) == RK_ERR_ARG
    assert call(p=u32([0, 2, 1])) == RK_ERR_ARG and call(s=u32([1, 1])) == RK_ERR_ARG
    assert call(s=u32([1, 2 ** 30])) == RK_ERR_ARG and call(z=u32([2 ** 30, 1])) == RK_ERR_ARG
    assert recs.value == 0x1234 and abund.value == 0x4321 and n.value == 0x77 and (off == 0x77).all() and all((a == 0x77).all() for a in outs) and (occ == 0x77).all()
    assert call() == 0 and off.tolist() == [0, 2, 3] and n.value == 3 and occ.tolist() == [4, 3, 3, 5, 5, 5]
    assert ar.abund_tuples(capi._take_array(abund, 3, capi.SCREEN_ABUND_DTYPE)) == [(2, 0, 2, 0), (3, 3, 1, 1), (5, 5, 5, 5)]
    L.rk_free_host(recs)
    with pytest.raises(capi.RkError) as e:
        capi.screen_abund_lists(postings, counts, q_off, ql, [2, 0, 5], 2, rs, qsz, qocc)
    assert e.value.code == RK_ERR_ARG
    with pytest.raises(ValueError):
        capi.screen_abund_lists(postings, counts, q_off, ql, [2, 1], 2, rs, qsz, qocc)
    off, recs_, ab_, m, k, w, oc = capi.screen_abund_lists([], [], [0], [], [], 0, [], [], [])   # no query
    assert off.tolist() == [0] and len(recs_) == len(ab_) == len(m) == 0 and oc.shape == (0, 3)
    off, recs_, ab_, m, k, w, oc = capi.screen_abund_lists([], [], [0, 0, 0], [], [], 2, [3, 4], [5, 0], [9, 0])   # no list
    assert off.tolist() == [0, 0, 0] and len(recs_) == len(ab_) == 0 and oc.tolist() == [[9, 0, 0], [0, 0, 0]]


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_screen_abund_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_screen_abund_rows.argtypes = [C.c_void_p] * 13
    off = np.full(2, 0x77, dtype=np.uint64)
    recs, abund, n = C.c_void_p(0x1234), C.c_void_p(0x4321), C.c_uint64(0x77)
    o = capi.ScreenOpts(1, 0, 0, 0, 0)
    assert L.rk_screen_abund_rows(None, None, None, C.byref(o), off.ctypes.data, C.byref(recs), C.byref(abund), C.byref(n), None, None, None, None, None) == RK_ERR_ARG
    assert L.rk_screen_abund_rows(None, None, None, None, None, None, None, None, None, None, None, None, None) == RK_ERR_ARG
    assert recs.value == 0x1234 and abund.value == 0x4321 and n.value == 0x77 and (off == 0x77).all()


def test_symbols_constants_and_structures():
    L = capi.lib()
    for name in ("rk_screen_abund_rows", "rk_screen_abund_lists"):
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert callable(capi.Context.screen_abund_rows) and callable(capi.screen_abund_lists)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_SCREEN_ABUND 18\b", hdr) and capi.MS_SCREEN_ABUND == 18
    L.rk_ctx_last_ms.restype = C.c_double
    assert L.rk_ctx_last_ms(None, 18) == 0.0
    width = {"uint64_t": 8, "uint32_t": 4}

    def fields(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for t, names in re.findall(r"\b(uint64_t|uint32_t)\s+([\w\s,]+);", body):
            out += [(t, x.strip()) for x in names.split(",")]
        return out
    f = fields("rk_screen_abund_stats")
    assert [x for _, x in f] == [x for x, _ in capi.ScreenAbundStats._fields_]
    assert C.sizeof(capi.ScreenAbundStats) == sum(width[t] for t, _ in f) == 176
    assert f[:len(fields("rk_screen_stats"))] == fields("rk_screen_stats") and C.sizeof(capi.ScreenStats) == 120   # it begins with rk_screen_stats, which stays
    f = fields("rk_screen_abund")
    assert [x for _, x in f] == list(capi.SCREEN_ABUND_DTYPE.names) == list(ar.ABUND_FIELDS) and capi.SCREEN_ABUND_DTYPE.itemsize == 24
    assert [width[t] for t, _ in f] == [8, 8, 4, 4]


# ---- the stand-alone check under the host sanitizers ----------------------------------------------------------------------------------
def test_screen_abund_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/screen_abund_check.cpp: rk_screen_abund_lists and rk_mask_lists_counts against plain restatements in a program of its own,
    host code under -fsanitize=address,undefined.  No GPU call is made."""
    exe = str(tmp_path / "screen_abund_check")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"),
                        os.path.join(ROOT, "rabbitkssd_amd", "csrc", "rk_screen.hip"), os.path.join(ROOT, "rabbitkssd_amd", "csrc", "rk_mask.hip"), "-x", "hip",
                        os.path.join(ROOT, "tools", "screen_abund_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    e = {k: v for k, v in os.environ.items() if not k.startswith("RK_")}
    p = subprocess.run([exe], capture_output=True, text=True, env=e)
    assert p.returncode == 0 and p.stdout.startswith("screen_abund_check: ok"), (p.stdout + p.stderr)[-4000:]
    assert not any(m in p.stderr for m in ("AddressSanitizer", "runtime error", "LeakSanitizer"))
