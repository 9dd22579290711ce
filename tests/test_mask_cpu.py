"""The host side of the filter of query sketches by an index (rk_mask_lists), the refusals of rk_sketches_mask that need no context and
the sizes of its structures -- against tests/_mask_ref.py: the rule twice in plain Python, the two statements checked against each
other first.  The golden pairs carry the real reference's own `sub` outputs.  All comparisons are exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _mask_ref as mk
from conftest import GOLDEN, ROOT
from oracle import oracle as ok
from rabbitkssd_amd import capi
from rabbitkssd_amd.build import HIPCC

RK_ERR_ARG = -1
LISTS_ARGTYPES = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(capi.MaskRule), C.POINTER(C.c_void_p), C.c_void_p,
                  C.POINTER(capi.MaskStats)]
MASK_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.MaskRule), C.POINTER(C.c_void_p), C.POINTER(capi.MaskStats)]


def library(refs, queries, min_refs, max_refs, dtype=np.uint32):
    """rk_mask_lists over the exported lists: (the survivors per query as lists, stats)"""
    list_hashes, counts = mk.exported(refs)
    q, q_off = mk.as_arrays([list(x) for x in queries], dtype)
    h, off, st = capi.mask_lists(q, q_off, np.array(list_hashes, dtype=dtype), counts, min_refs, max_refs)
    assert h.dtype == dtype and off.dtype == np.uint64 and off[0] == 0 and off[-1] == len(h)
    return [p.tolist() for p in mk.parts_of(h, off)], st


def checked(refs, queries, min_refs, max_refs, dtype=np.uint32):
    """the library against the definition, stats included; returns the survivors"""
    want = mk.from_counter(refs, queries, min_refs, max_refs)
    got, st = library(refs, queries, min_refs, max_refs, dtype)
    assert got == want, (refs, queries, min_refs, max_refs)
    total = sum(len(q) for q in queries)
    assert st["path"] == 2 and st["hashes"] == total and st["kept"] == sum(len(k) for k in want)
    assert st["matched"] == mk.matched(refs, queries) and st["emptied"] == mk.emptied(queries, want)
    assert st["tile_hashes"] >= 64 and st["threads"] >= 64 and st["tiles"] == -(-total // st["tile_hashes"])
    return got


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree_on_every_small_collection():
    """every collection of up to 3 references and the queries over a universe of 5 hashes (small_collections says what that leaves
    out and why it loses nothing), under every band with bounds in 0 .. 3"""
    seen = 0
    for refs in mk.small_collections():
        lists = mk.exported(refs)
        for a, b in mk.BANDS:
            assert mk.from_counter(refs, mk.SUBSETS, a, b) == mk.from_lists(*lists, mk.SUBSETS, a, b), (refs, a, b)
        seen += 1
    assert seen == 1 + 32 + 528 + 5984 and len(mk.BANDS) == 10


def test_reference_on_a_case_worked_by_hand():
    A, B, C_ = [1, 2, 3, 4], [3, 4, 5], [4, 4, 9]       # 4 is held four times: C repeats it
    query = [9, 4, 7, 3, 3, 1]                          # its own order, a repeat, a hash nobody holds
    for f in (mk.from_counter, mk.fast):
        assert f([A, B, C_], [query], *mk.SUB) == [[7]]
        assert f([A, B, C_], [query], *mk.PRESENT) == [[9, 4, 3, 3, 1]]
        assert f([A, B, C_], [query], 0, 1) == [[9, 7, 1]]
        assert f([A, B, C_], [query], 2, 3) == [[3, 3]]
        assert f([A, B, C_], [query], 4, 4) == [[4]]
        assert f([A, B, C_], [query, [], [7]], 2, mk.MAX) == [[4, 3, 3], [], []]
        assert f([], [query], *mk.SUB) == [query] and f([], [query], *mk.PRESENT) == [[]]
    assert mk.exported([A, B, C_]) == ([1, 2, 3, 4, 5, 9], [1, 1, 2, 4, 1, 1])
    assert mk.matched([A, B, C_], [query]) == 5 and mk.emptied([query, [], [7]], [[4], [], []]) == 1


# ---- rk_mask_lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_mask_lists_equals_the_reference_on_every_small_collection(dtype):
    seen = 0
    for refs in mk.small_collections():
        for a, b in mk.BANDS if len(refs) == 3 else mk.BANDS + [mk.PRESENT, (2, mk.MAX)]:
            checked(refs, mk.SUBSETS, a, b, dtype)
        seen += 1
    assert seen == 6545


def random_case(rng, wide):
    top = (1 << 36) if wide else (1 << 24)
    universe = [int(x) for x in rng.integers(0, top, size=int(rng.integers(4, 60)))]
    pick = lambda n: [universe[int(i)] for i in rng.integers(0, len(universe), size=n)]   # noqa: E731  (repeats happen, on both sides)
    refs = [pick(int(rng.integers(0, 25))) for _ in range(int(rng.integers(0, 9)))]
    queries = [pick(int(rng.integers(0, 30))) + [int(x) for x in rng.integers(0, top, size=int(rng.integers(0, 4)))] for _ in range(int(rng.integers(0, 6)))]
    return refs, queries


@pytest.mark.parametrize("wide", [False, True])
def test_mask_lists_equals_the_reference_on_random_collections(wide):
    rng = np.random.default_rng(71 + wide)
    dtype = np.uint64 if wide else np.uint32
    repeats = partial = emptied = 0
    for case in range(300):
        refs, queries = random_case(rng, wide)
        for a, b in (mk.SUB, mk.PRESENT, (0, 1), (2, mk.MAX), (1, 2), (3, 3)):
            got = checked(refs, queries, a, b, dtype)
            assert mk.fast(refs, queries, a, b) == got
            repeats += any(len(set(k)) < len(k) for k in got)
            partial += any(0 < len(k) < len(q) for q, k in zip(queries, got))
            emptied += mk.emptied(queries, got) > 0
    assert repeats > 100 and partial > 100 and emptied > 100


def test_queries_with_repeats_and_in_descending_order_keep_both():
    refs = [[10, 20, 30], [20, 30], [30]]
    query = [40, 30, 30, 20, 20, 10, 10, 5]
    assert checked(refs, [query], *mk.PRESENT) == [[30, 30, 20, 20, 10, 10]]
    assert checked(refs, [query], *mk.SUB) == [[40, 5]]
    assert checked(refs, [query, query[::-1]], 2, 3) == [[30, 30, 20, 20], [20, 20, 30, 30]]
    assert checked(refs, [query], 1, 1, np.uint64) == [[10, 10]]


def test_counts_at_the_bounds_and_one_off_either_side():
    # hash k is held by k references, k = 0 .. 6 (hash 0 by none); one reference repeats hash 6: its list has 7 entries
    refs = [[k for k in range(1, 7) if k > r] for r in range(6)] + [[6]]
    lists = mk.exported(refs)
    assert lists == ([1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 7])
    query = [0, 1, 2, 3, 4, 5, 6]
    count = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 7}
    for a in range(0, 9):
        for b in list(range(a, 9)) + [mk.MAX]:
            assert checked(refs, [query], a, b) == [[h for h in query if a <= count[h] <= b]]
    assert checked(refs, [query], 3, 4) == [[3, 4]] and checked(refs, [query], 6, 6) == [[]] and checked(refs, [query], 7, 7) == [[6]]


def golden(tag):
    """(ref parts, qry parts, the reference's own sub output) of the committed fixtures: tag "32" or "64" """
    import json
    manifest = json.load(open(os.path.join(GOLDEN, "f4", "manifest.json")))[tag]
    read = ok.read_sketches64 if tag == "64" else ok.read_sketches32
    out = []
    for path in (manifest["ref"], manifest["qry"], os.path.join("f4", "sub%s.sketch" % tag)):
        _, _, h, off = read(os.path.join(GOLDEN, path))
        out.append(mk.parts_of(h, off))
    return out


@pytest.mark.parametrize("tag", ["32", "64"])
def test_golden_pairs_equal_the_references_own_sub(tag):
    ref, qry, sub = golden(tag)
    dtype = np.uint64 if tag == "64" else np.uint32
    assert len(sub) == len(qry) and sum(len(s) for s in sub) > 0
    got = checked(ref, qry, *mk.SUB, dtype)
    assert [sorted(k) for k in got] == [sorted(s.tolist()) for s in sub]          # sketch by sketch as sorted arrays
    assert got == [s.tolist() for s in sub]                                         # (and in the file's order too: both keep the query's)
    present = checked(ref, qry, *mk.PRESENT, dtype)
    assert sum(len(k) for k in present) > 0
    for q, a, b in zip(qry, got, present):                                          # the two partition every query
        assert sorted(a + b) == sorted(q.tolist()) and not set(a) & set(b)


def test_sub_and_present_partition_every_query():
    rng = np.random.default_rng(9)
    for case in range(100):
        refs, queries = random_case(rng, case % 2 == 1)
        dtype = np.uint64 if case % 2 else np.uint32
        absent, present = library(refs, queries, *mk.SUB, dtype)[0], library(refs, queries, *mk.PRESENT, dtype)[0]
        for q, a, b in zip(queries, absent, present):
            assert sorted(a + b) == sorted(q) and not set(a) & set(b)


def test_mask_lists_refusals_write_nothing():
    L = capi.lib()
    L.rk_mask_lists.argtypes = LISTS_ARGTYPES
    for dtype in (np.uint32, np.uint64):
        q = np.array([5, 3, 9], dtype=dtype)
        q_off = np.array([0, 2, 3], dtype=np.uint64)
        lists = np.array([3, 9], dtype=dtype)
        counts = np.array([1, 2], dtype=np.uint32)
        off = np.full(3, 0x77, dtype=np.uint64)
        h = C.c_void_p(0x1234)
        st = capi.MaskStats()
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

        def call(qq=q, qo=q_off, nq=2, lh=lists, c=counts, n_lists=2, rule=(0, 0), ho=C.byref(h), o=off, s=C.byref(st)):
            r = capi.MaskRule(*rule) if rule is not None else None
            return L.rk_mask_lists(ptr(qq), int(dtype == np.uint64), ptr(qo), nq, ptr(lh), ptr(c), n_lists, C.byref(r) if r is not None else None, ho, ptr(o), s)
        assert call(rule=(2, 1)) == RK_ERR_ARG                                          # min_refs > max_refs
        assert call(rule=None) == RK_ERR_ARG
        assert call(qo=np.array([1, 2, 3], dtype=np.uint64)) == RK_ERR_ARG              # offsets that do not begin at 0
        assert call(qo=np.array([0, 2, 1], dtype=np.uint64)) == RK_ERR_ARG              # ... that descend
        assert call(lh=np.array([9, 3], dtype=dtype)) == RK_ERR_ARG                     # list hashes that descend
        assert call(lh=np.array([9, 9], dtype=dtype)) == RK_ERR_ARG                     # ... or repeat
        for null in ("qq", "qo", "lh", "c", "ho", "o"):
            assert call(**{null: None}) == RK_ERR_ARG, null
        assert h.value == 0x1234 and (off == 0x77).all() and st.hashes == 0x5A5A5A5A5A5A5A5A and st.path == 0x5A5A5A5A
        with pytest.raises(capi.RkError) as e:
            capi.mask_lists(q, q_off, lists, counts, 2, 1)
        assert e.value.code == RK_ERR_ARG
        assert call() == 0 and off.tolist() == [0, 1, 1] and st.kept == 1 and st.matched == 2 and st.emptied == 1   # and the good call writes
        assert np.frombuffer(C.string_at(h.value, q.itemsize), dtype=dtype).tolist() == [5]
        L.rk_free_host(h)
        assert call(s=None) == 0                                                         # the stats are optional
        L.rk_free_host(h)
    # no query; no list; nothing survives: RK_OK, NULL hashes
    h, off, st = capi.mask_lists(np.zeros(0, np.uint32), [0], np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert len(h) == 0 and off.tolist() == [0] and st["hashes"] == st["tiles"] == 0
    h, off, st = capi.mask_lists(np.array([4, 4], np.uint32), [0, 0, 2], np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert h.tolist() == [4, 4] and off.tolist() == [0, 0, 2] and st["matched"] == 0
    h, off, st = capi.mask_lists(np.array([4, 4], np.uint32), [0, 0, 2], np.array([4], np.uint32), [1])
    assert len(h) == 0 and off.tolist() == [0, 0, 0] and st["emptied"] == 1 and st["matched"] == 2


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_sketches_mask_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_sketches_mask.argtypes = MASK_ARGTYPES
    h = C.c_void_p(0x1234)
    r, st = capi.MaskRule(0, 0), capi.MaskStats()
    assert L.rk_sketches_mask(None, None, None, C.byref(r), C.byref(h), C.byref(st)) == RK_ERR_ARG
    assert L.rk_sketches_mask(None, None, None, None, None, None) == RK_ERR_ARG
    assert h.value == 0x1234 and st.path == 0


def test_mask_symbols_and_constants():
    L = capi.lib()
    for name in ("rk_sketches_mask", "rk_mask_lists"):
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert callable(capi.Context.sketches_mask) and callable(capi.mask_lists)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_MASK 15\b", hdr) and capi.MS_MASK == 15 and capi.MASK_MAX == mk.MAX == 2 ** 32 - 1
    L.rk_ctx_last_ms.restype = C.c_double
    assert L.rk_ctx_last_ms(None, 15) == 0.0


def test_mask_structures_have_the_headers_sizes():
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
    st = fields("rk_mask_stats")
    assert [x for _, x in st] == [x for x, _ in capi.MaskStats._fields_]
    assert C.sizeof(capi.MaskStats) == sum(width[t] for t, _ in st) == 56
    rule = fields("rk_mask_rule")
    assert [x for _, x in rule] == [x for x, _ in capi.MaskRule._fields_] == ["min_refs", "max_refs"] and C.sizeof(capi.MaskRule) == 8


# ---- the stand-alone check under the host sanitizers ----------------------------------------------------------------------------------
def test_mask_lists_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/mask_lists_check.cpp: rk_mask_lists against a plain restatement in a program of its own, host code under
    -fsanitize=address,undefined.  No GPU call is made."""
    exe = str(tmp_path / "mask_lists_check")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"),
                        os.path.join(ROOT, "rabbitkssd_amd", "csrc", "rk_mask.hip"), "-x", "hip", os.path.join(ROOT, "tools", "mask_lists_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    e = {k: v for k, v in os.environ.items() if not k.startswith("RK_")}
    p = subprocess.run([exe], capture_output=True, text=True, env=e)
    assert p.returncode == 0 and p.stdout.startswith("mask_lists_check: ok"), (p.stdout + p.stderr)[-4000:]
    assert not any(m in p.stderr for m in ("AddressSanitizer", "runtime error", "LeakSanitizer"))
