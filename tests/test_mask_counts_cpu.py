"""The host side of masking counted sketches (rk_mask_lists_counts) against tests/_mask_ref.py: the hashes, offsets and stats of
rk_mask_lists, byte for byte, and every survivor with its own count; the refusals; the symbols."""
import ctypes as C

import numpy as np
import pytest

import _mask_ref as mk
from rabbitkssd_amd import capi

RK_ERR_ARG = -1
COUNTS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(capi.MaskRule), C.POINTER(C.c_void_p),
                   C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(capi.MaskStats)]


def check(refs, queries, counts_of, band, dtype=np.uint32):
    """queries: lists of hashes in any order; counts_of(query index, position) -> count"""
    lh, lc = mk.exported(refs)
    q_h, q_off = mk.as_arrays(queries, dtype)
    q_c = np.array([counts_of(i, j) for i, q in enumerate(queries) for j in range(len(q))], dtype=np.uint32)
    h, c, off, st = capi.mask_lists_counts(q_h, q_c, q_off, lh, lc, *band)
    h0, off0, st0 = capi.mask_lists(q_h, q_off, lh, lc, *band)
    assert h.tobytes() == h0.tobytes() and off.tobytes() == off0.tobytes() and st == st0 and h.dtype == dtype and c.dtype == np.uint32
    want = mk.fast(refs, queries, *band)
    assert [p.tolist() for p in mk.parts_of(h, off)] == want
    keep = [[j for j, x in enumerate(q) if x in set(k)] for q, k in zip(queries, want)]   # (a hash survives wherever it stands)
    assert c.tolist() == [counts_of(i, j) for i, js in enumerate(keep) for j in js]
    return len(h)


def test_mask_lists_counts_on_every_small_collection_and_band():
    kept = 0
    for n, refs in enumerate(mk.small_collections(2)):
        for band in mk.BANDS:
            kept += check(refs, mk.SUBSETS, lambda i, j: 1 + (7 * i + 3 * j + n) % 5, band)
    assert kept > 10000


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_mask_lists_counts_on_random_collections(dtype):
    rng = np.random.default_rng(12)
    top = (1 << 36) if dtype == np.uint64 else (1 << 24)
    pool = rng.integers(0, top, size=3000, dtype=np.uint64)
    for trial in range(6):
        refs = [rng.choice(pool, size=int(rng.integers(0, 300)), replace=False).tolist() for _ in range(12)]
        queries = [rng.permutation(np.unique(rng.choice(pool, size=int(rng.integers(0, 400))))).tolist() for _ in range(9)] + [[]]
        counts = [rng.integers(1, 2 ** 32, size=len(q), dtype=np.uint64) for q in queries]
        for band in (mk.SUB, mk.PRESENT, (0, 1), (2, mk.MAX), (1, 2), (3, 3)):
            check(refs, queries, lambda i, j: int(counts[i][j]), band, dtype)


def test_refusals_write_nothing_and_symbols():
    L = capi.lib()
    for name in ("rk_sketches_mask_counts", "rk_mask_lists_counts"):
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert callable(capi.Context.sketches_mask_counts) and callable(capi.mask_lists_counts)
    L.rk_mask_lists_counts.argtypes = COUNTS_ARGTYPES
    q, qc, off, lh, lc = np.array([5, 9], dtype=np.uint32), np.array([2, 3], dtype=np.uint32), np.array([0, 2], dtype=np.uint64), np.array([5], dtype=np.uint32), \
        np.array([1], dtype=np.uint32)
    out = np.full(2, 0x77, dtype=np.uint64)
    h, c = C.c_void_p(0x1234), C.c_void_p(0x4321)
    r = capi.MaskRule(0, 0)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

    def call(q=q, qc=qc, off=off, lh=lh, lc=lc, rule=r, hp=C.byref(h), cp=C.byref(c), o=out):
        return L.rk_mask_lists_counts(ptr(q), ptr(qc), 0, ptr(off), 1, ptr(lh), ptr(lc), 1, C.byref(rule) if rule is not None else None, hp, cp, ptr(o), None)
    for null in ("q", "qc", "off", "lh", "lc", "rule", "hp", "cp", "o"):
        assert call(**{null: None}) == RK_ERR_ARG, null
    assert call(rule=capi.MaskRule(2, 1)) == RK_ERR_ARG
    assert h.value == 0x1234 and c.value == 0x4321 and (out == 0x77).all()
    assert call() == 0 and out.tolist() == [0, 1]
    assert capi._take_array(h, 1, np.uint32).tolist() == [9] and capi._take_array(c, 1, np.uint32).tolist() == [3]
    hh, cc, oo, st = capi.mask_lists_counts(np.zeros(0, dtype=np.uint32), [], [0, 0], [5], [1])   # nothing survives: no arrays
    assert len(hh) == len(cc) == 0 and oo.tolist() == [0, 0]
    L.rk_sketches_mask_counts.argtypes = [C.c_void_p] * 6
    assert L.rk_sketches_mask_counts(None, None, None, None, None, None) == RK_ERR_ARG
