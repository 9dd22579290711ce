"""rk_cluster_merge (host only) and the refusals of rk_cluster_rows that need no context: the fold of two partitions against a
Python union-find, null pointers and entries beyond n, the size of rk_cluster_stats against the header's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rabbitkssd_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG = -1


def canonical(parent_of_edges, n):
    """labels (smallest member of the component) of the graph with the given edges: a plain union-find"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in parent_of_edges:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.uint32)


def random_partition(rng, n):
    k = int(rng.integers(0, 2 * n))
    return canonical(zip(rng.integers(0, n, size=k).tolist(), rng.integers(0, n, size=k).tolist()), n)


def want_merge(a, b):
    n = len(a)
    return canonical([(i, int(a[i])) for i in range(n)] + [(i, int(b[i])) for i in range(n)], n)


def test_merge_equals_a_python_union_find():
    rng = np.random.default_rng(20)
    for case in range(200):
        n = 1 + case * 499 // 199   # 1 .. 500
        a, b = random_partition(rng, n), random_partition(rng, n)
        got = capi.cluster_merge(a, b)
        want = want_merge(a, b)
        assert np.array_equal(got, want), (case, n)
        assert np.array_equal(got[got], got) and np.all(got <= np.arange(n))
        assert np.array_equal(capi.cluster_merge(b, a), want)
    assert n == 500


def test_merge_identity_all_zero_and_aliasing():
    rng = np.random.default_rng(21)
    L = capi.lib()
    L.rk_cluster_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    for n in (1, 2, 7, 64, 333):
        ident, zero = np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        a = random_partition(rng, n)
        assert np.array_equal(capi.cluster_merge(ident, ident), ident)
        assert np.array_equal(capi.cluster_merge(a, ident), a)
        assert np.array_equal(capi.cluster_merge(ident, a), a)
        assert np.array_equal(capi.cluster_merge(a, a), a)
        assert np.array_equal(capi.cluster_merge(a, zero), zero)
        b = random_partition(rng, n)
        want = want_merge(a, b)
        inplace = a.copy()   # out aliases a
        assert L.rk_cluster_merge(inplace.ctypes.data, b.ctypes.data, n, inplace.ctypes.data) == 0
        assert np.array_equal(inplace, want)
    assert L.rk_cluster_merge(ident.ctypes.data, ident.ctypes.data, 0, ident.ctypes.data) == 0   # n = 0: nothing read or written


def test_merge_refuses_entries_beyond_n_and_null_pointers():
    L = capi.lib()
    L.rk_cluster_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    good = np.array([0, 0, 2, 2], dtype=np.uint32)
    out = np.full(4, 77, dtype=np.uint32)
    for bad in ([0, 0, 4, 2], [0, 0, 2, 0xFFFFFFFF]):
        bad = np.array(bad, dtype=np.uint32)
        assert L.rk_cluster_merge(bad.ctypes.data, good.ctypes.data, 4, out.ctypes.data) == RK_ERR_ARG
        assert L.rk_cluster_merge(good.ctypes.data, bad.ctypes.data, 4, out.ctypes.data) == RK_ERR_ARG
        assert np.all(out == 77)   # refused before anything is written
        with pytest.raises(capi.RkError) as e:
            capi.cluster_merge(good, bad)
        assert e.value.code == RK_ERR_ARG
    assert L.rk_cluster_merge(None, good.ctypes.data, 4, out.ctypes.data) == RK_ERR_ARG
    assert L.rk_cluster_merge(good.ctypes.data, None, 4, out.ctypes.data) == RK_ERR_ARG
    assert L.rk_cluster_merge(good.ctypes.data, good.ctypes.data, 4, None) == RK_ERR_ARG


def test_cluster_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_cluster_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_void_p, C.POINTER(capi.ClusterStats)]
    opts = capi.DistOpts(1, 0, 20, 0, 0.05, 0, 1)
    labels = np.zeros(4, dtype=np.uint32)
    st = capi.ClusterStats()
    assert L.rk_cluster_rows(None, None, C.byref(opts), labels.ctypes.data, C.byref(st)) == RK_ERR_ARG
    assert L.rk_cluster_rows(None, None, None, None, None) == RK_ERR_ARG
    assert "rk_cluster_rows" in capi.EXPORTS and "rk_cluster_merge" in capi.EXPORTS


def test_cluster_stats_has_the_headers_size():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    m = re.search(r"typedef struct rk_cluster_stats \{(.*?)\} rk_cluster_stats;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    width = {"uint64_t": 8, "uint32_t": 4}
    fields = [(t, name) for t, name in re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", body)]
    assert [name for _, name in fields] == [name for name, _ in capi.ClusterStats._fields_]
    assert C.sizeof(capi.ClusterStats) == sum(width[t] for t, _ in fields) == 40
    for (t, name), (_, ctype) in zip(fields, capi.ClusterStats._fields_):
        assert C.sizeof(ctype) == width[t], name
