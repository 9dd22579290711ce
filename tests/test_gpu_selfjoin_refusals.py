"""The refusals in front of the self join's stage (csrc/rk_edge_stage.h: stage_options, stage_index), one table for all seven calls: which
options each call refuses, with which code and which text -- written out here, not taken from the library --, and which of two faults
it names.  One collection of 64 genomes and one index of it; every leg is one call that returns before or just behind a tiny join.
The join-only index and the 2^30 limit are not here: the first needs a sharded build (the suites of greedy, dbscan and mreach have
one), the second cannot be reached at test size."""
import numpy as np
import pytest

from _selfjoin_cases import KMER, device_index
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
RK_ERR_ARG = -1
N = 64

CALLS = {
    "rk_cluster_rows": lambda c, i: c.cluster_rows(i, 0, KMER, 0.05),
    "rk_forest_rows": lambda c, i: c.forest_rows(i, 0, KMER, 0.05),
    "rk_greedy_rows": lambda c, i: c.greedy_rows(i, 0, KMER, 0.05),
    "rk_knn_rows": lambda c, i: c.knn_rows(i, 0, KMER, 0.05, 3),
    "rk_dbscan_rows": lambda c, i: c.dbscan_rows(i, 0, KMER, 0.05, 3),
    "rk_mreach_rows": lambda c, i: c.mreach_rows(i, 0, KMER, 0.05, 3),
    "rk_medoid_rows": lambda c, i: c.medoid_rows(i, 0, KMER, 0.05, np.zeros(N, dtype=np.uint32)),
}
TRIANGLE = {
    "rk_cluster_rows": "rk_cluster_rows works on a self join: triangle must be 1",
    "rk_forest_rows": "rk_forest_rows works on a self join: triangle must be 1",
    "rk_greedy_rows": "rk_greedy_rows works on a self join: triangle must be 1",
    "rk_knn_rows": "rk_knn_rows works on a self join: triangle must be 1",
    "rk_dbscan_rows": "rk_dbscan_rows works on a self join: triangle must be 1",
    "rk_mreach_rows": "rk_mreach_rows works on a self join: triangle must be 1",
    "rk_medoid_rows": "rk_medoid_rows works on a self join: triangle must be 1",
}
EVERY_ROW = {   # the other four compose from row shards
    "rk_greedy_rows": "rk_greedy_rows needs every row: the greedy rule does not compose from row shards",
    "rk_dbscan_rows": "rk_dbscan_rows needs every row: the degrees of a row shard are partial, and the core test does not compose from shards",
    "rk_mreach_rows": "rk_mreach_rows needs every row: the core distances of a row shard are partial, and the weights do not compose from shards",
}
DENSE = {   # rk_cluster_rows answers a dense report
    "rk_forest_rows": "rk_forest_rows: a dense report (a threshold above 1.0) is not offered: pairs that share nothing carry no order",
    "rk_greedy_rows": "rk_greedy_rows: a dense report (a threshold above 1.0) is not offered: pairs that share nothing carry no order",
    "rk_knn_rows": "rk_knn_rows: a dense report (a threshold above 1.0) is not offered: pairs that share nothing carry no order",
    "rk_dbscan_rows": "rk_dbscan_rows: a dense report (a threshold above 1.0) is not offered: pairs that share nothing carry no order",
    "rk_mreach_rows": "rk_mreach_rows: a dense report (a threshold above 1.0) is not offered: pairs that share nothing carry no order",
    "rk_medoid_rows": "rk_medoid_rows: a dense report (a threshold above 1.0) is not offered: pairs that share nothing carry no order",
}
DENSE_D = (1.5, float(np.nextafter(1.0, 2.0)))


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


@pytest.fixture(scope="module")
def idx(ctx):
    names, h, off = synth.clade_sketches(N, 120, 24, strains_per_clade=8, seed=71)
    assert len(names) == N
    return device_index(ctx, h, off, 24)


@pytest.fixture
def options(monkeypatch):
    """options(...) fixes the rk_dist_opts of the capi calls that follow in this test, whatever the method itself would pass (every one
    passes triangle = 1, greedy_rows no row shard)"""
    def fix(triangle=1, D=0.05, row_step=1, row_block=0):
        monkeypatch.setattr(capi, "_opts", lambda *a, **k: capi.DistOpts(triangle, 0, KMER, row_block, D, 0, row_step))
    return fix


def refused(call, ctx, idx, text):
    with pytest.raises(capi.RkError) as e:
        CALLS[call](ctx, idx)
    assert e.value.code == RK_ERR_ARG
    assert str(e.value) == "rabbitkssd error -1: " + text


@pytest.mark.parametrize("call", sorted(CALLS))
def test_triangle_0_is_refused(ctx, idx, options, call):
    options(triangle=0)
    refused(call, ctx, idx, TRIANGLE[call])


@pytest.mark.parametrize("call", sorted(CALLS))
def test_a_row_shard_is_refused_by_the_calls_that_need_every_row(ctx, idx, options, call):
    options(row_step=2, row_block=32)
    if call in EVERY_ROW:
        refused(call, ctx, idx, EVERY_ROW[call])
    else:
        CALLS[call](ctx, idx)


@pytest.mark.parametrize("D", DENSE_D)
@pytest.mark.parametrize("call", sorted(CALLS))
def test_a_dense_report_is_refused_by_all_but_the_clusters(ctx, idx, options, call, D):
    options(D=D)
    if call in DENSE:
        refused(call, ctx, idx, DENSE[call])
    else:
        labels, st = CALLS[call](ctx, idx)
        assert len(labels) == N and len(set(labels.tolist())) == 1 and st["n_clusters"] == 1


@pytest.mark.parametrize("call", sorted(CALLS))
def test_of_two_faults_the_first_in_the_order_is_named(ctx, idx, options, call):
    options(triangle=0, D=1.5)
    refused(call, ctx, idx, TRIANGLE[call])
    if call in EVERY_ROW:
        options(D=1.5, row_step=2, row_block=32)
        refused(call, ctx, idx, EVERY_ROW[call])
