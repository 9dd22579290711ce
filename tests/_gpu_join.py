"""What the GPU suites of the self join share: a context with developer switches, exact comparison of hits, row shards, and the
records rk_dist_rows_dev leaves in a device buffer with a guard behind it."""
import numpy as np

from rabbitkssd_amd import capi

# developer switches that are read when a context is created: make_ctx clears every one of them before a leg, so that no leg
# inherits another's
CREATION = ("RK_INDEX_RELABEL", "RK_DIST_TILES", "RK_INDEX_TILES", "RK_DIST_NEAR", "RK_DIST_NEAR_UW", "RK_DIST_PAIR",
            "RK_DIST_BAND_MIN_ROWS", "RK_DIST_LDS_KB", "RK_DIST_ROWS", "RK_DIST_PERSIST", "RK_DIST_THREADS", "RK_DIST_CAND_CAP",
            "RK_DIST_STAGE_HITS", "RK_DIST_XCD_ROWS", "RK_DIST_BANDS", "RK_DIST_DEBUG")
REC = capi.HIT_DTYPE.itemsize
GUARD = 4096               # bytes of a known pattern behind every device hit buffer


def make_ctx(monkeypatch, env, relabel=False):
    """a context with these developer switches (they are read when it is created) and, unless `relabel`, the caller's order"""
    env = dict(env)
    if not relabel:
        env["RK_INDEX_RELABEL"] = "0"
    for k in CREATION:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in CREATION
        monkeypatch.setenv(k, v)
    ctx = capi.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


def assert_hits_equal(mine, want):
    """as tests/test_gpu_parity.py: integers equal, jorc and dist bit for bit (rk_dist_rows)"""
    assert len(mine) == len(want), (len(mine), len(want))
    for f in ("row", "col", "common", "size0", "size1"):
        assert np.array_equal(mine[f], want[f]), f
    assert np.array_equal(mine["jorc"], want["jorc"])
    assert np.array_equal(mine["dist"], want["dist"])


def join(ctx, idx, metric, D, k, **shard):
    return ctx.dist_rows(idx, None, 1, metric, k, D, **shard)[0]


def assert_shards(ctx, idx, metric, D, k, want, shards):
    for step, block in shards:
        parts = [join(ctx, idx, metric, D, k, row_first=r, row_step=step, row_block=block) for r in range(step)]
        for r, p in enumerate(parts):
            assert np.all(idx.shard_of(p, step, block) == r)
        merged = np.concatenate(parts)
        assert_hits_equal(merged[np.lexsort((merged["col"], merged["row"]))], want)


def pairs_of(hits):
    return set(zip(hits["row"].tolist(), hits["col"].tolist()))


def dev_records(ctx, idx, qs, triangle, metric, D, k, cap, **shard):
    """(*n_hits_dev, the min(n, cap) records by (row, col)) of rk_dist_rows_dev; the guard behind the buffer must be untouched"""
    import torch
    buf = torch.full((cap * REC + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.dist_rows_dev(idx, triangle, metric, k, D, buf.data_ptr(), cap, cnt.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream, queries=qs, **shard)
    torch.cuda.synchronize()
    n = int(cnt.item())
    raw = buf.cpu().numpy()
    assert np.all(raw[cap * REC:] == 0xA5), "bytes behind hits_cap were written"
    got = np.frombuffer(raw[: min(n, cap) * REC].tobytes(), dtype=capi.HIT_DTYPE)
    return n, got[np.lexsort((got["col"], got["row"]))]


def check_dev(dev, want):
    """device records against the reference: integers and jorc equal, dist within 1e-12 (the device's own log)"""
    assert len(dev) == len(want)
    for f in ("row", "col", "common", "size0", "size1", "pad", "jorc"):
        assert np.array_equal(dev[f], want[f]), f
    assert np.max(np.abs(dev["dist"] - want["dist"]), initial=0.0) <= 1e-12


def assert_capped_records(n, got, want, cap, n_cols):
    """rk_dist_rows_dev over its capacity: *n_hits_dev counts every hit, the `cap` records written are distinct members of the
    result"""
    assert n == len(want) and len(got) == cap
    wkey = want["row"].astype(np.int64) * n_cols + want["col"]
    gkey = got["row"].astype(np.int64) * n_cols + got["col"]
    assert len(np.unique(gkey)) == cap                          # no record twice
    at = np.searchsorted(wkey, gkey)
    assert np.all(at < len(wkey)) and np.array_equal(wkey[np.minimum(at, len(wkey) - 1)], gkey)
    check_dev(got, want[at])
