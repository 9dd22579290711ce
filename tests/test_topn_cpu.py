"""CPU checks of `dist -N` on the device (rk_dist_topn, rabbitkssd_amd/csrc/rk_topn.hip): the entry point is exported and
refuses bad arguments without a GPU, and a numpy model of its selection kernel -- the same rule, the same margins -- keeps
a subsequence of every distance stream below over which the reference's heap (capi.topn_rows) ends exactly as it does over
the whole stream ("dist -N on the device")."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rabbitkssd_amd import capi

THREADS, PER = 256, 4                   # k_topn_select: cells per step before / after N certain cells are known
DIST_MARGIN, JORC_MARGIN = 2.0 ** -40, 2.0 ** -20


def test_dist_topn_is_exported_and_refuses_null_pointers():
    """Without a GPU there is no context: only the null-pointer checks can be reached here (the refusal of triangle = 1 needs
    a context and is tested on the GPU, tests/test_gpu_topn.py::test_triangle_is_refused)."""
    L = capi.lib()
    assert hasattr(L, "rk_dist_topn") and "rk_dist_topn" in capi.EXPORTS
    hits, n = C.c_void_p(), C.c_uint64()
    opts = capi.DistOpts(0, 0, 20, 0, 1.0, 0, 1)
    assert L.rk_dist_topn(None, None, None, C.byref(opts), C.c_uint64(5), C.byref(hits), C.byref(n)) == -1
    assert L.rk_dist_topn(None, None, None, None, C.c_uint64(5), None, None) == -1


def test_model_constants_are_the_kernels():
    """The model below restates k_topn_select's rule; its step sizes and margins are read back from the kernel's source,
    so that the two cannot drift apart unnoticed."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rabbitkssd_amd", "csrc",
                            "rk_topn.hip")).read()
    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1).strip()
    assert int(const("kSelThreads")) == THREADS and int(const("kSelPer")) == PER
    assert float.fromhex(const("kDistMargin")) == DIST_MARGIN and float.fromhex(const("kJorcMargin")) == JORC_MARGIN
    assert "1024 + 16 * max_neighbor" in src and "std::min<uint64_t>(R, " in src   # the candidate room per row


def host_distance(common, size0, size1, metric, k):
    """rk_distance (src/dist.cpp:218-231 / :239-252), vectorised: the 'host' values of the model."""
    common, size0, size1 = (np.asarray(x, dtype=np.int64) for x in (common, size0, size1))
    denom = np.minimum(size0, size1) if metric else size0 + size1 - common
    zero = (size0 == 0) | (size1 == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        j = np.where(zero, 0.0, common / np.where(denom == 0, 1, denom).astype(np.float64))
        x = j if metric else (2 * j) / (1.0 + j)
        d = (-1.0 / k) * np.log(np.where(j > 0, x, 1.0))
    d = np.where(j == 1.0, 0.0, np.where(j == 0.0, 1.0, d))
    return j, d


def jorc_below(d, metric, k):
    t = np.exp(-float(k) * d)
    return (t if metric else t / (2.0 - t)) * (1.0 - JORC_MARGIN)


def select_model(common, size0, size1, metric, k, D, N, dev_dist):
    """k_topn_select over one row: the columns it emits.  dev_dist: the device's own distance of every cell (its log may
    differ from the host's in the last bits)."""
    R = len(common)
    emitted = []
    best = np.zeros(0)
    lo = jorc_below(D, metric, k)
    c0 = 0
    while c0 < R:
        full = len(best) >= N
        top = best[N - 1] if full else np.inf
        jt = jorc_below(top, metric, k) if full else 0.0
        c1 = min(R, c0 + THREADS * (PER if full else 1))
        c, s0, s1 = (np.asarray(x[c0:c1], dtype=np.int64) for x in (common, size0, size1))
        zero = (c == 0) | (s0 == 0) | (s1 == 0)
        denom = (np.minimum(s0, s1) if metric else s0 + s1 - c).astype(np.float64)
        live = zero | ~((c < lo * denom) | (full & (c < jt * denom)))
        d = dev_dist[c0:c1]
        m = np.abs(d) * DIST_MARGIN
        dl = np.where(zero, 1.0, d - m)
        du = np.where(zero, 1.0, d + m)
        emit = live & (dl <= D) & ((not full) | (dl < top))
        add = live & (du <= D) & ((not full) | (du < top))
        emitted.extend((c0 + np.nonzero(emit)[0]).tolist())
        best = np.sort(np.concatenate([best, du[add]]))[:N]
        c0 = c1
    return np.array(emitted, dtype=np.int64)


def replay_check(common, size0, size1, metric, k, D, N, rng):
    R = len(common)
    j, h = host_distance(common, size0, size1, metric, k)
    # the device's log: the host value moved by up to 3 ulps either way (exact where the special cases apply)
    steps = rng.integers(-3, 4, size=R)
    dev = h.copy()
    for s in range(1, 4):
        dev = np.where((steps >= s) & (j > 0) & (j < 1), np.nextafter(dev, np.inf), dev)
        dev = np.where((steps <= -s) & (j > 0) & (j < 1), np.nextafter(dev, -np.inf), dev)
    rec = np.zeros(R, dtype=capi.HIT_DTYPE)
    rec["row"] = 7
    rec["col"] = np.arange(R)
    rec["common"], rec["size0"], rec["size1"], rec["jorc"], rec["dist"] = common, size0, size1, j, h
    stream = rec[h <= D]                                         # src/dist.cpp:624: the cells the heap sees
    want = capi.topn_rows(stream, N)
    sel = select_model(common, size0, size1, metric, k, D, N, dev) if N else np.zeros(0, dtype=np.int64)
    cand = rec[sel]
    got = capi.topn_rows(cand[cand["dist"] <= D], N)             # the host finish: exact threshold, then the heap
    assert got.tobytes() == want.tobytes(), (metric, D, N, len(sel))
    return len(sel)


def stream_random(rng, R):
    size1 = int(rng.integers(2000, 60000))
    size0 = rng.integers(20, 3000, size=R)
    common = np.minimum(size0, rng.geometric(0.3, size=R) - 1)
    common[rng.random(R) < 0.3] = 0                               # no shared hash: exactly 1.0
    hot = rng.random(R) < 0.02                                    # relatives: a large share
    common[hot] = (size0[hot] * rng.random(hot.sum())).astype(np.int64)
    return common, size0, np.full(R, size1)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("N", [1, 3, 100, 1024])
def test_model_random_order(metric, N):
    rng = np.random.default_rng(11 + N + metric)
    for D in (1.0, 1.5, 1e9):
        common, size0, size1 = stream_random(rng, 20000)
        n_sel = replay_check(common, size0, size1, metric, 20, D, N, rng)
        if N <= 3:
            assert n_sel < 256 + 600          # one step of single cells, then ~N ln(R / 256) improvements


@pytest.mark.parametrize("N", [1, 3, 100, 1024])
def test_model_strictly_decreasing_distance(N):
    """Every cell beats every earlier one: the heap takes all of them, the model must emit all of them."""
    rng = np.random.default_rng(3)
    R = 3000
    common = np.arange(1, R + 1)
    n_sel = replay_check(common, np.full(R, R + 10), np.full(R, 40000), 0, 20, 1.0, N, rng)
    assert n_sel == R


@pytest.mark.parametrize("N", [1, 3, 100, 1024])
def test_model_ten_thousand_ties_at_one(N):
    """Unrelated sketches at -D 1.0: every cell at exactly 1.0, the heap keeps the first N; the model emits the first step."""
    rng = np.random.default_rng(4)
    R = 10000
    n_sel = replay_check(np.zeros(R, dtype=np.int64), rng.integers(1, 500, size=R), np.full(R, 5000), 0, 20, 1.0, N, rng)
    assert n_sel <= max(THREADS, -(-N // THREADS) * THREADS) + THREADS * PER


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("N", [1, 3, 100, 1024])
def test_model_interior_ties(metric, N):
    """Few distinct (common, sizes) triples repeated in random order: ties at interior distances everywhere."""
    rng = np.random.default_rng(5 + N)
    R = 12000
    pick = rng.integers(0, 6, size=R)
    common = np.array([0, 3, 7, 7, 20, 50])[pick]
    size0 = np.array([100, 100, 100, 200, 100, 400])[pick]
    replay_check(common, size0, np.full(R, 900), metric, 20, 1.0, N, rng)


@pytest.mark.parametrize("N", [1, 3, 100, 1024])
def test_model_zero_common_next_to_distances_above_one(N):
    """common == 0 is exactly 1.0; a tiny positive jaccard has mashD > 1.0 (not monotone there): with -D 1.05 some of those
    are in the stream, some not, and all of them sit around the 1.0 cells."""
    rng = np.random.default_rng(6)
    R = 8000
    common = rng.integers(0, 2, size=R)
    size1 = rng.choice([2_000_000_000, 25_000_000, 12_000_000, 100], size=R)
    size0 = np.full(R, 1)
    j, h = host_distance(common, size0, size1, 0, 16)
    assert (h > 1.0).any() and ((h > 1.0) & (h <= 1.05)).any() and (h > 1.05).any() and (h == 1.0).any()
    for D in (1.0, 1.05, 1.2):
        replay_check(common, size0, size1, 0, 16, D, N, rng)


def test_model_more_neighbours_than_columns_and_none():
    rng = np.random.default_rng(8)
    common, size0, size1 = stream_random(rng, 300)
    assert replay_check(common, size0, size1, 0, 20, 1.0, 1000, rng) == 300
    replay_check(common, size0, size1, 0, 20, 1.0, 0, rng)
