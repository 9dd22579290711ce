"""rk_sketches_mask_counts on the device: the hashes, offsets and stats of rk_sketches_mask byte for byte and every survivor with its own
count (tests/_mask_ref.py says who survives) -- totals around a tile and around a 64-lane seam, 36-bit hashes, every band of
tests/test_gpu_mask.py's edge list, the host leg; the result goes into rk_screen_abund_rows and rk_index_build; one record of the screen
with abundances against the masked counts of that reference alone; what is refused; `rabbit_kssd mask --abund`."""
import ctypes as C
import os
import shutil
import statistics
import subprocess

import numpy as np
import pytest

import _mask_ref as mk
import _screen_abund_ref as ar
from _screen_cases import index_of
from _selfjoin_cases import TOOL, csr
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi

pytestmark = pytest.mark.gpu
BANDS = ar.MASK_BANDS
assert BANDS[:2] == [mk.SUB, mk.PRESENT]
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def counted(ctx, queries, wide=False):
    """counted sketches from dicts hash -> count"""
    dtype = np.uint64 if wide else np.uint32
    hs = [np.array(sorted(m), dtype=dtype) for m in queries]
    h, off = csr(hs, dtype)
    c = np.array([m[int(x)] for m, p in zip(queries, hs) for x in p], dtype=np.uint32)
    return ctx.sketches_from_host_counts(h, c, off, wide=wide)


def masked(ctx, qs, idx, refs, queries, band, path=1):
    """the call, compared with rk_sketches_mask on the same sketches and with the model; returns the masked sketches"""
    out, st = ctx.sketches_mask_counts(qs, idx, *band)
    plain, st0 = ctx.sketches_mask(qs, idx, *band)
    (h, off), (h0, off0) = out.download(), plain.download()
    assert h.tobytes() == h0.tobytes() and off.tobytes() == off0.tobytes() and st == st0 and st["path"] == path
    assert out.has_counts and not plain.has_counts
    want = mk.fast(refs, [sorted(m) for m in queries], *band)
    assert [p.tolist() for p in mk.parts_of(h, off)] == want
    assert out.download_counts().tolist() == [m[x] for m, k in zip(queries, want) for x in k]
    return out


def random_case(rng, wide, n_hashes):
    """4 references and queries over one pool, so that every band has survivors; n_hashes: the query sizes"""
    top = (1 << 36) if wide else (1 << 24)
    pool = np.unique(rng.integers(0, top, size=sum(n_hashes) + 4000, dtype=np.uint64))
    refs = [rng.choice(pool, size=len(pool) // 4, replace=False) for _ in range(4)]
    queries = [{int(h): int(c) for h, c in zip(rng.choice(pool, size=n, replace=False), rng.integers(1, 2 ** 32, size=n, dtype=np.uint64))} for n in n_hashes]
    return refs, queries


@pytest.mark.parametrize("wide", [False, True])
def test_totals_around_a_tile_and_a_lane_seam_through_every_band(ctx, wide):
    rng = np.random.default_rng(50 + wide)
    one = ctx.sketches_mask(ctx.sketches_from_host(np.array([1], dtype=np.uint32), np.array([0, 1], dtype=np.uint64)),
                            index_of(ctx, [np.array([1], dtype=np.uint32)]), 0, 0)[1]
    T = one["tile_hashes"]
    for total in (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 65):
        sizes = [total] if total < 100 else [total // 3, 0, total - total // 3 - 7, 7]   # one sketch, or boundaries inside the tiles
        refs, queries = random_case(rng, wide, sizes)
        idx = index_of(ctx, [np.sort(r).astype(np.uint64 if wide else np.uint32) for r in refs], wide, 36 if wide else 24)
        qs = counted(ctx, queries, wide)
        for band in (BANDS if total in (65, T + 1) else BANDS[:2]):
            out = masked(ctx, qs, idx, refs, queries, band)
            assert out.total <= total


def test_the_host_leg_gives_the_same_arrays(ctx, monkeypatch):
    rng = np.random.default_rng(60)
    for wide in (False, True):
        refs, queries = random_case(rng, wide, [300, 0, 2500, 1])
        idx = index_of(ctx, [np.sort(r).astype(np.uint64 if wide else np.uint32) for r in refs], wide, 36 if wide else 24)
        qs = counted(ctx, queries, wide)
        for band in BANDS:
            dev = masked(ctx, qs, idx, refs, queries, band)
            monkeypatch.setenv("RK_MASK_DEVICE", "0")
            host = masked(ctx, qs, idx, refs, queries, band, path=2)
            monkeypatch.delenv("RK_MASK_DEVICE")
            assert dev.download_counts().tobytes() == host.download_counts().tobytes() and dev.download()[0].tobytes() == host.download()[0].tobytes()


def test_the_result_goes_into_the_screen_with_abundances_and_the_index_build(ctx):
    rng = np.random.default_rng(70)
    refs, queries = random_case(rng, False, [400, 900, 0, 50])
    refs = [np.sort(r).astype(np.uint32) for r in refs]
    idx = index_of(ctx, refs)
    host = index_of(ctx, [refs[3]])   # "remove the host, then screen": the queries lose what reference 3 holds
    qs = counted(ctx, queries)
    left = masked(ctx, qs, host, [refs[3]], queries, mk.SUB)
    kept = [{h: c for h, c in m.items() if h not in set(refs[3].tolist())} for m in queries]
    got = ctx.screen_abund_rows(idx, left)
    w_off, w_recs, w_abund, w_matched, w_cand, w_claimed, w_occ = ar.as_arrays(ar.fast(refs, kept), refs, kept)
    assert got[0].tolist() == w_off and ar.abund_tuples(got[2]) == w_abund and got[6].tolist() == w_occ and len(w_abund) >= 6
    assert all(int(r["ref"]) != 3 for r in got[1])
    built = ctx.index_build(left, 24)   # the counts do not stand in the way of any other consumer
    assert built.genomes == 4 and built.total == left.total
    # one reference r alone under {1, UINT32_MAX}: the survivors are what the query shares with r -- their counts' sum and lower median are
    # occ_common and med_common of r's record
    off, recs, abund = ctx.screen_abund_rows(idx, qs)[:3]
    for r in range(4):
        shared = ctx.sketches_mask_counts(qs, index_of(ctx, [refs[r]]), *mk.PRESENT)[0]
        c, o = shared.download_counts(), shared.download()[1]
        for q in range(len(queries)):
            mine = [i for i in range(int(off[q]), int(off[q + 1])) if recs[i]["ref"] == r]
            values = c[int(o[q]):int(o[q + 1])].tolist()
            assert len(mine) == (1 if values else 0)
            if values:
                assert (int(abund[mine[0]]["occ_common"]), int(abund[mine[0]]["med_common"])) == (sum(values), statistics.median_low(values))


def test_what_is_refused_and_the_empty_cases(ctx):
    refs = [np.array([3, 5, 9], dtype=np.uint32)]
    idx = index_of(ctx, refs)
    plain = ctx.sketches_from_host(np.array([3, 4], dtype=np.uint32), np.array([0, 2], dtype=np.uint64))
    L = capi.lib()
    L.rk_sketches_mask_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.MaskRule), C.POINTER(C.c_void_p), C.POINTER(capi.MaskStats)]
    out = C.c_void_p(0x1234)
    r = capi.MaskRule(0, 0)
    assert L.rk_sketches_mask_counts(ctx._h, plain._h, idx._h, C.byref(r), C.byref(out), None) == RK_ERR_UNSUPPORTED and out.value == 0x1234
    assert b"counts" in L.rk_last_error(ctx._h)
    with pytest.raises(capi.RkError) as e:
        ctx.sketches_mask_counts(plain, idx)
    assert e.value.code == RK_ERR_UNSUPPORTED
    qs = counted(ctx, [{3: 7, 4: 2}])
    bad = capi.MaskRule(2, 1)
    assert L.rk_sketches_mask_counts(ctx._h, qs._h, idx._h, C.byref(bad), C.byref(out), None) == RK_ERR_ARG and out.value == 0x1234
    for skip in (1, 2, 3, 4):
        args = [ctx._h, qs._h, idx._h, C.byref(r), C.byref(out), None]
        args[skip] = None
        assert L.rk_sketches_mask_counts(*args) == RK_ERR_ARG and out.value == 0x1234
    none_q = ctx.sketches_from_host_counts(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    assert ctx.sketches_mask_counts(none_q, idx)[0] is None   # no query sketch: nothing runs
    gone = masked(ctx, counted(ctx, [{3: 7, 9: 1}, {}]), idx, refs, [{3: 7, 9: 1}, {}], mk.SUB)   # nothing survives: counts all the same
    assert gone.total == 0 and gone.has_counts and len(gone.download_counts()) == 0


def test_tool_mask_abund_then_abund(ctx, tmp_path):
    """`mask --abund` writes out.sketch.abund, which `abund` reads: per query its survivors, their occurrences, the largest and the lower
    median of their counts; and what dies without the side-car"""
    _, rh, roff = ok.read_sketches32(os.path.join(GOLDEN, "dist", "ref.sketch"))[1:]
    _, qnames, qh, qoff = ok.read_sketches32(os.path.join(GOLDEN, "dist", "qry.sketch"))
    refs, queries = mk.parts_of(rh, roff), mk.parts_of(qh, qoff)
    for name in ("ref.sketch", "qry.sketch"):
        shutil.copy(os.path.join(GOLDEN, "dist", name), tmp_path / name)
    qd = ar.with_counts(queries, np.random.default_rng(9))
    ar.write_abund(tmp_path / "qry.sketch.abund", [len(q) for q in queries], [qd[i][int(h)] for i, q in enumerate(queries) for h in q])
    for extra, band in ((["--keep", "present"], mk.PRESENT), ([], mk.SUB)):
        p = subprocess.run([TOOL, "mask", "-r", "ref.sketch", "-q", "qry.sketch", "--abund", "-o", "out.sketch"] + extra, cwd=tmp_path, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        p = subprocess.run([TOOL, "abund", "-i", "out.sketch", "-o", "report.txt", "--bins", "1"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        want = mk.fast(refs, [sorted(int(h) for h in q) for q in queries], *band)
        lines = [x for x in (tmp_path / "report.txt").read_text().splitlines() if not x.startswith(">=")]
        assert sum(len(k) for k in want) > 100
        assert lines == ["%s\t%d\t%d\t%d\t%d" % (qnames[q], len(k), sum(qd[q][h] for h in k), max([qd[q][h] for h in k], default=0),
                                                  statistics.median_low([qd[q][h] for h in k]) if k else 0) for q, k in enumerate(want)]
        plain = subprocess.run([TOOL, "mask", "-r", "ref.sketch", "-q", "qry.sketch", "-o", "plain.sketch"] + extra, cwd=tmp_path, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE)
        assert plain.returncode == 0 and (tmp_path / "plain.sketch").read_bytes() == (tmp_path / "out.sketch").read_bytes()   # the sketches: today's
        assert not (tmp_path / "plain.sketch.abund").exists()
    os.remove(tmp_path / "qry.sketch.abund")
    p = subprocess.run([TOOL, "mask", "-r", "ref.sketch", "-q", "qry.sketch", "--abund", "-o", "x.sketch"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--abund needs the occurrence counts" in p.stderr and b"qry.sketch.abund" in p.stderr and not (tmp_path / "x.sketch").exists()
