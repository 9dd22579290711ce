"""Counted sketches without a GPU: the new symbols of the C ABI, the side-car file <path>.sketch.abund and its reader's refusals
(tools/abund_file_check.cpp under the sanitizers), and the host subcommand `rabbit_kssd abund` on .sketch files and side-cars that
the test writes itself (tests/_abund_ref.py), in both hash widths: the report against the same statistics in numpy, the threshold
at the edges of its band, every refusal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _abund_ref as ab
from conftest import ROOT
from rabbitkssd_amd import capi

TOOL = os.path.join(ROOT, "rabbitkssd_amd", "rabbit_kssd")
RK_ERR_ARG = -1
NEW = ("rk_sketch_batch_counts", "rk_sketch_packed_dev_counts", "rk_sketches_has_counts", "rk_sketches_counts_dev",
       "rk_sketches_download_counts", "rk_sketches_from_host_counts")


def test_the_new_symbols_resolve_and_refuse_null_pointers():
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(L, name), name
    out = C.c_void_p()
    one = np.zeros(1, dtype=np.uint64)
    assert L.rk_sketches_has_counts(None) == 0
    assert L.rk_sketches_counts_dev(None) is None
    assert L.rk_sketches_download_counts(None, one.ctypes.data_as(C.c_void_p)) == RK_ERR_ARG
    # no context, no filter, no output (a context needs a GPU: these are refused before anything is touched)
    assert L.rk_sketches_from_host_counts(None, None, 0, None, one.ctypes.data_as(C.c_void_p), 0, C.byref(out)) == RK_ERR_ARG
    assert L.rk_sketch_batch_counts(None, None, None, None, 0, 1, one.ctypes.data_as(C.c_void_p), 0, one.ctypes.data_as(C.c_void_p), 0,
                                    C.byref(out)) == RK_ERR_ARG
    assert L.rk_sketch_packed_dev_counts(None, None, None, 0, None, None, 0, 1, None, C.byref(out)) == RK_ERR_ARG
    assert out.value is None


def compile_check(exe, extra=()):
    return subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "rabbitkssd_amd", "host"), "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"),
                           os.path.join(ROOT, "tools", "abund_file_check.cpp"), "-o", exe, "-lz", "-lpthread"], capture_output=True, text=True)


def test_the_file_check_is_clean_under_the_sanitizers(tmp_path):
    """writer, reader and its refusals, report, threshold and the counted pass's layout (which leaves the uncounted offsets alone):
    the program checks itself; here it must also leave AddressSanitizer and UBSan silent"""
    exe = str(tmp_path / "abund_file_check")
    p = compile_check(exe, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"))
    sanitized = p.returncode == 0
    if not sanitized:
        assert "cannot find" in p.stderr or "unrecognized" in p.stderr, p.stderr[-4000:]   # a compiler without the runtimes: plain
        p = compile_check(exe)
    assert p.returncode == 0, p.stderr[-4000:]
    work = tmp_path / "files"
    work.mkdir()
    p = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stderr[-4000:]
    assert int(p.stdout.split()[1]) > 100
    assert not any(m in p.stderr for m in ("AddressSanitizer", "runtime error", "LeakSanitizer")), p.stderr[-4000:]
    assert sanitized, "built without -fsanitize=address,undefined: this compiler lacks the runtimes"


def tool(args, ok_expected=True):
    p = subprocess.run([TOOL] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (p.returncode == 0) == ok_expected, p.stderr.decode()[-2000:]
    return p


def hand_made(ksl, rng):
    """names, hashes (ascending per genome), off, counts: five genomes, two of them empty, counts on both sides of every bin edge"""
    wide = ksl[0] - ksl[2] > 8
    sizes = [300, 0, 1, 0, 77]
    names = ["g%d.fa" % i for i in range(len(sizes))]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    top = (1 << 40) if wide else (1 << 24)
    hashes = np.concatenate([np.unique(rng.integers(0, top, 2 * n))[:n] for n in sizes]).astype(np.uint64 if wide else np.uint32)
    assert len(hashes) == off[-1]
    counts = rng.choice([1, 1, 1, 2, 2, 3, 5, 8, 62, 63, 64, 65, 100, 5000, 0xFFFFFFFF], int(off[-1])).astype(np.uint32)
    counts[:8] = [1, 2, 3, 63, 64, 65, 4, 5]
    return names, hashes, off, counts


@pytest.mark.parametrize("ksl", [(8, 5, 2), (11, 5, 2)])
def test_abund_report_threshold_and_refusals(tmp_path, ksl):
    rng = np.random.default_rng(sum(ksl))
    names, hashes, off, counts = hand_made(ksl, rng)
    sk = tmp_path / "x.sketch"
    ab.save_sketches(sk, ksl, names, hashes, off)
    sizes = np.diff(off.astype(np.int64))
    (tmp_path / "x.sketch.abund").write_bytes(ab.abund_bytes(sizes, counts))
    # ---- the report: stdout and -o, default bins and others
    assert tool(["abund", "-i", sk]).stdout.decode() == ab.report_text(names, off, counts, 64)
    for bins in (1, 2, 4, 64, 65, 101):
        tool(["abund", "-i", sk, "--bins", bins, "-o", tmp_path / "rep.txt"])
        assert (tmp_path / "rep.txt").read_text() == ab.report_text(names, off, counts, bins), bins
    text = ab.report_text(names, off, counts, 64)
    assert ">=64\t" in text and "\n63\t" in text and "g1.fa\t0\t0\t0\t0\n" in text   # the model itself reaches the edges
    # ---- the threshold at the edges of its band
    for lo, hi in ((1, None), (2, None), (2, 2), (3, 64), (64, 64), (65, 0xFFFFFFFF), (0xFFFFFFFF, None), (6, 7)):
        args = ["abund", "-i", sk, "--min-count", lo, "-o", tmp_path / "y.sketch"] + (["--max-count", hi] if hi is not None else [])
        for stale in ("y.sketch.dict", "y.sketch.index"):
            assert not (tmp_path / stale).exists()
        tool(args)
        keep = (counts >= lo) & (counts <= (hi if hi is not None else 0xFFFFFFFF))
        assert np.any(keep) or (lo, hi) == (6, 7)
        got_names, got_h, got_off = ab.read_sketches(tmp_path / "y.sketch", ksl)
        got_sizes, got_counts = ab.read_abund(tmp_path / "y.sketch.abund")
        want_sizes = np.array([np.count_nonzero(keep[int(off[g]):int(off[g + 1])]) for g in range(len(names))])
        assert got_names == names and np.array_equal(np.diff(got_off.astype(np.int64)), want_sizes) and np.array_equal(got_sizes, want_sizes)
        assert np.array_equal(got_h, hashes[keep]) and got_h.dtype == hashes.dtype and np.array_equal(got_counts, counts[keep])
        assert (tmp_path / "y.sketch").read_bytes()[:20] == sk.read_bytes()[:20]   # the same header
        assert not (tmp_path / "y.sketch.dict").exists() and not (tmp_path / "y.sketch.index").exists()
    tool(["abund", "-i", sk, "--max-count", 2, "-o", tmp_path / "z.sketch"])      # --max-count alone: from 1
    assert np.array_equal(ab.read_abund(tmp_path / "z.sketch.abund")[1], counts[counts <= 2])
    # ---- refusals of the options
    for args in (["--min-count", 0], ["--min-count", -3], ["--min-count", 3, "--max-count", 2], ["--min-count", 2], ["--bins", 0]):
        with_out = ["-o", tmp_path / "no.sketch"] if args != ["--min-count", 2] else []
        p = tool(["abund", "-i", sk] + args + with_out, ok_expected=False)
        assert b"ERROR" in p.stderr and not (tmp_path / "no.sketch").exists()
    # ---- refusals of the side-car, each naming the file
    side = tmp_path / "x.sketch.abund"
    good = side.read_bytes()
    n, total = len(sizes), len(counts)
    zero = counts.copy()
    zero[total // 2] = 0
    swapped = sizes.copy()
    swapped[[0, 4]] = swapped[[4, 0]]
    for bad, word in ((None, "cannot open"), (ab.abund_bytes(sizes, counts, magic=b"RKABUND2"), "magic"), (good[:-4], "length"), (good + b"\0" * 4, "length"),
                      (good[:20], "magic"), (ab.abund_bytes(sizes, counts, total=total - 1), "length"),
                      (ab.abund_bytes(np.append(sizes, 0), counts), "number of genomes"), (ab.abund_bytes(sizes[:-2], counts[:-77]), "number of genomes"),
                      (ab.abund_bytes(swapped, counts), "size"), (ab.abund_bytes(sizes, zero), "count of 0")):
        if bad is None:
            side.unlink()
        else:
            side.write_bytes(bad)
        for args in ([], ["--min-count", 1, "-o", tmp_path / "no.sketch"]):
            p = tool(["abund", "-i", sk] + args, ok_expected=False)
            assert word in p.stderr.decode() and str(side) in p.stderr.decode(), p.stderr.decode()
            assert not (tmp_path / "no.sketch").exists()
    p = tool(["abund"], ok_expected=False)
    assert b"abund needs -i" in p.stderr
