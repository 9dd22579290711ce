"""The side-car of a counted sketch, <path>.sketch.abund, and the report of `rabbit_kssd abund`, restated in numpy from their
description (rabbitkssd_amd/host/formats.hpp) for tests/test_abund_cpu.py and tests/test_gpu_abund.py; and the model of a counted
sketch over tests/_sketch_ref.py: the distinct dr_tuples of a genome's candidate stream with the number of times each occurred."""
import struct

import numpy as np

import _sketch_ref as sr
from oracle import oracle as ok

MAGIC = b"RKABUND1"


def abund_bytes(sizes, counts, magic=MAGIC, n_genomes=None, total=None):
    """the file: magic, u32 n_genomes, u32 0, u64 total, u32 sizes[], u32 counts[], little-endian"""
    sizes, counts = np.asarray(sizes, dtype="<u4"), np.asarray(counts, dtype="<u4")
    head = struct.pack("<8sIIQ", magic, len(sizes) if n_genomes is None else n_genomes, 0, len(counts) if total is None else total)
    return head + sizes.tobytes() + counts.tobytes()


def read_abund(path):
    """(sizes, counts) of a side-car, its header checked"""
    b = open(path, "rb").read()
    magic, n, reserved, total = struct.unpack("<8sIIQ", b[:24])
    assert magic == MAGIC and reserved == 0 and len(b) == 24 + 4 * n + 4 * total, path
    return np.frombuffer(b, dtype="<u4", count=n, offset=24), np.frombuffer(b, dtype="<u4", count=total, offset=24 + 4 * n)


def save_sketches(path, ksl, names, hashes, off):
    (ok.save_sketches64 if ksl[0] - ksl[2] > 8 else ok.save_sketches32)(str(path), ksl[0], ksl[1], ksl[2], names, hashes, off)


def read_sketches(path, ksl):
    """(names, hashes, off)"""
    return (ok.read_sketches64 if ksl[0] - ksl[2] > 8 else ok.read_sketches32)(str(path))[1:]


def report_text(names, off, counts, bins=64):
    """what `abund -i` prints: per genome name, distinct hashes, occurrences, largest count, lower median; then count<TAB>hashes per
    non-empty bin below `bins`, and >=bins for the rest"""
    out = []
    for g, name in enumerate(names):
        c = np.sort(np.asarray(counts[int(off[g]):int(off[g + 1])], dtype=np.uint64))
        n = len(c)
        out.append("%s\t%d\t%d\t%d\t%d" % (name, n, int(c.sum()), int(c[-1]) if n else 0, int(c[(n - 1) // 2]) if n else 0))
        for v in range(1, bins):
            if np.count_nonzero(c == v):
                out.append("%d\t%d" % (v, np.count_nonzero(c == v)))
        if np.count_nonzero(c >= bins):
            out.append(">=%d\t%d" % (bins, np.count_nonzero(c >= bins)))
    return "".join(line + "\n" for line in out)


def counted(ps, genomes, min_count=1, quals=None, least_qual=0):
    """the model of a counted sketch call over genomes [(seq, rec_off)]: (hashes uint64, off uint64, counts uint32) -- per genome the
    distinct candidates that occur at least min_count times, ascending, each with its full count"""
    hs, cs, off = [], [], [0]
    for i, (seq, rec_off) in enumerate(genomes):
        dr = sr.candidates(ps, seq, rec_off, None if quals is None else quals[i], least_qual)[0]
        u, n = np.unique(dr, return_counts=True)
        hs.append(u[n >= min_count])
        cs.append(n[n >= min_count])
        off.append(off[-1] + len(hs[-1]))
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, dtype=t)
    return cat(hs, np.uint64), np.array(off, dtype=np.uint64), cat(cs, np.uint32)
