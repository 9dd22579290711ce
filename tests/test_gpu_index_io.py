"""What moves a finished index in or out (rk_index_io.hip): the single-buffer blob of rk_index_pack_dev / rk_index_unpack_dev, the
imports and the exports.

The blob's layout is asserted from a second source: this file holds its own copy of the 168-byte header (a numpy structured dtype)
and of the layout rule (sections 256-byte aligned, from 256 on, in the order postings, uhash, upos, sizes, [orig], [src],
[self, selfoff, split]), and compares what a packed buffer says field by field -- never whole buffers: the pad between sections is
not written.  Five indexes between them have every optional section once and lack it once.  A damaged blob, a file whose counts do
not add up and an export of the wrong width are refused with their present texts.  Collections are tiny (41 genomes of at most 80
hashes); every comparison is of integers or of doubles computed on the host: no tolerance."""

import numpy as np
import pytest

from oracle import oracle as ok
from rabbitkssd_amd import capi

pytestmark = pytest.mark.gpu
KMER = 20
BITS32, BITS64 = 20, 36
KNOBS = ("RK_INDEX_FAST", "RK_INDEX_RELABEL", "RK_INDEX_NO_SELF", "RK_INDEX_TILES", "RK_DIST_TILES", "RK_DIST_TILES_MIN_GENOMES")
MAGIC = int.from_bytes(b"RSKDIDX7", "little")
OFFSETS = ("off_postings", "off_uhash", "off_upos", "off_sizes", "off_self", "off_selfoff", "off_src", "off_split", "off_orig")
HEADER = np.dtype([(n, "<u8") for n in ("magic", "bytes", "H", "U", "max_src_size", "max_ref_size", "min_ref_size", "n_self")] +
                  [(n, "<u4") for n in ("n_ref", "has_self", "ref_sets", "relabeled")] +
                  [(n, "<i4") for n in ("hash_bits", "wide", "has_src")] + [("pad", "<u4")] + [(n, "<u8") for n in OFFSETS])
assert HEADER.itemsize == 168


def al256(x):
    return (x + 255) & ~255


def layout(H, U, n_ref, n_self, wide, relabeled, has_src, has_self):
    """(offset of every section -- 0: absent --, bytes of the blob)"""
    off = dict.fromkeys(OFFSETS, 0)
    p = 256

    def put(name, nbytes):
        nonlocal p
        off[name] = p
        p = al256(p + nbytes)
    put("off_postings", (H + 1) * 4)
    put("off_uhash", (U + 1) * (8 if wide else 4))
    put("off_upos", (U + 2) * 4)
    put("off_sizes", (n_ref + 1) * 4)
    if relabeled:
        put("off_orig", (n_ref + 1) * 4)
    if has_src:
        put("off_src", (n_ref + 1) * 8)
    if has_self:
        put("off_self", (n_self + 1) * 8)
        put("off_selfoff", (n_ref + 1) * 8)
        put("off_split", (n_ref + 1) * 8)
    return off, p


_COLLECTIONS = {}


def collection(wide):
    """41 genomes of 30..80 hashes: two clades of near-copies (non-empty slice records) dealt over the singletons, one empty genome;
    with it the oracle's index, computed once: (hashes, offsets, postings, distinct hashes, list lengths, dense counts or None)"""
    if wide in _COLLECTIONS:
        return _COLLECTIONS[wide]
    rng = np.random.default_rng(64 if wide else 32)
    bits = BITS64 if wide else BITS32

    def draw(n):
        return np.unique(rng.integers(0, 1 << bits, size=n, dtype=np.uint64))
    sets = []
    for members in (9, 7):
        base = draw(76)
        for m in range(members):
            keep = base[rng.random(len(base)) < 0.9][: 30 + int(rng.integers(0, 45))]
            sets.append(np.unique(np.concatenate([keep, draw(3 + m)])))
    while len(sets) < 40:
        sets.append(draw(30 + int(rng.integers(0, 51))))
    sets = [sets[i] for i in rng.permutation(40)]
    sets.insert(17, np.zeros(0, dtype=np.uint64))
    assert all(len(s) <= 80 for s in sets) and min(len(s) for s in sets if len(s)) >= 25
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.uint64)
    h = np.concatenate(sets).astype(np.uint64 if wide else np.uint32)
    if wide:
        assert int(h.max()) >= 1 << 32
        uhash, ucount, postings = ok.index_build64(h, off)
        counts = None
    else:
        postings, counts = ok.index_build32(h, off, bits)
        uhash, ucount = np.flatnonzero(counts).astype(np.uint64), counts[counts > 0]
    H, U = len(h), len(uhash)
    assert H % 64 and U % 64 and H - U > 64, (H, U)       # (neither a multiple of the block; slice records to ship)
    for a in (h, off, postings, uhash, ucount, counts):
        if a is not None:
            a.setflags(write=False)
    _COLLECTIONS[wide] = (h, off, postings, uhash, ucount, counts)
    return _COLLECTIONS[wide]


class Case:
    """one index, the context it lives in, and what the test knows about it without asking the library"""

    def __init__(self, name, monkeypatch):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        self.name = name
        self.wide = name == "b"
        self.built = name != "e"
        self.h, self.off, self.postings, self.uhash, self.ucount, self.counts = collection(self.wide)
        self.bits = BITS64 if self.wide else BITS32
        self.sizes = np.diff(self.off.astype(np.int64)).astype(np.uint32)
        if name == "c":
            monkeypatch.setenv("RK_INDEX_NO_SELF", "1")
        if name == "d":
            monkeypatch.setenv("RK_INDEX_RELABEL", "0")
        self.ctx = capi.Context(0)      # (reads the switches)
        if self.built:
            self.sk = self.ctx.sketches_from_host64(self.h, self.off) if self.wide else self.ctx.sketches_from_host(self.h, self.off)
            self.idx = self.ctx.index_build(self.sk, self.bits)
        else:
            self.idx = self.ctx.index_import(self.postings, self.counts, self.bits, self.sizes)
        H, U = len(self.h), len(self.ucount)
        self.want = {"magic": MAGIC, "H": H, "U": U, "max_src_size": int(self.sizes.max()) if self.built else 0,
                     "max_ref_size": int(self.sizes.max()), "min_ref_size": int(self.sizes[self.sizes > 0].min()),
                     "n_ref": len(self.sizes), "has_self": int(name in "abd"), "ref_sets": 1, "relabeled": int(name in "abc"),
                     "hash_bits": self.bits, "wide": int(self.wide), "has_src": int(self.built)}
        self.want["n_self"] = H - U if self.want["has_self"] else 0    # (sets: every member of a list but its last has a slice)

    def pack(self):
        import torch
        n = self.idx.blob_bytes
        blob = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.idx.pack_dev(blob.data_ptr(), n)
        torch.cuda.synchronize()
        return blob

    def close(self):
        del self.idx
        self.ctx.close()


def header_of(blob):
    return np.frombuffer(blob[:HEADER.itemsize].cpu().numpy().tobytes(), dtype=HEADER)[0]


def exports(idx, wide):
    if wide:
        return idx.export64()
    return idx.export() + idx.export_lists()


def assert_hits_equal(mine, want, what):
    assert len(mine) == len(want), "%s: %d hits against %d" % (what, len(mine), len(want))
    for f in ("row", "col", "common", "size0", "size1", "jorc", "dist"):
        assert np.array_equal(mine[f], want[f]), "%s: %s" % (what, f)


@pytest.mark.parametrize("name", "abcde")
def test_blob_header_layout_and_round_trip(monkeypatch, name):
    import torch
    case = Case(name, monkeypatch)
    try:
        idx, c = case.idx, case.ctx
        assert idx.products & 1 == case.want["has_self"]
        blob = case.pack()
        n = idx.blob_bytes
        # ---- the header, field by field, and the offsets from this file's own rule
        hd = header_of(blob)
        for f, v in case.want.items():
            assert int(hd[f]) == v, "%s: %s is %d, not %d" % (name, f, int(hd[f]), v)
        off, total = layout(case.want["H"], case.want["U"], case.want["n_ref"], case.want["n_self"], case.wide,
                            case.want["relabeled"], case.want["has_src"], case.want["has_self"])
        for f in OFFSETS:
            assert int(hd[f]) == off[f], "%s: %s is %d, not %d" % (name, f, int(hd[f]), off[f])
        assert int(hd["bytes"]) == total == n
        absent = [f for f in OFFSETS if off[f] == 0]
        assert absent == {"a": [], "b": [], "c": ["off_self", "off_selfoff", "off_split"], "d": ["off_orig"],
                          "e": ["off_self", "off_selfoff", "off_src", "off_split", "off_orig"]}[name]
        # ---- what the sections carry, where this file can say it: the lists and the sizes
        raw = blob.cpu().numpy()

        def section(f, dtype, count):
            return np.frombuffer(raw[off[f]: off[f] + count * np.dtype(dtype).itemsize].tobytes(), dtype=dtype)
        H, U, N = case.want["H"], case.want["U"], case.want["n_ref"]
        order = idx.order
        if not case.want["relabeled"]:
            assert np.array_equal(order, np.arange(N))
        upos = section("off_upos", "<u4", U + 1)
        assert np.array_equal(np.diff(upos.astype(np.int64)), case.ucount) and upos[0] == 0 and upos[U] == H
        assert np.array_equal(section("off_uhash", "<u8" if case.wide else "<u4", U).astype(np.uint64), case.uhash)
        assert np.array_equal(section("off_sizes", "<u4", N), case.sizes[order])
        if case.want["relabeled"]:
            assert np.array_equal(section("off_orig", "<u4", N), order)
        if case.want["has_src"]:
            assert np.array_equal(section("off_src", "<u8", N + 1), np.concatenate([[0], np.cumsum(case.sizes[order].astype(np.uint64))]))
        posts = order[section("off_postings", "<u4", H)]       # (a list's genomes ascend by internal id: sort each by the caller's)
        assert np.array_equal(posts[np.lexsort((posts, np.repeat(np.arange(U), case.ucount)))], case.postings)
        # ---- the copy agrees with the original
        copy = c.index_unpack_dev(blob.data_ptr(), n)
        for mine, want in zip(exports(copy, case.wide), exports(idx, case.wide)):
            assert np.array_equal(mine, want)
        assert np.array_equal(copy.order, order)
        assert (copy.total, copy.distinct, copy.genomes, copy.hash_bits) == (idx.total, idx.distinct, idx.genomes, idx.hash_bits) == (H, U, N, case.bits)
        assert copy.products & 1 == idx.products & 1
        assert copy.blob_bytes == n
        if case.built:
            want_hits = c.dist_rows(idx, None, 1, 0, KMER, 0.05)[0]
            assert len(want_hits) > 10
            assert_hits_equal(c.dist_rows(copy, None, 1, 0, KMER, 0.05)[0], want_hits, name)
        del copy
        torch.cuda.synchronize()
    finally:
        case.close()


def test_a_damaged_blob_is_refused(monkeypatch):
    import torch
    case = Case("a", monkeypatch)
    try:
        idx, c = case.idx, case.ctx
        blob = case.pack()
        n = idx.blob_bytes
        hd = header_of(blob)
        word = {f: HEADER.fields[f][1] for f in HEADER.names}     # byte offset of every field

        def refused(damaged, text, nbytes=n):
            torch.cuda.synchronize()
            with pytest.raises(capi.RkError, match=text):
                c.index_unpack_dev(damaged.data_ptr(), nbytes)

        def with_u32(byte_off, value):
            d = blob.clone()
            d[byte_off: byte_off + 4] = torch.from_numpy(np.array([value], dtype="<u4").view(np.uint8).copy()).cuda()
            return d

        def with_u64(byte_off, value):
            d = blob.clone()
            d[byte_off: byte_off + 8] = torch.from_numpy(np.array([value], dtype="<u8").view(np.uint8).copy()).cuda()
            return d
        c.index_unpack_dev(blob.data_ptr(), n).close()         # (the undamaged blob is taken)
        # what rk_index_unpack_dev checks before it sizes anything
        foreign = "not an index blob of this library"
        refused(blob, foreign, n - 1)
        refused(with_u64(word["magic"], MAGIC ^ 1), foreign)
        refused(with_u64(word["off_upos"], int(hd["off_upos"]) + 256), foreign)
        refused(with_u32(word["wide"], 1), foreign)
        # payload values that k_validate_blob reads in bounds
        corrupt = "inconsistent with its header"
        N, H = case.want["n_ref"], case.want["H"]
        refused(with_u32(int(hd["off_postings"]) + 4 * (H // 2), N), corrupt)
        refused(with_u32(int(hd["off_orig"]) + 4 * 5, N), corrupt)
        raw = blob.cpu().numpy()
        split1 = int(np.frombuffer(raw[int(hd["off_split"]) + 8: int(hd["off_split"]) + 16].tobytes(), dtype="<u8")[0])
        refused(with_u64(int(hd["off_selfoff"]) + 8, split1 + 1), corrupt)
        # a buffer one byte short
        short = torch.empty(n - 1, dtype=torch.uint8, device="cuda")
        with pytest.raises(capi.RkError, match="blob needs"):
            idx.pack_dev(short.data_ptr(), n - 1)
        torch.cuda.synchronize()
    finally:
        case.close()


def test_import_and_export_refusals(monkeypatch):
    narrow, wide = Case("a", monkeypatch), Case("b", monkeypatch)
    try:
        c = narrow.ctx
        # a file whose counts do not add up to its postings; a hash twice
        counts = narrow.counts.copy()
        counts[np.flatnonzero(counts)[3]] += 1
        with pytest.raises(capi.RkError, match="mismatched total"):
            c.index_import(narrow.postings, counts, narrow.bits, narrow.sizes)
        twice = wide.uhash.copy()
        twice[1] = twice[0]
        with pytest.raises(capi.RkError, match="duplicate hash in the index file"):
            c.index_import64(wide.postings, twice, wide.ucount, wide.bits, wide.sizes)
        ucount = wide.ucount.copy()
        ucount[3] += 1
        with pytest.raises(capi.RkError, match="mismatched total"):
            c.index_import64(wide.postings, wide.uhash, ucount, wide.bits, wide.sizes)
        # an export of the other width (the dense array of a 36-bit space is never allocated: the refusal comes first)
        postings, some_counts = np.zeros(wide.idx.total, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
        rc = capi.lib().rk_index_export(wide.idx._h, capi._ptr(postings), capi._ptr(some_counts))
        with pytest.raises(capi.RkError, match=r"64-bit index: use rk_index_export64 \(sparse \.index layout\)"):
            wide.ctx.check(rc)
        with pytest.raises(capi.RkError, match=r"32-bit index: use rk_index_export \(dense \.index layout\)"):
            narrow.idx.export64()
        with pytest.raises(capi.RkError, match=r"64-bit index: use rk_index_export64$"):
            wide.idx.export_lists()
        assert np.array_equal(wide.idx.export(want_counts=False)[0], wide.postings)      # (postings alone: any width)
    finally:
        narrow.close()
        wide.close()


def test_export_under_renumbering(monkeypatch):
    narrow, wide = Case("a", monkeypatch), Case("b", monkeypatch)
    try:
        order = narrow.idx.order
        assert not np.array_equal(order, np.arange(len(order)))       # (the clades were dealt over the collection: it IS renumbered)
        postings, counts = narrow.idx.export()
        lp, lh, lc = narrow.idx.export_lists()
        assert np.array_equal(postings, lp) and np.array_equal(postings, narrow.postings)
        assert np.array_equal(counts, narrow.counts)
        assert np.array_equal(lh, narrow.uhash) and np.array_equal(lc, narrow.ucount)
        assert not np.array_equal(wide.idx.order, np.arange(len(order)))
        p64, h64, c64 = wide.idx.export64()
        assert np.array_equal(p64, wide.postings) and np.array_equal(h64, wide.uhash) and np.array_equal(c64, wide.ucount)
    finally:
        narrow.close()
        wide.close()
