"""rk_group_sketches on the device against tests/_group_ref.py: the reference's own union and sub outputs, random collections under every
rule and both hash widths, every length class of the list kernels at its seams (read from the call's stats, not copied), the spill, the
retry, the host leg, the round trip into an index, the refusals and `rabbit_kssd group`."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _assign_ref as ar
import _group_ref as gr
from _selfjoin_cases import KMER, TOOL, csr, device_index
from conftest import GOLDEN, ROOT
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth
from test_group_cpu import SKETCHES_ARGTYPES, golden, marked, random_labels, untouched

pytestmark = pytest.mark.gpu
RK_ERR_ARG = -1
NONE = gr.NONE
RULE_NAMES = ("pan", "core", "majority", "markers", "min2")


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def grouped(ctx, idx, labels, rule):
    """the call, in the reference's form, with what every result must satisfy: (group_label, group_size, kept), stats, the object"""
    sk, gl, gs, st = ctx.group_sketches(idx, labels, rule)
    assert st["groups"] == len(gl) == len(gs) and st["labelled"] == sum(l != NONE for l in labels)
    if sk is None:
        assert len(gl) == 0 and st["path"] == 0 and st["kept"] == 0
        return ([], [], []), st, None
    h, off = sk.download()
    assert sk.count == len(gl) and st["kept"] == sk.total == len(h) == off[-1] and sk.is64 == (h.dtype == np.uint64)
    kept = [p.tolist() for p in gr.parts_of(h, off)]
    assert all(all(a < b for a, b in zip(k, k[1:])) for k in kept)   # strictly ascending
    if st["path"] == 1:
        assert st["lane_lists"] + st["wave_lists"] + st["block_lists"] == st["lists"] == idx.distinct and st["postings"] == idx.total
        assert st["spilled"] <= st["block_lists"] and st["attempts"] in (1, 2)
    return (gl.tolist(), gs.tolist(), kept), st, sk


def object_bytes(sk):
    h, off = sk.download()
    return h.tobytes() + off.tobytes()


def index_of(ctx, parts, wide=False, bits=24):
    h, off = csr(parts, np.uint64 if wide else np.uint32)
    return device_index(ctx, h, off, bits, wide)


def imported_index(ctx, parts, wide, bits):
    """the same collection through the oracle's .dict / .index arrays: no sketches, identity genome order"""
    h, off = csr(parts, np.uint64 if wide else np.uint32)
    sizes = np.diff(off).astype(np.uint32)
    if wide:
        uhash, ucount, postings = ok.index_build64(h, off)
        return ctx.index_import64(postings, uhash, ucount, bits, sizes)
    postings, counts = ok.index_build32(h, off, bits)
    return ctx.index_import(postings, counts, bits, sizes)


# ---- 1. the reference's own union and sub ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,how", [("32", "built"), ("32", "imported"), ("64", "built"), ("64", "imported")])
def test_pan_is_the_references_union_and_markers_its_sub(ctx, tag, how):
    ref, qry, union, sub = golden(tag)
    wide, bits = (True, 36) if tag == "64" else (False, 24)
    make = index_of if how == "built" else imported_index
    n = len(ref)
    got, st, _ = grouped(ctx, make(ctx, ref, wide, bits), [0] * n, "pan")
    assert st["path"] == 1 and got == ([0], [n], [union[0].tolist()])
    some = range(len(qry)) if how == "built" else (0, len(qry) - 1)   # (an import of 32-bit hashes uploads the dense 2^24 array)
    for q in some:
        got, st, _ = grouped(ctx, make(ctx, ref + [qry[q]], wide, bits), [0] * n + [n], "markers")
        assert st["path"] == 1 and got[0] == [0, n] and got[1] == [n, 1] and got[2][1] == sorted(int(x) for x in sub[q])


# ---- 2. random collections, every rule, both widths ---------------------------------------------------------------------------------
_clades = {}


def clades(wide):
    """(parts, bits, kmer) of 1,000 genomes in clades of 10, sketches of about 40 hashes, in a shuffled caller order"""
    if wide not in _clades:
        bits, kmer = (36, 24) if wide else (24, 20)
        names, h, off = synth.clade_sketches(1000, 40, bits, kmer_size=kmer, strains_per_clade=10, seed=71 + wide, wide=wide)
        names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=5))
        _clades[wide] = (gr.parts_of(h, off), bits, kmer)
    return _clades[wide]


@pytest.mark.parametrize("wide", [False, True])
def test_random_collections_under_every_rule(ctx, wide):
    parts, bits, kmer = clades(wide)
    n = len(parts)
    idx = index_of(ctx, parts, wide, bits)
    before = ctx.dist_rows(idx, None, 1, 0, kmer, 0.05)[0]
    clustered = ctx.cluster_rows(idx, 0, kmer, 0.05)[0].tolist()
    assert 50 < len(set(clustered)) < n
    drawn = random_labels(np.random.default_rng(9), n)
    assert NONE in drawn and any(l != NONE and drawn[l] != l for l in drawn)
    for labels in (clustered, drawn):
        for name in RULE_NAMES:
            got, st, _ = grouped(ctx, idx, labels, gr.RULES[name])
            assert st["path"] == 1 and got == gr.fast(parts, labels, gr.RULES[name]), name
    assert grouped(ctx, idx, clustered, (2, 3, 2, 1))[0] == gr.fast(parts, clustered, (2, 3, 2, 1))
    after = ctx.dist_rows(idx, None, 1, 0, kmer, 0.05)[0]
    assert len(before) > 1000 and before.tobytes() == after.tobytes()   # the index is unchanged by the calls


# ---- 3. the length classes at their seams ---------------------------------------------------------------------------------------------
N_SEAM = 3000


def constants(ctx):
    st = ctx.group_sketches(index_of(ctx, [np.array([1], dtype=np.uint32)]), [0])[3]
    return st["lane_max"], st["wave_max"], st["table_groups"], st["chunk"]


def seam_collection(lengths, seed):
    """N_SEAM genomes of 6 private hashes each and, per length L, one shared hash held by L random genomes"""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(1 << 22)[: 6 * N_SEAM + len(lengths)].astype(np.uint32)
    parts = [list(pool[6 * v: 6 * v + 6]) for v in range(N_SEAM)]
    shared = pool[6 * N_SEAM:]
    for L, s in zip(lengths, shared):
        for v in rng.choice(N_SEAM, size=L, replace=False):
            parts[v].append(s)
    return [np.sort(np.array(p, dtype=np.uint32)) for p in parts], [int(s) for s in shared]


def test_every_length_class_at_its_seams(ctx):
    lane_max, wave_max, table_groups, chunk = constants(ctx)
    assert 1 <= lane_max < wave_max <= 64 < chunk and table_groups + 2 < N_SEAM and 2 * chunk + 2 < N_SEAM
    # a = the first length (the first number of groups) a class does NOT take
    lengths = sorted({1, 2, N_SEAM} | {a + d for a in (lane_max + 1, wave_max + 1, table_groups + 1, chunk + 1, 2 * chunk + 1) for d in (-1, 0, 1)})
    parts, shared = seam_collection(lengths, 3)
    idx = index_of(ctx, parts)
    assert idx.distinct == 6 * N_SEAM + len(lengths)
    holders = {s: [g for g in range(N_SEAM) if s in parts[g]] for s in shared}
    assert [len(holders[s]) for s in shared] == lengths
    v = np.arange(N_SEAM)
    labellings = {"one": np.full(N_SEAM, 7), "distinct": v, "alternating": v % 2, "runs": v // 7 * 7, "reversed": N_SEAM - 1 - v}
    for name, lab in labellings.items():
        for holes in (False, True):
            labels = [NONE if holes and i % 50 == 11 else int(l) for i, l in enumerate(lab)]   # unlabelled holders defeat markers
            for rule in RULE_NAMES:
                got, st, _ = grouped(ctx, idx, labels, gr.RULES[rule])
                # every class got its lists ...
                assert st["path"] == 1 and st["attempts"] == 1
                assert st["lane_lists"] == 6 * N_SEAM + sum(L <= lane_max for L in lengths)
                assert st["wave_lists"] == sum(lane_max < L <= wave_max for L in lengths)
                assert st["block_lists"] == sum(L > wave_max for L in lengths)
                # ... and the lists with more groups than the table holds were spilled
                want_spilled = sum(L > wave_max and len({labels[g] for g in holders[s]} - {NONE}) > table_groups for L, s in zip(lengths, shared))
                assert st["spilled"] == want_spilled
                assert want_spilled >= (4 if name in ("distinct", "reversed") else 1 if name == "runs" else 0) and (want_spilled == 0) == (name in ("one", "alternating"))
                want = gr.fast(parts, labels, gr.RULES[rule])
                assert got == want, (name, holes, rule)
    # the shared hashes are where the classes differ: under pan with one label every one of them is kept, under markers with
    # holes the long ones are defeated
    got = grouped(ctx, idx, [7] * N_SEAM, "pan")[0]
    assert set(shared) <= set(got[2][0]) and len(got[2][0]) == idx.distinct


def test_repeated_hashes_count_genomes_not_occurrences(ctx):
    lane_max, wave_max, table_groups, chunk = constants(ctx)
    parts, labels, core_traps, marker_keeps = [], [], [], []
    h = 1000
    for half in (2, wave_max // 4, chunk):   # lists of 2 * half postings: one per class
        a = len(parts)
        # group a: 2 * half genomes; only `half` of them hold hash h, each TWICE: c = half < m unless occurrences are counted
        parts += [np.array([h, h, h + 1], dtype=np.uint32)] * half + [np.array([h + 1], dtype=np.uint32)] * half
        labels += [a] * (2 * half)
        core_traps.append((a, h))
        b = len(parts)
        # group b: `half` genomes that all hold hash h + 2 twice and nobody else does: c = t = half unless one of them counts occurrences
        parts += [np.array([h + 2, h + 2, h + 3], dtype=np.uint32)] * half
        labels += [b] * half
        marker_keeps.append((b, h + 2))
        h += 10
    parts.append(np.array([1003, 1013, 1023], dtype=np.uint32))   # an unlabelled holder of every h + 3
    labels.append(NONE)
    idx = index_of(ctx, parts)
    assert idx.total == sum(len(p) for p in parts)   # (the repeats are in the lists)
    core, st, _ = grouped(ctx, idx, labels, "core")
    assert st["path"] == 1 and st["lane_lists"] > 0 and st["wave_lists"] > 0 and st["block_lists"] > 0
    assert core == gr.from_sets(parts, labels, gr.RULES["core"]) == gr.fast(parts, labels, gr.RULES["core"])
    for a, hh in core_traps:
        assert core[2][core[0].index(a)] == [hh + 1]
    markers = grouped(ctx, idx, labels, "markers")[0]
    assert markers == gr.from_sets(parts, labels, gr.RULES["markers"])
    for b, hh in marker_keeps:
        assert markers[2][markers[0].index(b)] == [hh]   # (h + 3 is defeated by the unlabelled holder)


# ---- 4. the retry, the host leg, the timed span ---------------------------------------------------------------------------------------
def test_overflow_of_the_key_buffer_and_of_the_spill_buffer_run_once_more(ctx, monkeypatch):
    lengths = [1, 9, 70, 300, 600]
    parts, shared = seam_collection(lengths, 4)
    idx = index_of(ctx, parts)
    for labels in ([3] * N_SEAM, list(range(N_SEAM))):
        roomy, st, sk = grouped(ctx, idx, labels, "pan")
        assert st["attempts"] == 1 and (labels[0] == 3 or st["spilled"] == 2)
        for switch in ("RK_GROUP_CAP", "RK_GROUP_SPILL_CAP"):
            if switch == "RK_GROUP_SPILL_CAP" and not st["spilled"]:
                continue
            monkeypatch.setenv(switch, "16")
            tight, st2, sk2 = grouped(ctx, idx, labels, "pan")
            monkeypatch.delenv(switch)
            assert st2["attempts"] == 2 and tight == roomy and object_bytes(sk2) == object_bytes(sk)
            assert {k: v for k, v in st2.items() if k != "attempts"} == {k: v for k, v in st.items() if k != "attempts"}


CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from rabbitkssd_amd import capi
import test_gpu_group as t
ctx = capi.Context(0)
parts, bits, kmer = t.clades(False)
idx = t.index_of(ctx, parts, False, bits)
labels = t.child_labels(len(parts))
for rule in ("core", "markers"):
    sk, gl, gs, st = ctx.group_sketches(idx, labels, rule)
    print(rule, st["path"], st["attempts"], hashlib.sha256(t.object_bytes(sk) + gl.tobytes() + gs.tobytes()).hexdigest())
"""


def child_labels(n):
    return [NONE if v % 9 == 4 else (v * 7919) % n // 10 * 10 for v in range(n)]


def test_host_leg_in_a_child_process_gives_the_same_bytes(ctx):
    parts, bits, kmer = clades(False)
    idx = index_of(ctx, parts, False, bits)
    labels = child_labels(len(parts))
    env = dict(os.environ, RK_GROUP_DEVICE="0")
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [line.split() for line in p.stdout.decode().splitlines() if line.split()[:1] in (["core"], ["markers"])]
    assert [l[0] for l in lines] == ["core", "markers"]
    for rule, path, attempts, digest in lines:
        sk, gl, gs, st = ctx.group_sketches(idx, labels, rule)
        assert st["path"] == 1 and int(path) == 2 and int(attempts) == 0
        assert hashlib.sha256(object_bytes(sk) + gl.tobytes() + gs.tobytes()).hexdigest() == digest
        assert grouped(ctx, idx, labels, rule)[0] == gr.fast(parts, labels, gr.RULES[rule])


def test_timed_span_and_the_host_leg_in_process(ctx, monkeypatch):
    parts, bits, kmer = clades(True)
    idx = index_of(ctx, parts, True, bits)
    labels = child_labels(len(parts))
    device, st, sk = grouped(ctx, idx, labels, "majority")
    ctx.set_timing(True)
    grouped(ctx, idx, labels, "majority")
    assert ctx.last_ms(capi.MS_GROUP) > 0.0
    monkeypatch.setenv("RK_GROUP_DEVICE", "0")
    host, st2, sk2 = grouped(ctx, idx, labels, "majority")
    monkeypatch.delenv("RK_GROUP_DEVICE")
    assert ctx.last_ms(capi.MS_GROUP) == 0.0
    ctx.set_timing(False)
    assert st2["path"] == 2 and st2["attempts"] == 0 and host == device and object_bytes(sk2) == object_bytes(sk) and sk2.is64
    assert {k: st2[k] for k in ("lists", "postings", "kept", "labelled", "groups")} == {k: st[k] for k in ("lists", "postings", "kept", "labelled", "groups")}


# ---- 5. the result is a sketches object like any other ---------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_round_trip_into_an_index_a_join_and_a_placement(ctx, wide):
    parts, bits, kmer = clades(wide)
    n = len(parts)
    idx = index_of(ctx, parts, wide, bits)
    labels = ctx.cluster_rows(idx, 0, kmer, 0.05)[0].tolist()
    want, _, sk = grouped(ctx, idx, labels, "pan")
    assert want == gr.fast(parts, labels, gr.RULES["pan"])
    K = len(want[0])
    species = ctx.index_build(sk, bits)
    assert species.genomes == K
    dtype = np.uint64 if wide else np.uint32
    qh, qoff = csr([parts[v] for v in range(0, n, 37)], dtype)
    qs = ctx.sketches_from_host64(qh, qoff) if wide else ctx.sketches_from_host(qh, qoff)
    rh, roff = gr.csr(want[2], dtype)
    sizes = np.diff(roff).astype(np.uint32)
    for metric in (0, 1):
        if wide:
            uhash, ucount, postings = ok.index_build64(rh, roff)
            hits = ok.index_dist64(uhash, ucount, postings, sizes, qh, qoff, 0, metric, kmer, 0.3, threads=4)[0]
        else:
            postings, counts = ok.index_build32(rh, roff, bits)
            hits = ok.index_dist32(counts, bits, postings, sizes, qh, qoff, 0, metric, kmer, 0.3, threads=4)[0]
        mine = ctx.dist_rows(species, qs, 0, metric, kmer, 0.3)[0]
        assert len(hits) >= len(qoff) - 1
        key = lambda r: np.lexsort((r["col"], r["row"]))   # noqa: E731
        for f in ("row", "col", "common", "size0", "size1"):
            assert np.array_equal(mine[f][key(mine)], hits[f][key(hits)]), f
    placed = ctx.assign_rows(species, qs, 1, kmer, 0.3, list(range(K)))
    expect = ar.assign(ar.hit_tuples(hits), len(qoff) - 1, K, list(range(K)), 1)
    assert placed[0].tolist() == expect[0] and placed[1].tolist() == expect[1]
    # a query is a member of a cluster: under containment its own cluster's pan sketch holds all of it
    assert all(want[0][placed[0][q]] == labels[v] for q, v in enumerate(range(0, n, 37)))


# ---- 6. what is refused ---------------------------------------------------------------------------------------------------------------
def raw_call(ctx, idx, labels, rule, skip=None):
    L = capi.lib()
    L.rk_group_sketches.argtypes = SKETCHES_ARGTYPES
    out, k = marked()
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    r = None if rule is None else capi.GroupRule(*rule)
    ptrs = [None if i == skip else C.byref(o) for i, o in enumerate(out[:3])]
    rc = L.rk_group_sketches(ctx._h, idx._h, None if lab is None else lab.ctypes.data, None if r is None else C.byref(r), ptrs[0], ptrs[1], ptrs[2],
                             None if skip == 3 else C.byref(k), C.byref(capi.GroupStats()))
    return rc, untouched(out, k)


def test_arguments_that_are_refused(ctx):
    parts, bits, kmer = clades(False)
    n = len(parts)
    idx = index_of(ctx, parts, False, bits)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    good = (0, 1, 1, 0)
    for wrong in (n, n + 7, 0xFFFFFFFE):
        assert raw_call(ctx, idx, [0] * (n - 1) + [wrong], good) == (RK_ERR_ARG, True) and b"label" in last()
    assert raw_call(ctx, idx, None, good) == (RK_ERR_ARG, True) and b"labels is null" in last()
    for rule in ((0, 0, 1, 0), (2, 1, 1, 0), (0, 1, 0, 0), (0, 1, 1, 2)):
        assert raw_call(ctx, idx, [0] * n, rule) == (RK_ERR_ARG, True) and b"rule" in last()
    assert raw_call(ctx, idx, [0] * n, None) == (RK_ERR_ARG, True)
    for skip in range(4):
        assert raw_call(ctx, idx, [0] * n, good, skip=skip) == (RK_ERR_ARG, True)
    # nothing labelled, and nothing at all: RK_OK, nothing runs
    got, st, sk = grouped(ctx, idx, [NONE] * n, "pan")
    assert sk is None and st["path"] == 0 and st["attempts"] == 0 and st["lists"] == idx.distinct
    # every member's sketch empty: the group exists, its sketch is empty
    got, st, sk = grouped(ctx, index_of(ctx, [np.zeros(0, dtype=np.uint32)] * 2 + [np.array([5], dtype=np.uint32)]), [2, 2, NONE], "core")
    assert got == ([2], [2], [[]]) and sk.count == 1 and sk.total == 0


def test_indexes_without_all_posting_lists_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    n = len(names)
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    assert raw_call(ctx, parts[0], [0] * n, (0, 1, 1, 0)) == (RK_ERR_ARG, True)   # one hash range of a sharded build
    assert b"posting lists" in capi.lib().rk_last_error(ctx._h)
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    recv = torch.cat([bufs[r][: 12 * sent[r][0]] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
    torch.cuda.synchronize()
    j = ctx.index_join_shard(parts[0], recv.data_ptr(), sum(sent[r][0] for r in range(S)))
    assert raw_call(ctx, j, [0] * n, (0, 1, 1, 0)) == (RK_ERR_ARG, True)   # the join-only index: tile records of its rows, no lists
    assert b"posting lists" in capi.lib().rk_last_error(ctx._h)
    del j, parts, sk


# ---- 7. the tool ----------------------------------------------------------------------------------------------------------------------
def run_tool(cwd, args):
    return subprocess.run([TOOL, "group"] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_group_subcommand(ctx, tmp_path):
    import shutil
    ref, qry, union, sub = golden("32")
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "ref.sketch")
    shutil.copy(os.path.join(GOLDEN, "dist", "qry.sketch"), tmp_path / "qry.sketch")
    (tmp_path / "zeros.txt").write_text("0\n" * len(ref))
    p = run_tool(tmp_path, ["-i", "ref.sketch", "--labels", "zeros.txt", "-o", "pan.sketch", "--map", "pan.map"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    info, names, h, off = ok.read_sketches32(str(tmp_path / "pan.sketch"))
    rinfo, rnames, _, _ = ok.read_sketches32(str(tmp_path / "ref.sketch"))
    assert off.tolist() == [0, 1870] and np.array_equal(h, union[0]) and names == [rnames[0]]
    assert (info.half_k, info.half_subk, info.drlevel, info.genomeNumber) == (rinfo.half_k, rinfo.half_subk, rinfo.drlevel, 1)
    assert (tmp_path / "pan.map").read_text() == "1\t0\t%d\t1870\t%s\n" % (len(ref), rnames[0])
    # the output is a .sketch like any other: info reads it, dist takes it as -r
    p = subprocess.run([TOOL, "info", "-i", "pan.sketch", "-o", "pan.info"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and (tmp_path / "pan.info").read_text()
    p = subprocess.run([TOOL, "dist", "-r", "pan.sketch", "-q", "qry.sketch", "-M", "1", "-D", "1.0", "-o", "pan.dist"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert len((tmp_path / "pan.dist").read_text().splitlines()) >= 1
    # --by cluster --core --map against rk_cluster_rows + the reference
    p = run_tool(tmp_path, ["-i", "ref.sketch", "--by", "cluster", "-D", "0.3", "--core", "-o", "core.sketch", "--map", "core.map"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    idx = index_of(ctx, ref)
    labels = ctx.cluster_rows(idx, 0, 2 * rinfo.half_k, 0.3)[0].tolist()
    want = gr.from_sets(ref, labels, gr.RULES["core"])
    assert 1 < len(want[0]) < len(ref)
    first = [labels.index(l) for l in want[0]]
    _, names, h, off = ok.read_sketches32(str(tmp_path / "core.sketch"))
    assert [p_.tolist() for p_ in gr.parts_of(h, off)] == want[2] and names == [rnames[v] for v in first]
    assert (tmp_path / "core.map").read_text() == "".join("%d\t%d\t%d\t%d\t%s\n" % (k + 1, want[0][k], want[1][k], len(want[2][k]), rnames[first[k]]) for k in range(len(want[0])))
    # --share, --min-count, --only travel
    p = run_tool(tmp_path, ["-i", "ref.sketch", "--by", "cluster", "-D", "0.3", "--share", "1/2", "--min-count", "2", "--only", "-o", "m.sketch"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _, _, h, off = ok.read_sketches32(str(tmp_path / "m.sketch"))
    assert [p_.tolist() for p_ in gr.parts_of(h, off)] == gr.from_sets(ref, labels, (1, 2, 2, 1))[2]
    # what dies, with a message, before a file is written
    for args, text in ((["-i", "ref.sketch"], b"needs -i and -o"), (["-o", "x.sketch"], b"needs -i"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--by", "cluster", "--labels", "zeros.txt"], b"exclude each other"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--by", "kmeans"], b"--by must be"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--pan", "--core"], b"exclude each other"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--share", "3/2"], b"--share needs P/Q"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--share", "half"], b"--share needs P/Q"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--min-count", "0"], b"--min-count must be >= 1"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--gpus", "2"], b"one GPU"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "--by", "dbscan", "-m", "0"], b"minPts must be >= 1"),
                       (["-i", "ref.sketch", "-o", "x.sketch", "-D", "1.0"], b"below 1.0")):
        p = run_tool(tmp_path, args)
        assert p.returncode != 0 and text in p.stderr and not (tmp_path / "x.sketch").exists(), args
    (tmp_path / "short.txt").write_text("0\n" * (len(ref) - 1))
    p = run_tool(tmp_path, ["-i", "ref.sketch", "--labels", "short.txt", "-o", "x.sketch"])
    assert p.returncode != 0 and b"command_group()" in p.stderr and not (tmp_path / "x.sketch").exists()
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"group -i" in p.stderr and b" dist group union " in p.stderr
