"""rabbitkssd_amd/host/sketch_input.hpp (the host pipeline of `rabbit_kssd sketch` in front of the GPU) as plain C++:
tools/sketch_input_check.cpp, compiled here with g++, runs the two streamed readers of a big file with a sink of plain memory, at
inputs of a few hundred bytes and pieces of a few bytes, and prints the batch plan of a list.

The criterion is the rule the code states -- every window is seen exactly once: the k-byte windows without a 0x00 byte of the sink's
buffer [0, used) and of RecordReader::parse_packed over the whole text (pinned to the reference's kseq by tests/golden/kseq) are the
same multiset.  Every put is 1 KiB-aligned in offset and length and stays inside the capacity of the last grow, and every byte of
[0, used) was written (the sink poisons what it hands out: padding that is not zero, or a stale byte of a reused ring buffer, shows).
A reader may decline instead -- the tool then takes the whole-file path -- but only for the reasons it documents: where none of them
holds a decline is a failure, where one holds it is required.

The batch plan is compared with the statements sketch_list had inline before the header, rewritten below in the order they stood
there -- not with numbers recorded from the program."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tools", "sketch_input_check.cpp")
MIB = 1 << 20


def compile_check(exe, extra=()):
    return subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "rabbitkssd_amd", "host"), SRC, "-o", exe, "-lz", "-lpthread"], capture_output=True, text=True)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("sketch_input")


@pytest.fixture(scope="module")
def exe(work):
    path = str(work / "sketch_input_check")
    p = compile_check(path)
    assert p.returncode == 0, p.stderr
    return path


def run_cases(exe, work, cases, env=None, name="cases.txt"):
    """{case line: (verdict, {key: value})} of one run of the program"""
    (work / name).write_text("".join(c + "\n" for c in cases))
    e = {k: v for k, v in os.environ.items() if not k.startswith("RK_")}
    e.update(env or {})
    p = subprocess.run([exe, str(work / name)], capture_output=True, text=True, env=e)
    assert p.returncode == 0, p.stderr[-4000:]
    out = {}
    for line in p.stdout.splitlines():
        case, result = line.split(" : ", 1)
        words = result.split()
        out[case] = (words[0], dict(w.split("=", 1) for w in words[1:] if "=" in w), result)
    assert list(out) == list(dict.fromkeys(cases)), p.stderr[-4000:]
    return out, p.stderr


# ------------------------------------------------------------------------------------------ inputs
def fasta_text(k, seed):
    """records of 1, k-2, k-1, k, k+1 and 3k bases in lines of 1, k-1, k and 60 characters, a header directly after a header, an
    empty line inside a record, a last line without a newline"""
    rng = np.random.default_rng(seed)
    out, n_rec = [], 0
    for width in (1, k - 1, k, 60):
        for n in (1, k - 2, k - 1, k, k + 1, 3 * k):
            bases = bytes(rng.choice(list(b"ACGTacgtN"), n).tolist())
            lines = [bases[i:i + width] for i in range(0, n, width)]
            if n == 3 * k and width < n:
                lines.insert(len(lines) // 2, b"")                    # an empty line inside the record
            n_rec += 1
            out.append(b">r%d w%d\n" % (n_rec, width) + b"\n".join(lines) + b"\n")
        out.append(b">empty%d\n" % width)                             # a header directly after the next record's header
    return b"".join(out)[:-1] + b"\n>last\n" + b"ACGT" * (k // 4)            # ... and no newline at the end


def narrow_fasta_text(k, seed):
    """lines of at most 3 characters, headers included: the sequential reader takes pieces of 4 bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for r, n in enumerate((1, k - 1, k, k + 1, 2, 3 * k, k - 2)):
        bases = bytes(rng.choice(list(b"ACGT"), n).tolist())
        width = 1 + r % 3
        out.append(b">%d\n" % r + b"\n".join(bases[i:i + width] for i in range(0, n, width)) + b"\n")
    return b"".join(out)


def fastq_text(seed, eol=b"\n"):
    """four-line records of 20 to 45 bases; quality lines that start with '@' and with '+', '+name' lines, qualities on both sides
    of the gate at 50"""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(40):
        n = int(rng.integers(20, 46))
        bases = bytes(rng.choice(list(b"ACGTN"), n, p=[0.24, 0.24, 0.24, 0.24, 0.04]).tolist())
        qual = bytearray(rng.choice([45, 60, 65, 70], n, p=[0.04, 0.32, 0.32, 0.32]).tolist())
        if r % 3 == 0:
            qual[0] = ord("@")
        if r % 3 == 1:
            qual[0] = ord("+")
        out.append(b"@read%d/1" % r + eol + bases + eol + (b"+read%d/1" % r if r % 4 == 0 else b"+") + eol + bytes(qual) + eol)
    return b"".join(out)


def gz_variants(text):
    """single member; three members, the last one the smallest"""
    c1 = len(text) // 2
    c2 = max(c1, len(text) - 7)
    return {"gz1": gzip.compress(text, mtime=0),
            "gz3": gzip.compress(text[:c1], mtime=0) + gzip.compress(text[c1:c2], mtime=0) + gzip.compress(text[c2:], mtime=0)}


def lines_of(text):
    ls = text.split(b"\n")
    return ls[:-1] if text.endswith(b"\n") else ls


def clean_fasta(text):
    """a text the streamed FASTA readers have no documented reason to refuse (its size aside)"""
    return text.startswith(b">") and b"\r" not in text and not any(l[:1] in (b"+", b"@") for l in lines_of(text))


def four_line_fastq(text):
    ls = [l.rstrip(b"\r") for l in lines_of(text)]
    return (len(ls) >= 4 and len(ls) % 4 == 0 and text.endswith(b"\n") and
            all(ls[i][:1] == b"@" and ls[i + 2][:1] == b"+" and len(ls[i + 1]) == len(ls[i + 3]) > 0 for i in range(0, len(ls), 4)))


def longest_record(text):
    ls = text.split(b"\n")
    return max([sum(len(l) + 1 for l in ls[i:i + 4]) for i in range(0, len(ls) - 1, 4)], default=0)


def mapped_pieces(text, piece):
    """the cuts of a mapped file as the tool made them before the header (sketch_big_fasta_streamed): the line start behind the first newline at or after
    `piece` bytes behind the cut before"""
    cuts = [0]
    while cuts[-1] < len(text):
        p = min(len(text), cuts[-1] + piece)
        if p < len(text):
            e = text.find(b"\n", p)
            p = e + 1 if e >= 0 else len(text)
        cuts.append(p)
    return len(cuts) - 1


# ------------------------------------------------------------------------------------------ the streamed readers
MUST, MAY, DECLINE = "must agree", "may decline", "must decline"


def collect(work):
    """[(case line, expectation, note)]: every input at its piece sizes through the readers that take it"""
    cases = []
    n_file = [0]

    def put(name, data):
        n_file[0] += 1
        p = work / ("%03d_%s" % (n_file[0], name))
        p.write_bytes(data)
        return str(p)

    def fasta(name, text, ks, pieces_of, why_not=None):
        path = put(name, text)
        clean = clean_fasta(text)
        longest = max([len(l) for l in lines_of(text)], default=0)
        variants = dict({"plain": path}, **{v: put(name + "." + v + ".gz", d) for v, d in gz_variants(text).items()})
        for k in ks:
            for piece in pieces_of(k) + [len(text) + 100]:
                want = why_not or (MUST if clean and len(text) >= 64 else DECLINE if clean and len(text) < 64 else MAY)
                cases.append(("mapped %s %d %d 3" % (path, k, piece), want, name))
                want = why_not or (MAY if not clean else MUST if piece >= longest + 1 else DECLINE)
                for v, f in variants.items():
                    cases.append(("seq %s fa 0 %d %d 3 %d" % (f, k, piece, 64 * 1024), want, name + " " + v))

    def fastq(name, text, pieces, gates=(0,)):
        path = put(name, text)
        four = four_line_fastq(text)
        variants = dict({"plain": path}, **{v: put(name + "." + v + ".gz", d) for v, d in gz_variants(text).items()})
        for gate in gates:
            for piece in pieces + [len(text) + 100]:
                want = MUST if four and piece >= 2 * longest_record(text) else MAY
                for v, f in variants.items():
                    cases.append(("seq %s fq %d 16 %d 3 %d" % (f, gate, piece, 64 * 1024), want, name + " " + v))

    fa_pieces = lambda k: [1, 2, k - 1, k, k + 1, 61]
    # the committed fixtures
    for d, ks in (("kseq", (4, 16)), ("sketch", (16, 32))):
        for f in sorted(os.listdir(os.path.join(GOLDEN, d))):
            text = open(os.path.join(GOLDEN, d, f), "rb").read()
            if f.endswith(".fa"):
                fasta(f, text, ks, fa_pieces if len(text) < 1000 else (lambda k: fa_pieces(k) + [997]))
            elif f.endswith(".fq"):
                fastq(f, text, [len(text) // 2, 61], gates=(0, 60))
    # the byte strings of test_cli.test_record_reader_edge_cases
    edge = {"empty.fa": b"", "header_only.fa": b">x", "header_nl.fa": b">x\n", "one_base.fa": b">x\nA", "cr_only.fa": b">x\nA\r\nC\r\n",
            "blank_lines.fa": b"\n\n>a desc\n\nACGT\n\nAC\n>b\n>c\nTT", "leading_junk.fa": b"junk\n>a\nACGT\n",
            "gt_in_seq.fa": b">a\nAC\n>\nGG\n"}
    for name, text in edge.items():
        fasta("edge_" + name, text, (4,), fa_pieces)
    fastq("edge_fq.fq", b"@r\nACGT\n+\nIIII\n@r2\nAC\n+r2\nII\n", [8, 16, 24], gates=(0, 74))
    # generated texts
    for k in (16, 32):
        fasta("gen_k%d.fa" % k, fasta_text(k, k), (k,), fa_pieces)
        fasta("narrow_k%d.fa" % k, narrow_fasta_text(k, 100 + k), (k,), lambda k: [4, 5, k + 1])
    for eol, tag in ((b"\n", "lf"), (b"\r\n", "crlf")):
        text = fastq_text(7, eol)
        rec = longest_record(text)
        fastq("gen_%s.fq" % tag, text, [2 * rec, 3 * rec, 5 * rec], gates=(0, 50))
    # the refusals, each on a text that is fine otherwise
    body = b"".join(b">r%d\n%s\n" % (i, b"ACGTTGCA" * 5) for i in range(6))
    assert clean_fasta(body) and len(body) > 200
    fasta("refuse_crlf.fa", body.replace(b"\n", b"\r\n"), (16,), lambda k: [61], why_not=DECLINE)
    fasta("refuse_junk.fa", b"junk\n" + body, (16,), lambda k: [61], why_not=DECLINE)
    fasta("refuse_at_line.fa", body[:90] + b"@r\n" + body[90:], (16,), lambda k: [61], why_not=DECLINE)
    assert body[89:90] == b"\n"
    fasta("size_63.fa", (b">s\n" + b"ACGT" * 15)[:62] + b"\n", (16,), lambda k: [7, 61])     # mapped: under 64 bytes; sequential: line of 59
    fasta("size_64.fa", (b">s\n" + b"ACGT" * 15)[:63] + b"\n", (16,), lambda k: [7, 61])
    # a first piece of exactly 1,024 packed bytes: no padding follows it, and the next piece starts with bases
    full = b">x\n" + b"".join(b"ACGTTGCAAGCTTGCATGCAGTCAGTCAGTACGATCGATCGTAGCTAGCTAGCATCGATCGACT"[:64] + b"\n" for _ in range(20))
    path = put("kib.fa", full)
    cases.append(("seq %s fa 0 16 %d 2 %d" % (path, 3 + 16 * 65, 1024), MUST, "kib.fa"))
    # a device capacity of 1 KiB: the buffer grows several times, what was put before survives
    multi = os.path.join(GOLDEN, "sketch", "multi_record.fa")
    assert clean_fasta(open(multi, "rb").read())
    cases.append(("seq %s fa 0 16 997 3 1024" % multi, MUST, "growth"))
    return cases


@pytest.fixture(scope="module")
def streamed(exe, work):
    cases = collect(work)
    got, _ = run_cases(exe, work, [c for c, _, _ in cases])
    return cases, got


def check_agrees(case, fields, raw):
    assert fields["completed"] == "1", (case, raw)
    assert fields["unaligned"] == fields["beyond"] == fields["shrunk"] == "0", (case, raw)      # the rules of a put
    assert fields["unwritten"] == "0" and int(fields["used"]) % 1024 == 0 and int(fields["used"]) <= int(fields["cap"]), (case, raw)
    assert fields["got"] == fields["want"], (case, raw)                                          # every window exactly once


def test_every_window_is_seen_exactly_once_or_the_reader_declines_for_a_reason(streamed):
    cases, got = streamed
    seen = {MUST: 0, MAY: 0, DECLINE: 0}
    for case, want, note in cases:
        verdict, fields, raw = got[case]
        seen[want] += 1
        if verdict == "declined":
            assert want != MUST, (case, note)
            assert fields["completed"] == "0", (case, note)      # nothing usable was delivered
        else:
            assert want != DECLINE, (case, note)
            check_agrees(case, fields, raw)
    assert min(seen.values()) > 20, seen


def test_the_cases_reach_their_edges(streamed):
    """conditions on the cases themselves"""
    cases, got = streamed
    by_note = lambda note, what: [(c, got[c]) for c, _, n in cases if n == note and c.startswith(what)]
    for k in (16, 32):
        text = fasta_text(k, k)
        lens = []
        for l in lines_of(text):
            if l.startswith(b">"):
                lens.append(0)
            else:
                lens[-1] += len(l)
        want_windows = sum(max(0, n - k + 1) for n in lens)
        assert sorted(set(lens))[:6] == [0, 1, k - 2, k - 1, k, k + 1] and b"\n\n" in text and not text.endswith(b"\n")
        runs = by_note("gen_k%d.fa" % k, "mapped")
        assert len(runs) == 7
        for c, (verdict, fields, _) in runs:                      # the digest's count is the count by hand
            assert verdict == "ok" and int(fields["want"].split(",")[0]) == want_windows > 0, c
        pieces = [int(f["pieces"]) for _, (_, f, _) in runs]
        assert pieces == [mapped_pieces(text, p) for p in (1, 2, k - 1, k, k + 1, 61, len(text) + 100)]
        assert pieces[0] == len(lines_of(text)) - text.count(b"\n\n") and pieces[-1] == 1   # a piece of 1 byte: every non-empty line a piece
        assert [v for _, (v, _, _) in by_note("gen_k%d.fa plain" % k, "seq")] == ["declined"] * 5 + ["ok", "ok"]   # lines of 60: pieces from 61
        assert [v for _, (v, _, _) in by_note("narrow_k%d.fa gz3" % k, "seq")] == ["ok"] * 4
        assert int(by_note("narrow_k%d.fa plain" % k, "seq")[0][1][1]["pieces"]) > 20
    for tag in ("lf", "crlf"):
        for v in ("plain", "gz1", "gz3"):
            runs = by_note("gen_%s.fq %s" % (tag, v), "seq")
            assert [x for _, (x, _, _) in runs] == ["ok"] * 8 and int(runs[0][1][1]["pieces"]) >= 10
            gate_off, gate_on = (int(runs[i][1][1]["want"].split(",")[0]) for i in (0, 4))
            assert 0 < gate_on < gate_off                          # the quality gate zeroes some bases, not all
    for name in ("refuse_crlf.fa", "refuse_junk.fa", "refuse_at_line.fa"):
        for what in ("mapped", "seq"):
            assert {v for n in (name, name + " plain", name + " gz1", name + " gz3") for _, (v, _, _) in by_note(n, what)} == {"declined"}
    assert [v for _, (v, _, _) in by_note("size_63.fa", "mapped")] == ["declined"] * 3
    assert [v for _, (v, _, _) in by_note("size_64.fa", "mapped")] == ["ok"] * 3
    assert [v for _, (v, _, _) in by_note("size_63.fa plain", "seq")] == ["declined", "ok", "ok"]   # a line of 59 in pieces of 7
    (_, (verdict, fields, _)), = by_note("kib.fa", "seq")
    assert verdict == "ok" and fields["pieces"] == "2" and fields["used"] == "3072"   # 1,024 bytes and their separator: 2 KiB
    (_, (verdict, fields, _)), = by_note("growth", "seq")
    assert verdict == "ok" and int(fields["grows"]) >= 5 and int(fields["cap"]) >= 24 * 1024


# ------------------------------------------------------------------------------------------ sanitizers (host code, this program only)
# (the runtimes are linked statically: the program then needs nothing of the order in which shared libraries are loaded)
@pytest.mark.parametrize("flags,marks", [(("-fsanitize=thread", "-static-libtsan"), ("ThreadSanitizer",)),
                                         (("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"),
                                          ("AddressSanitizer", "runtime error", "LeakSanitizer"))])
def test_the_threads_are_clean_under_a_sanitizer(work, flags, marks):
    path = str(work / ("check" + flags[0].replace("-fsanitize=", "_").replace(",", "_")))
    p = compile_check(path, flags)
    if p.returncode != 0 and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no runtime for %s: %s" % (flags[0], p.stderr.strip().splitlines()[-1]))
    assert p.returncode == 0, p.stderr
    fa = work / "san.fa"
    fa.write_bytes(fasta_text(16, 5) + b"\n" + narrow_fasta_text(16, 6))
    narrow = work / "san_narrow.fa.gz"
    narrow.write_bytes(gz_variants(narrow_fasta_text(32, 8))["gz3"])
    fq = work / "san.fq"
    fq.write_bytes(fastq_text(9))
    rec = longest_record(fastq_text(9))
    cases = []
    for threads in (1, 2, 8):
        cases += ["mapped %s 16 1 %d" % (fa, threads), "mapped %s 16 17 %d" % (fa, threads), "seq %s fa 0 16 61 %d 1024" % (fa, threads),
                  "seq %s fa 0 32 4 %d 1024" % (narrow, threads), "seq %s fq 50 16 %d %d 1024" % (fq, 2 * rec, threads)]
    e = {k: v for k, v in os.environ.items() if not k.startswith("RK_")}
    (work / "san_cases.txt").write_text("".join(c + "\n" for c in cases))
    p = subprocess.run([path, str(work / "san_cases.txt")], capture_output=True, text=True, env=e)
    assert p.returncode == 0 and not any(m in p.stderr for m in marks), p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(cases)
    for line in lines:
        case, result = line.split(" : ", 1)
        fields = dict(w.split("=", 1) for w in result.split()[1:])
        assert result.startswith("ok "), line
        check_agrees(case, fields, result)
        assert int(fields["pieces"]) >= 10, line


# ------------------------------------------------------------------------------------------ the batch plan: the parent's statements, by hand
def packed_bound(path):
    sz = os.path.getsize(path)
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b" and sz >= 18:
        isize = data[-4] | (data[-3] << 8) | (data[-2] << 16) | (data[-1] << 24)
        sz = max(isize, sz)
    return sz


def stage_and_batches(bound, stage_mb):
    """stage_mb: the value of RK_STAGE_MB, None when it is not set"""
    total_bound = sum(bound)
    stage_bytes = min(256 << 20, max(64 << 20, total_bound // 8))
    if stage_mb is not None:
        stage_bytes = max(1, stage_mb) << 20
    stage_bytes = (stage_bytes + 1023) & ~1023
    batches, i = [], 0
    while i < len(bound):
        first, pos, slots = i, 0, []
        if bound[i] > stage_bytes:
            batches.append((first, i + 1, bound[i], 1, [(0, bound[i])]))
            i += 1
            continue
        while i < len(bound) and pos + bound[i] <= stage_bytes:
            slots.append((pos, bound[i]))
            pos += bound[i]
            i += 1
        batches.append((first, i, pos, 0, slots))
    return stage_bytes, batches


def plan_line(bound, stage_mb):
    stage, batches = stage_and_batches(bound, stage_mb)
    return " | ".join(["stage=%d" % stage] + [" ".join(["%d %d %d %d" % b[:4]] + ["%d:%d" % s for s in b[4]]) for b in batches])


S = 64 * MIB
PLANS = {"none": [], "one": [5 * 1024], "below": [S - 1024], "at": [S], "above": [S + 1024],
         "sum_lands_on_stage": [S // 4, S // 4, S // 2, 1024, S - 1024, 1024, 1024],
         "oversized_first": [S + 1024, 1024, 2048], "oversized_middle": [1024, S + 1024, 2048], "oversized_last": [1024, 2048, S + 1024],
         "two_oversized": [3 * S, 2 * S, 1024],
         "an_eighth_of_the_input": [S] * 9 + [S // 8 * 9 + 1024, 1024],      # the staging buffer follows the total: 64 MiB no longer
         "capped": [200 * MIB] * 11 + [256 * MIB, 256 * MIB + 1024]}


def test_batch_plan_equals_the_rules_it_replaces(exe, work):
    lines = {name: " ".join(["plan"] + [str(b) for b in bound] + ["#" + name]) for name, bound in PLANS.items()}
    # (the trailing #name is no number: the program stops reading bounds there)
    got, _ = run_cases(exe, work, list(lines.values()), name="plans.txt")
    for name, bound in PLANS.items():
        assert got[lines[name]][2] == plan_line(bound, None), name
    assert got[lines["none"]][2] == "stage=%d" % S
    assert got[lines["below"]][2].endswith("| 0 1 %d 0 0:%d" % (S - 1024, S - 1024)) and got[lines["at"]][2].endswith("| 0 1 %d 0 0:%d" % (S, S))
    assert got[lines["above"]][2].endswith("| 0 1 %d 1 0:%d" % (S + 1024, S + 1024))             # alone, pageable
    assert got[lines["sum_lands_on_stage"]][2].split(" | ")[1].startswith("0 3 %d 0 " % S)       # a batch filled to the byte
    assert [b.split()[3] for b in got[lines["oversized_middle"]][2].split(" | ")[1:]] == ["0", "1", "0"]
    assert got[lines["an_eighth_of_the_input"]][2].startswith("stage=%d " % (((9 * S + S // 8 * 9 + 2048) // 8 + 1023) & ~1023))
    assert got[lines["capped"]][2].startswith("stage=%d " % (256 * MIB)) and got[lines["capped"]][2].endswith(" 1 0:%d" % (256 * MIB + 1024))
    # RK_STAGE_MB
    for mb, env in ((1, "1"), (3, "3"), (0, "0")):
        got, _ = run_cases(exe, work, list(lines.values()), env={"RK_STAGE_MB": env}, name="plans_mb.txt")
        for name, bound in PLANS.items():
            assert got[lines[name]][2] == plan_line(bound, mb), (name, mb)
    small = [300 * 1024] * 7 + [MIB, MIB + 1024, 1024]
    line = " ".join(["plan"] + [str(b) for b in small])
    got, _ = run_cases(exe, work, [line], env={"RK_STAGE_MB": "1"}, name="plans_small.txt")
    assert got[line][2] == plan_line(small, 1)
    assert [b.split()[:4] for b in got[line][2].split(" | ")[1:]] == [["0", "3", str(900 * 1024), "0"], ["3", "6", str(900 * 1024), "0"],
                                                                    ["6", "7", str(300 * 1024), "0"], ["7", "8", str(MIB), "0"],
                                                                    ["8", "9", str(MIB + 1024), "1"], ["9", "10", "1024", "0"]]


def test_packed_bound_reads_the_gzip_trailer(exe, work):
    rng = np.random.default_rng(3)
    text = b">g\n" + bytes(rng.choice(list(b"ACGT"), 5000).tolist()) + b"\n"
    files = {"plain.fa": text, "member.fa.gz": gzip.compress(text, mtime=0),               # the trailer is larger than the file
             "members.fa.gz": gz_variants(text)["gz3"],                                   # ... smaller: the last member's 7 bytes
             "tiny.gz": b"\x1f\x8b" + b"\0" * 15, "empty.fa": b"", "kib.fa": b"A" * 1023, "kib1.fa": b"A" * 1024}
    cases = []
    for name, data in files.items():
        (work / name).write_bytes(data)
        cases.append("bound %s" % (work / name))
    cases.append("bound %s" % (work / "missing.fa"))
    got, _ = run_cases(exe, work, cases, name="bounds.txt")
    for name, case in zip(files, cases):
        b = packed_bound(str(work / name))
        assert got[case][2] == "%d %d" % (b, (b + 1 + 1023) & ~1023), name
    assert got[cases[0]][2] == "5004 5120"
    assert got[cases[1]][2].split()[0] == "5004" and len(files["member.fa.gz"]) < 5004
    assert got[cases[2]][2].split()[0] == str(len(files["members.fa.gz"])) and len(files["members.fa.gz"]) > 7
    assert got[cases[3]][2] == "17 1024" and got[cases[5]][2] == "1023 1024" and got[cases[6]][2] == "1024 2048"
    assert got[cases[-1]][2] == "unreadable"
