"""rk_index_blob.h (the header and the section table of the single-buffer index) as plain C++: tools/blob_layout_check.cpp, compiled
here with g++, prints the layout, the bytes copied and the bytes allocated on unpack over a grid of dimensions, widths and flags;
the expected values are the three hand-written lists the table replaced (blob_layout, rk_index_pack_dev, rk_index_unpack_dev),
written out below section by section."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = ("postings", "uhash", "upos", "sizes", "self", "selfoff", "src", "split", "orig")     # the header's order of offset words
IDS = ("postings", "uhash", "upos", "sizes", "orig", "src", "self", "selfoff", "split")       # the buffer's order of sections


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blob_layout") / "blob_layout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"),
                           os.path.join(ROOT, "tools", "blob_layout_check.cpp"), "-o", exe])
    return subprocess.check_output([exe], text=True).splitlines()


def al256(x):
    return (x + 255) & ~255


def expected(H, U, n_self, n_ref, wide, relabeled, has_src, has_self):
    """({section: offset}, bytes of the blob, {section: (bytes copied, bytes allocated on unpack)}) as the three lists had them"""
    hw = 8 if wide else 4
    off, carried = dict.fromkeys(WORDS, 0), {}
    p = 256
    off["postings"] = p; p = al256(p + (H + 1) * 4); carried["postings"] = (H * 4, (H + 8) * 4)                    # noqa: E702
    off["uhash"] = p; p = al256(p + (U + 1) * hw); carried["uhash"] = (U * hw, (U + 1) * hw)                        # noqa: E702
    off["upos"] = p; p = al256(p + (U + 2) * 4); carried["upos"] = ((U + 1) * 4, (U + 2) * 4)                        # noqa: E702
    off["sizes"] = p; p = al256(p + (n_ref + 1) * 4); carried["sizes"] = (n_ref * 4, (n_ref + 1) * 4)                # noqa: E702
    if relabeled:
        off["orig"] = p; p = al256(p + (n_ref + 1) * 4); carried["orig"] = (n_ref * 4, (n_ref + 1) * 4)              # noqa: E702
    if has_src:
        off["src"] = p; p = al256(p + (n_ref + 1) * 8); carried["src"] = ((n_ref + 1) * 8, (n_ref + 1) * 8)          # noqa: E702
    if has_self:
        off["self"] = p; p = al256(p + (n_self + 1) * 8); carried["self"] = (n_self * 8, (n_self + 1) * 8)            # noqa: E702
        off["selfoff"] = p; p = al256(p + (n_ref + 1) * 8); carried["selfoff"] = ((n_ref + 1) * 8, (n_ref + 1) * 8)  # noqa: E702
        off["split"] = p; p = al256(p + (n_ref + 1) * 8); carried["split"] = ((n_ref + 1) * 8, (n_ref + 1) * 8)      # noqa: E702
    return off, p, carried


def test_header_size_magic_and_section_count(lines):
    assert lines[0] == "header 168 magic RSKDIDX7 sections 9"


def test_layout_copies_and_allocations_equal_the_lists_the_table_replaced(lines):
    got = {}
    for l in lines[1:]:
        key, offs, secs = l[5:].split(" :")
        got[tuple(int(x) for x in key.split())] = ([int(x) for x in offs.split()], secs.split())
    dims = (0, 1, 63, 64, 65, 1000)
    cases = 0
    for H in dims:
        for U in dims:
            for n_self in dims:
                for n_ref in (0, 1, 33):
                    for wide in (0, 1):
                        for flags in range(8):
                            off, total, carried = expected(H, U, n_self, n_ref, wide, flags & 1, flags & 2, flags & 4)
                            offs, secs = got[(H, U, n_self, n_ref, wide, flags)]
                            assert offs == [off[w] for w in WORDS] + [total], (H, U, n_self, n_ref, wide, flags)
                            want = ["%d=%d/%d" % ((i,) + carried[name]) for i, name in enumerate(IDS) if name in carried]
                            assert secs == want, (H, U, n_self, n_ref, wide, flags)
                            cases += 1
    assert cases == len(got) == 6 * 6 * 6 * 3 * 2 * 8
    # (an index of 1000 postings, 65 lists, 33 genomes, every section: the sections in buffer order, the size by hand)
    offs, _ = got[(1000, 65, 1000, 33, 0, 7)]
    assert offs == [256, 4352, 4864, 5376, 6400, 14592, 5888, 15104, 5632, 15616]
