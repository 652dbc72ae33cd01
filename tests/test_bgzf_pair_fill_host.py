"""The device-free side of the paired file call on two BGZF files (docs/design/mapper.md, "Compressed input for pairs"): the fill
policy BgzfPairFill (csrc/asm_host.h) under ChunkReader and the pair cut's rule (csrc/asm_pair_cut.h), driven by
host/bgzf_pair_fill_host_check.cpp, which plays the device's part on the host.  Built here plain and under ASan + UBSan as a
stand-alone program.  The references: the inflated texts themselves, asm_fastq_cut_n (inside the program), and what FastqPairFill
reports of the same texts (host/asm_host_check.cpp --pairs)."""
import os
import struct
import subprocess

import pytest

from tests import bgzf_in_cases as bi
from tests import bgzf_pair_cases as pc
from tests.test_map_file_host import PKG, san_flags
from tests.test_map_pairs_file_host import host_check, run_pairs  # noqa: F401  (host_check is a fixture)

SRC = os.path.join(PKG, "host", "bgzf_pair_fill_host_check.cpp")
SLOTS = 3       # ChunkReader's slots: a chunk is filled with the consumer's word of the chunk three before it at the latest


def compiled(exe, flags):
    assert os.path.exists(SRC), "host/bgzf_pair_fill_host_check.cpp: the host build of the paired BGZF fill policy"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def pair_check(tmp_path_factory):
    return compiled(str(tmp_path_factory.mktemp("pair_fill") / "bgzf_pair_fill_host_check_asan"), san_flags())


@pytest.fixture(scope="module")
def pair_plain(tmp_path_factory):
    return compiled(str(tmp_path_factory.mktemp("pair_fill_plain") / "bgzf_pair_fill_host_check"), ["-O2"])


def run_gz(exe, tmp, gz1: bytes, gz2: bytes, want: int):
    """-> ([(R, done1, done2, members1, members2, region 1, region 2)], end facts); a sanitizer report fails here"""
    f1, f2, out = tmp / "r1.fq.gz", tmp / "r2.fq.gz", tmp / "chunks.bin"
    f1.write_bytes(gz1)
    f2.write_bytes(gz2)
    r = subprocess.run([exe, str(f1), str(f2), str(want), str(out)], capture_output=True, text=True, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", r.stderr[-3000:]
    assert r.returncode == 0, r.returncode
    data, chunks, at = out.read_bytes(), [], 0
    while struct.unpack_from("<Q", data, at)[0] != 2**64 - 1:
        R, d1, d2, m1, m2, len1, len2 = struct.unpack_from("<7Q", data, at)
        at += 56
        chunks.append((R, d1, d2, m1, m2, data[at:at + len1], data[at + len1:at + len1 + len2]))
        at += len1 + len2
    status, peak, n1, n2, e1, e2, mo1, mo2, empty, text_peak = struct.unpack_from("<10Q", data, at + 8)
    assert at + 88 == len(data)
    return chunks, dict(status=status, carry_peak=peak, records=(n1, n2), extra_lines=(e1, e2), more=(mo1, mo2), empty_chunks=empty,
                        text_peak=text_peak)


def end_report(end):
    """what the call says of the files' ends, from a policy's facts: the plain call's order -> (kind, file, record) or None"""
    for f in range(2):
        if end["extra_lines"][f]:
            return "truncated", f + 1, end["records"][f] + 1
    for f in range(2):
        if end["more"][f]:
            return "no mate", f + 1, end["records"][1 - f] + 1
    return None


def member_texts(gz):
    return [len(bi.reference(m)) for _, m in bi.split_members(gz)]


def carry_bound(want, gz1, gz2, text1, text2):
    """The bound of the design section, from the inputs alone.  A chunk hands out less than want + m1 + m2 text bytes (each file goes
    past its share by less than one member of m1, m2 text bytes).  The policy splits by what it knows to be unpaired: exact up to the
    chunk the consumer has last reported, which is at most SLOTS chunks back, plus the chunk being filled and one more for the share that is
    clamped at 0 while the other file catches up; so one file is ahead by at most (SLOTS + 2) such chunks.  Behind a cut each file also keeps
    less than one record."""
    longest = [max((len(r) for r in t.split(b"\n@")), default=0) + 2 for t in (text1, text2)]
    return (SLOTS + 2) * (want + max(member_texts(gz1), default=0) + max(member_texts(gz2), default=0)) + longest[0] + longest[1]


def cut_by_name(text, how):
    return {"bgzip": lambda: pc.container(text), "small": lambda: pc.container(text, pc.SMALL),
            "small+empties": lambda: pc.container(text, pc.SMALL, empties=50), "bgzip+empties": lambda: pc.container(text, empties=1),
            "no eof": lambda: pc.container(text, eof=False), "4099": lambda: pc.container(text, (4099,))}[how]()


def drop_last_newline(t):
    return t[:-1]


def cases():
    """{name: (text 1, text 2, cut of file 1, cut of file 2)}: mates of 36 and 150 bp, so file 2 is about three times file 1"""
    t1, t2 = pc.mates(1200)
    c1, c2 = pc.mates(300, crlf=(True, False))
    short1, short2 = pc.mates(40)
    l1, l2 = pc.mates(400, long_every=100)
    rec1, rec2 = pc.records(t1)[0], pc.records(t2)[0]
    assert rec1 == rec2 == 1200
    out = {
        "bgzip members against small ones": (t1, t2, "bgzip+empties", "small+empties"),
        "small members against bgzip ones": (t1, t2, "small", "bgzip"),
        "file 1 CRLF, file 2 without its last newline": (c1, drop_last_newline(c2), "4099", "no eof"),
        "file 2 longer by one record": (pc.whole_records(t1, 1199), t2, "bgzip", "small"),
        "file 1 longer by 500 records": (t1, pc.whole_records(t2, 700), "bgzip", "4099"),
        "file 1 truncated": (t1[:-60], t2, "bgzip", "small"),
        "file 2 truncated, no last newline": (short1, short2[:-200], "small", "small"),
        "records longer than a chunk": (l1, l2, "bgzip", "small"),
        "one record each": (pc.whole_records(t1, 1), pc.whole_records(t2, 1), "bgzip", "bgzip"),
    }
    return out


CASES = cases()
WANTS = (1, 4096, 0)    # 0: both texts in one chunk


def check(exe, host_check, tmp_path, name, want):
    text1, text2, how1, how2 = CASES[name]
    gz1, gz2 = cut_by_name(text1, how1), cut_by_name(text2, how2)
    assert bi.reference(gz1) == text1 and bi.reference(gz2) == text2
    want = want or len(text1) + len(text2)
    chunks, end = run_gz(exe, tmp_path, gz1, gz2, want)
    assert end["status"] == 0
    # the regions, chunk after chunk, are each file's text up to the last whole pair
    pairs = min(pc.records(text1)[0], pc.records(text2)[0])
    assert sum(c[0] for c in chunks) == pairs
    for f, text in enumerate((text1, text2)):
        assert b"".join(c[5 + f] for c in chunks) == pc.whole_records(text, pairs), (name, f)
        assert all(c[5 + f].count(b"\n") == 4 * c[0] for c in chunks)
    # the ends of the files: FastqPairFill's word on the inflated texts, in the call's own terms
    _, ref = run_pairs(host_check, tmp_path, text1, text2, 4096)
    assert ref["failed"] == 0
    assert end_report(end) == end_report(ref), (name, end, ref)
    assert end["extra_lines"] == ref["extra_lines"] and end["more"] == ref["more"], (name, end, ref)
    for f in range(2):
        if not end["more"][f]:      # (a file that goes on holds as many whole records as the reader happened to have read)
            assert end["records"][f] == ref["records"][f] == pc.records((text1, text2)[f])[0]
    # a chunk hands out whole members, less than one past each share, and the carries stay bounded whatever the file's length
    m1, m2 = max(member_texts(gz1), default=0), max(member_texts(gz2), default=0)
    assert end["text_peak"] < want + m1 + m2
    assert end["carry_peak"] < carry_bound(want, gz1, gz2, text1, text2), (name, want, end["carry_peak"])
    return chunks, end


@pytest.mark.parametrize("want", WANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_bgzf_files_stay_in_step(pair_check, host_check, tmp_path, name, want):
    check(pair_check, host_check, tmp_path, name, want)


def test_carries_stay_flat_however_long_the_files(pair_check, host_check, tmp_path):
    """with members of 4 099 bytes the bound at 4 096 bytes a chunk is below a tenth of the files: the carries do not grow with them"""
    text1, text2 = pc.mates(3000, seed=6)
    gz1, gz2 = pc.container(text1, (4099,)), pc.container(text2, (4099,))
    bound = carry_bound(4096, gz1, gz2, text1, text2)
    assert 10 * bound < len(text1) + len(text2)
    chunks, end = run_gz(pair_check, tmp_path, gz1, gz2, 4096)
    assert end["status"] == 0 and end_report(end) is None and sum(c[0] for c in chunks) == 3000
    assert end["carry_peak"] < bound


def test_chunks_without_a_pair_are_part_of_the_stream(pair_check, host_check, tmp_path):
    """a mate of 6 000 bases is a record of 12 KB: a chunk of 4 096 bytes that lies inside it holds no whole pair, and the
    split leans on with everything as carry; one member a chunk does the same all the time"""
    for name, want in (("records longer than a chunk", 4096), ("bgzip members against small ones", 1)):
        _, end = check(pair_check, host_check, tmp_path, name, want)
        assert end["empty_chunks"] > 0, name


def test_levels_1_and_9_stay_in_step(pair_check, tmp_path):
    """compression ratios that differ: the split by compressed bytes is only the start, the measured bytes per record take over"""
    text1, text2 = pc.mates(1500, 100, 100, seed=9)
    gz1, gz2 = pc.container(text1, (4099,), level=1), pc.container(text2, (4099,), level=9)
    chunks, end = run_gz(pair_check, tmp_path, gz1, gz2, 8192)
    assert end["status"] == 0 and end_report(end) is None and sum(c[0] for c in chunks) == 1500
    assert end["carry_peak"] < carry_bound(8192, gz1, gz2, text1, text2)


def test_only_eof_blocks_and_nothing(pair_check, tmp_path):
    for gz1, gz2 in ((bi.EOF_BLOCK, bi.EOF_BLOCK), (b"", b""), (bi.EOF_BLOCK, b""), (bi.EOF_BLOCK * 3, bi.EOF_BLOCK)):
        chunks, end = run_gz(pair_check, tmp_path, gz1, gz2, 4096)
        assert end["status"] == 0 and end_report(end) is None and end["records"] == (0, 0)
        assert all(c[0] == 0 and c[5] == c[6] == b"" for c in chunks)


def test_a_bad_header_ends_the_stream(pair_check, tmp_path):
    text1, text2 = pc.mates(50)
    bad = bi.corrupt()["bad magic"][0]
    for gz1, gz2 in ((pc.container(text1), bad), (bad, pc.container(text2))):
        _, end = run_gz(pair_check, tmp_path, gz1, gz2, 4096)
        assert end["status"] == 2


def test_plain_build_agrees(pair_check, pair_plain, tmp_path):
    text1, text2, how1, how2 = CASES["file 1 CRLF, file 2 without its last newline"]
    gz1, gz2 = cut_by_name(text1, how1), cut_by_name(text2, how2)
    a, b = run_gz(pair_plain, tmp_path, gz1, gz2, 4096), run_gz(pair_check, tmp_path, gz1, gz2, 4096)
    assert [c[5:] for c in a[0]] and b"".join(c[5] for c in a[0]) == b"".join(c[5] for c in b[0])
    assert {k: a[1][k] for k in ("records", "extra_lines", "more")} == {k: b[1][k] for k in ("records", "extra_lines", "more")}
