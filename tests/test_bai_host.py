"""The BAM index on the CPU (docs/design/mapper.md, "BAM index").  First tests/bai_cases.py itself on hand-made cases; then
host/bai_host_check.cpp, built here under ASan + UBSan and run as a program, and asm_bam_index_host through the library: both must
equal bai_cases.build() byte for byte on synthetic coordinate-sorted BAM files at the edges of the format; then the error cases."""
import os
import struct
import subprocess
import zlib

import pytest

from tests import bai_cases as bai
from tests import bam_cases as bc
from tests.test_map_file_host import san_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
P = bc.PAYLOAD
BIG = 1 << 29
REFS = [("empty_front", 3000), ("big", BIG), ("empty_mid", 70000), ("small", 70000), ("empty_last", 12)]


def rec(tid, pos, cigar=((100, "M"),), flag=0, name="r", pad=0):
    """a record of the hand-made files; pad: the length of a Z tag that brings the stream to a chosen size (0: none)"""
    cigar = list(cigar)
    l_seq = sum(n for n, op in cigar if op in "MI=X") if cigar else 20
    tags = [("XZ", "Z", "x" * (pad - 4))] if pad else []
    return bc.encode_record(tid, pos, 30 if cigar else 0, flag, -1, -1, 0, name, cigar, "A" * l_seq, bytes(l_seq), tags)


def sort_key(r):
    tid, pos = struct.unpack_from("<ii", r, 4)
    return (1 << 31 if tid < 0 else tid, pos if tid >= 0 else 0)


def stream_of(records, refs=REFS):
    return bc.encode_header(b"@HD\tVN:1.6\tSO:coordinate\n", refs), b"".join(sorted(records, key=sort_key))


def padded(records, blocks):
    """the records and one more in front of the unplaced ones whose tag brings the record stream to exactly `blocks` payloads"""
    have = sum(len(r) for r in records)
    bare = len(rec(3, 69000, name="pad"))
    pad = blocks * P - have - bare
    assert pad >= 5
    return records + [rec(3, 69000, name="pad", pad=pad)]


def frame(asm, head, body, level=0, cut=None):
    """the file: the header in blocks of its own and the records in blocks of P (the library's cut), or, with cut, the whole stream in
    members of those sizes in turn"""
    comp = (lambda s: bc.frame_stored(s, eof=False)) if level == 0 else (lambda s: asm.bgzf_compress_host(s, eof=False, level=level))
    if cut is None:
        return comp(head) + comp(body) + bc.EOF_BLOCK
    whole, out, at, k = head + body, b"", 0, 0
    while at < len(whole):
        n = cut[k % len(cut)]
        out += comp(whole[at:at + n]) if n else bc.EOF_BLOCK              # an empty member in the middle
        at, k = at + n, k + 1
    return out + bc.EOF_BLOCK


def edge_records():
    out = []
    for shift in (14, 17, 20, 23, 26):
        for k in (1, 3):
            edge = k << shift
            out += [rec(1, edge - 100, name="in%d" % shift), rec(1, edge - 50, name="x%d" % shift), rec(1, edge, name="at%d" % shift),
                    rec(1, edge - 1, ((1, "M"),), name="one%d" % shift)]
    out.append(rec(1, BIG - 100, name="last"))                                                   # ends at exactly 2^29
    out.append(rec(1, 5 * 16384 - 60, ((30, "M"), (50, "D"), (20, "M")), name="del"))            # pos + l_seq stays below the edge
    out.append(rec(1, 7 * 16384 - 10, ((5, "M"), (30, "N"), (5, "M")), name="skip"))
    out += [rec(1, 40000 + 7 * t, name="m%d" % t, flag=16 * (t % 2)) for t in range(300)]
    out += [rec(3, 100 + 31 * t, name="s%d" % t) for t in range(900)]
    out += [rec(3, 16384 - 40, name="s_edge"), rec(3, 500, (), flag=4 | 1 | 64, name="placed_unmapped"), rec(3, 20000, (), flag=4, name="pu2")]
    out += [rec(-1, -1, (), flag=4, name="u%d" % t) for t in range(40)]
    return out


def multi_block_member(payload):
    """one BGZF member whose deflate stream has three blocks"""
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    third = len(payload) // 3
    d = z.compress(payload[:third]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(payload[third:2 * third]) + z.flush(zlib.Z_FULL_FLUSH)
    d += z.compress(payload[2 * third:]) + z.flush()
    return bc.FIXED + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(payload), len(payload))


def cases(asm):
    """name -> the file's bytes"""
    out = {}
    head, body = stream_of(edge_records())
    assert len(body) > 2 * P
    out["edges stored"] = frame(asm, head, body)
    out["edges deflate"] = frame(asm, head, body, level=1)
    out["odd members"] = frame(asm, head, body, cut=[1, 777, P, 13, 40001, 0, 65536 - 300, 5])
    out["odd members deflate"] = frame(asm, head, body, level=1, cut=[3, 60000, 0, 0, 1234])
    whole = head + body
    out["deflate blocks in a member"] = b"".join(multi_block_member(whole[at:at + 50000]) for at in range(0, len(whole), 50000)) + bc.EOF_BLOCK
    out["no eof block"] = frame(asm, head, body)[:-28]
    few = [rec(1, 1000 + 10 * t, name="f%d" % t) for t in range(50)] + [rec(-1, -1, (), flag=4, name="u")]
    for blocks in (1, 2):
        placed_last = padded([r for r in few if sort_key(r)[0] < 1 << 31], blocks)                 # the padded record is the last one
        h1, b1 = stream_of(placed_last)
        assert len(b1) == blocks * P
        out["exactly %d payloads" % blocks] = frame(asm, h1, b1)
        out["exactly %d payloads deflate" % blocks] = frame(asm, h1, b1, level=1)
    out["empty"] = frame(asm, *stream_of([]))
    out["only unplaced"] = frame(asm, *stream_of([rec(-1, -1, (), flag=4, name="u%d" % t) for t in range(30)]))
    out["no references"] = frame(asm, *stream_of([rec(-1, -1, (), flag=4, name="u%d" % t) for t in range(3)], refs=[]))
    out["one record"] = frame(asm, *stream_of([rec(4, 0, ((12, "M"),))]))
    return out


@pytest.fixture(scope="module")
def files(asm):
    return cases(asm)


@pytest.fixture(scope="module")
def built(files):
    """bai_cases.build of every case, once"""
    return {name: bai.build(data) for name, data in files.items()}


@pytest.fixture(scope="module")
def bai_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bai_check") / "bai_host_check_asan")
    src = os.path.join(PKG, "host", "bai_host_check.cpp")
    assert os.path.exists(src), "host/bai_host_check.cpp: the host build of the BAM index"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


# ---- bai_cases itself ------------------------------------------------------------------------------------------------------------------
def test_hand_made_index(asm):
    """three records whose index can be written down: two in bin 4681 of sequence 0 with one crossing into window 1 (bin 585), one
    unplaced"""
    refs = [("a", 40000), ("b", 100)]
    recs = [rec(0, 10, name="a"), rec(0, 16300, name="b"), rec(0, 16390, name="c"), rec(-1, -1, (), flag=4, name="u")]
    head, body = stream_of(recs, refs)
    data = frame(asm, head, body)
    at0 = len(bc.frame_stored(head, eof=False)) << 16
    size = len(recs[0])
    assert len(recs[1]) == len(recs[2]) == size
    v = [at0 + t * size for t in range(4)]
    want = b"BAI\x01" + struct.pack("<i", 2)
    want += struct.pack("<i", 4)
    want += struct.pack("<IiQQ", 585, 1, v[1], v[2])                    # [16300, 16400) crosses 2^14
    want += struct.pack("<IiQQ", 4681, 1, v[0], v[1])
    want += struct.pack("<IiQQ", 4682, 1, v[2], v[3])
    want += struct.pack("<IiQQQQ", 37450, 2, v[0], v[3], 3, 0)
    want += struct.pack("<iQQ", 2, v[0], v[1])
    want += struct.pack("<ii", 0, 0) + struct.pack("<Q", 1)
    assert bai.build(data) == want
    index = bai.parse(want, data)
    assert index["bins"] == 3 and index["chunks"] == 3 and index["intervals"] == 2 and index["no_coor"] == 1
    rd = bai.Reader(data)
    assert bai.query(index, rd, 0, 0, 100) == bai.scan(rd, 0, 0, 100) == [0]
    assert bai.query(index, rd, 0, 16384, 16385) == bai.scan(rd, 0, 16384, 16385) == [1]
    assert bai.query(index, rd, 0, 16399, 16400) == [1, 2] and bai.query(index, rd, 0, 16490, 30000) == []
    assert bai.query(index, rd, 1, 0, 100) == [] and bai.idxstats(index) == ([(3, 0), (0, 0)], 1)
    assert bai.reg2bins(0, 1 << 29) == list(range(37449)) and bai.reg2bins(16384, 16385) == [0, 1, 9, 73, 585, 4682]


def test_parse_refuses_a_broken_index(asm):
    head, body = stream_of([rec(1, 10, name="a"), rec(1, 20000, name="b")])
    data = frame(asm, head, body)
    good = bai.build(data)
    bai.parse(good, data)
    at = good.index(struct.pack("<Ii", 4681, 1)) + 8
    beg, end = struct.unpack_from("<QQ", good, at)
    for broken in (good[:at] + struct.pack("<QQ", end, end) + good[at + 16:],                      # an empty chunk
                   good[:at] + struct.pack("<QQ", beg + 1, end) + good[at + 16:]):                 # a chunk that starts inside a record
        with pytest.raises(AssertionError):
            bai.parse(broken, data)


def test_end_of_stream_on_a_block_edge(files):
    """the last v_end of a record stream of whole payloads is the EOF block's offset with in-block offset 0"""
    for blocks in (1, 2):
        data = files["exactly %d payloads" % blocks]
        index = bai.parse(bai.build(data), data)
        assert index["refs"][3]["pseudo"][1] == (len(data) - 28) << 16
        assert max(c[1] for ch in index["refs"][3]["bins"].values() for c in ch) == (len(data) - 28) << 16


# ---- the host build against it --------------------------------------------------------------------------------------------------------
def test_checker_equals_build(files, built, bai_check, tmp_path):
    for name, data in files.items():
        src, dst = tmp_path / "in.bam", tmp_path / "out.bai"
        src.write_bytes(data)
        r = subprocess.run([bai_check, str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stdout, r.stderr[-3000:])
        got = dst.read_bytes()
        assert got == built[name], name
        index = bai.parse(got, data)
        word = r.stdout.split()
        assert word[0] == "ok" and [int(x) for x in word[1:]] == [len(index["refs"]), index["bins"], index["chunks"], index["intervals"],
                                                                  index["no_coor"], len(got)], name


def test_library_equals_build(asm, files, built):
    for name, data in files.items():
        assert asm.bam_index_host(data) == built[name], name
    assert built["empty"] == b"BAI\x01" + struct.pack("<i", 5) + bytes(40) + bytes(8)
    assert built["no references"] == b"BAI\x01" + bytes(4) + struct.pack("<Q", 3)


def test_queries_find_what_the_scan_finds(files, built):
    data = files["edges deflate"]
    index, rd = bai.parse(built["edges deflate"], data), bai.Reader(data)
    regions = [(1, 0, BIG), (1, BIG - 1, BIG), (1, BIG - 101, BIG - 100), (3, 0, 70000), (3, 16383, 16384), (3, 16384, 16385), (0, 0, 3000),
               (1, 5 * 16384, 5 * 16384 + 1), (1, 5 * 16384 + 39, 5 * 16384 + 40), (1, 5 * 16384 + 40, 5 * 16384 + 41), (1, 7 * 16384, 7 * 16384 + 5)]
    for shift in (14, 17, 20, 23, 26):
        for k in (1, 3):
            edge = k << shift
            regions += [(1, edge - 1, edge), (1, edge, edge + 1), (1, edge - 101, edge - 100), (1, edge + 99, edge + 100), (1, edge - 1, edge + 1)]
    hits = 0
    for tid, beg, end in regions:
        got = bai.query(index, rd, tid, beg, end)
        assert got == bai.scan(rd, tid, beg, end), (tid, beg, end)
        hits += len(got)
    assert hits > 1000
    counts, no_coor = bai.idxstats(index)
    assert no_coor == 40 and counts[3] == (901, 2) and counts[0] == counts[2] == counts[4] == (0, 0) and sum(counts[1]) == 20 * 2 + 3 + 300
    assert [len(r["ioffset"]) for r in index["refs"]] == [0, BIG >> 14, 0, 2, 0]            # the small sequence's records end at 28 069


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def host_error(asm, data):
    with pytest.raises(asm.AsmError) as exc:
        asm.bam_index_host(data)
    return exc.value.code, str(exc.value)


def test_errors(asm, files, bai_check, tmp_path):
    head, _ = stream_of([])
    a, b, c = rec(1, 500, name="a"), rec(1, 400, name="b"), rec(3, 10, name="c")
    mk = lambda body: bc.frame_stored(head, eof=False) + bc.frame_stored(body)
    bad = {
        "unsorted": (mk(a + c + b), -1, "record 2 lies below its predecessor"),
        "unsorted pos": (mk(a + b), -1, "record 1 lies below its predecessor"),
        "unplaced in front": (mk(rec(-1, -1, (), flag=4) + a), -1, "record 1 lies below its predecessor"),
        "refID": (mk(a + rec(5, 10)), -1, "record 1 has refID 5 (n_ref = 5)"),
        "truncated": (mk((a + c)[:-7]), -1, "record 1 reaches past the end"),
        "truncated head": (mk(a + c[:20]), -1, "record 1 reaches past the end"),
        "magic": (bc.frame_stored(b"BAM\x02" + head[4:]), -1, "BAM magic"),
        "bin": (mk(bc.encode_record(1, 500, 30, 0, -1, -1, 0, "w", [(100, "M")], "A" * 100, bytes(100), [], bin_=4682)), -1,
                "record 0 has bin 4682, reg2bin of its position and CIGAR is 4681"),
        "above": (mk(a + rec(1, BIG - 99, name="over")), -4, "record 1 ends above 2^29"),
        "far above": (mk(a + bc.encode_record(1, BIG + 5, 30, 0, -1, -1, 0, "w", [(10, "M")], "A" * 10, bytes(10), [], bin_=0)), -4,
                      "needs a .csi index"),
        "container": (files["edges stored"][:-40], -1, "asm_bam_index_host: BGZF member"),
    }
    for name, (data, code, text) in bad.items():
        got_code, message = host_error(asm, data)
        assert got_code == code and text in message and ": asm_bam_index_host: " in message, (name, got_code, message)
        src, dst = tmp_path / "bad.bam", tmp_path / "bad.bai"
        src.write_bytes(data)
        r = subprocess.run([bai_check, str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert r.returncode == (3 if name == "container" else 4) and r.stderr == "" and not dst.exists(), (name, r.returncode, r.stderr[-2000:])
        if name != "container":
            assert r.stdout.startswith("refused %d " % {-1: 2 if "unsorted" in name or "unplaced" in name else 1, -4: 3}[code]) and text in r.stdout
    crc = bytearray(files["edges deflate"])
    crc[-40] ^= 1                                                            # inside the last data block's trailer
    code, message = host_error(asm, bytes(crc))
    assert code == -1 and "BGZF member" in message
    # dst_cap: the size comes back, nothing is written
    import ctypes
    lib, data = asm.load_library(), files["edges stored"]
    want = asm.bam_index_host(data)
    out, got = ctypes.create_string_buffer(b"\x5a" * len(want), len(want)), ctypes.c_size_t(0)
    assert lib.asm_bam_index_host(data, len(data), out, len(want) - 1, ctypes.byref(got)) == -1
    assert got.value == len(want) and out.raw == b"\x5a" * len(want) and b"dst_cap is below" in lib.asm_last_error(None)
    assert lib.asm_bam_index_host(data, len(data), out, len(want), ctypes.byref(got)) == 0 and out.raw == want
    assert lib.asm_bam_index_host(data, len(data), out, len(want), None) == -1 and lib.asm_bam_index_host(None, 5, out, 5, ctypes.byref(got)) == -1


def test_setter_without_a_handle(asm):
    lib = asm.load_library()
    assert lib.asm_map_set_bam_index(None, 2) == -1 and b"kind must be" in lib.asm_last_error(None)
    assert lib.asm_map_set_bam_index(None, 1) == -1 and lib.asm_last_error(None) == b"asm_map_set_bam_index: NULL handle"
    assert lib.asm_map_get_bam_index(None) == asm.BAM_INDEX_NONE == 0 and asm.BAM_INDEX_BAI == 1
