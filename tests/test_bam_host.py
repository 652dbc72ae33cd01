"""BAM output on the CPU (docs/design/mapper.md, "BAM output"): the reader of tests/bam_cases.py on its hand-made records; then
host/bam_host_check.cpp, built here under ASan + UBSan, which runs bam_format (csrc/asm_bam.h) through the lane sink for lanes 0..63
and sam_format on the same line, so that every decoded record must print as the SAM line of the same SamLine; the host CRC, combine
and slice copy of csrc/asm_bgzf.h against zlib; bam_header_bytes against the reader's encode_header; asm_bgzf_bound against the
formula."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

from tests import bam_cases as bc
from tests.test_map_file_host import san_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
NAMES = ["chrA", "chrB"]
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 1)


# ---- the reader on its own records ---------------------------------------------------------------------------------------------------
def test_reader_on_hand_made_records():
    stream = bc.encode_header(b"@HD\tVN:1.6\n", bc.HAND_REFS) + b"".join(bc.encode_record(**r) for r, _ in bc.HAND_RECORDS)
    data = bc.frame_stored(stream)
    text, refs, recs, blocks = bc.parse_bam(data)
    assert text == b"@HD\tVN:1.6\n" and refs == bc.HAND_REFS and len(blocks) == 2
    names = [n for n, _ in refs]
    assert [bc.sam_line(r, names) for r in recs] == [line for _, line in bc.HAND_RECORDS]
    assert bc.decode(data) == text + "".join(line for _, line in bc.HAND_RECORDS).encode()
    assert gzip.decompress(data) == stream


def test_reader_refuses_what_is_wrong():
    rec, _ = bc.HAND_RECORDS[0]
    with pytest.raises(AssertionError, match="reg2bin"):
        bc.parse_record(bc.encode_record(**rec, bin_=4680)[4:])
    with pytest.raises(AssertionError, match="smallest"):
        bc.sam_line(bc.parse_record(bc.encode_record(**dict(rec, tags=[("NM", "S", 1)]))[4:]), NAMES)
    good = bc.frame_stored(b"x" * 100)
    bad = bytearray(good)
    bad[23] ^= 1                                                   # a payload byte: the CRC no longer holds
    with pytest.raises(AssertionError, match="CRC"):
        bc.bgzf_blocks(bytes(bad))
    with pytest.raises(AssertionError):
        bc.check_stored(bc.bgzf_blocks(bc.frame_stored(b"x" * 10, eof=False) + bc.frame_stored(b"y" * 10)))   # a short block inside
    # the unplaced record's bin, and bins across the levels
    assert bc.reg2bin(-1, 0) == 4680 and bc.reg2bin(0, 1) == 4681 and bc.reg2bin(16383, 16385) == 585 and bc.reg2bin(0, 1 << 29) == 0


# ---- bam_format on the CPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bam_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_check") / "bam_host_check_asan")
    src = os.path.join(PKG, "host", "bam_host_check.cpp")
    assert os.path.exists(src), "host/bam_host_check.cpp: the host build of the BAM record and the BGZF CRC"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def ops_of(cigar):
    return [n << 3 | "MID=X".index(op) for n, op in cigar]


def case(name="r1", seq="ACGTACGTAC", qual=None, mapped=1, seq_id=0, pos=99, dist=1, cost=-2, strand=0, rank=0, cigar=((10, "M"),), nops=None,
         all_=0, n_rep=0, n_hits=0, rname="chrA", paired=0, mate=0, proper=0, rescued=0, mate_mapped=0, mate_seq_id=0, mate_pos=0,
         mate_strand=0, tlen=0, n_conc=0, mate_rname="", mapq=58, md=""):
    """one case of bam_host_check; nops: the row's operations when more than the 64 that are stored"""
    qual = "I" * len(seq) if qual is None else qual
    raw = ("@" + name + "\n" + seq + "\n+\n" + qual + "\n").encode("latin-1")
    rec = (1, len(name), 2 + len(name), len(seq), 5 + len(name) + len(seq), len(qual))
    ops = ops_of(cigar)
    out = struct.pack("<I", len(raw)) + raw + struct.pack("<6I", *rec)
    out += struct.pack("<iiIiiIIIIII", mapped, seq_id, pos, dist, cost, strand, rank, len(ops) if nops is None else nops, all_, n_rep, n_hits)
    out += struct.pack("<I%dH" % len(ops), len(ops), *ops) + struct.pack("<I", len(rname)) + rname.encode()
    out += struct.pack("<IIIIIiIIII", paired, mate, proper, rescued, mate_mapped, mate_seq_id, mate_pos, mate_strand, tlen, n_conc)
    out += struct.pack("<I", len(mate_rname)) + mate_rname.encode() + struct.pack("<i", mapq) + struct.pack("<I", len(md)) + md.encode()
    return out


def host_cases():
    rng = random.Random(5)
    long_seq = "".join(rng.choice("ACGT") for _ in range(131))
    pair = dict(paired=1, mate_mapped=1, mate_seq_id=0, mate_pos=400, mate_rname="chrA", tlen=311, proper=1, n_conc=1)
    cases = {
        "forward": case(),
        "reverse, odd l_seq, MD": case(seq="ACGTTGCAN", strand=1, cigar=((4, "M"), (1, "D"), (5, "M")), md="4^T5", qual="ABCDEFGHI"),
        "unmapped": case(mapped=0, cigar=()),
        "secondary, all hits": case(rank=2, all_=1, n_rep=4, n_hits=70000, strand=1, md="10"),
        "primary, all hits": case(all_=1, n_rep=255, n_hits=256),
        "lent: an unmapped mate borrows RNAME and POS": case(name="frag/2", mapped=0, cigar=(), paired=1, mate=1, mate_mapped=1,
                                                            mate_seq_id=1, mate_pos=16380, mate_strand=1, mate_rname="chrB"),
        "proper pair, mate 1": case(name="frag/1", **pair),
        "proper pair, mate 2, reverse, rescued": case(name="frag/2", mate=1, strand=1, pos=610, rescued=1, **dict(pair, mate_pos=99)),
        "pair on two sequences": case(paired=1, mate_mapped=1, mate_seq_id=1, mate_pos=7, mate_rname="chrB", mate_strand=1),
        "pair, mate unmapped": case(paired=1, mate=0),
        "more than 64 operations": case(seq=long_seq, cigar=tuple((1, "M") for _ in range(64)), nops=131),
        "exactly 64 operations": case(seq="ACGT" * 16, cigar=tuple((1, "MI"[t % 2]) for t in range(64))),
        "negative XG below -128": case(cost=-129),
        "negative XG below -32768": case(cost=-40000, mapq=0),
        "l_seq 0": case(seq="", qual="", cigar=((1, "M"),)),
        "QUAL of another length": case(seq="ACGTA", qual="III"),
        "no QUAL": case(seq="ACGTA", qual=""),
        "a non-IUPAC byte and lower case": case(seq="acgt*-.RYKMswbdhvn=U"),
        "= and X": case(cigar=((4, "="), (1, "X"), (5, "=")), pos=(1 << 14) - 3),
        "131 bases": case(seq=long_seq, cigar=((131, "M"),), pos=(1 << 17) - 100),
    }
    for v in (255, 256, 65535, 65536):
        cases["integer tag at %d" % v] = case(dist=v, all_=1, n_rep=v, n_hits=v)
        cases["XP at %d" % v] = case(**dict(pair, n_conc=v))
    return cases


def test_bam_format_equals_sam_format(bam_check, tmp_path):
    cases = host_cases()
    inp, out = tmp_path / "cases.bin", tmp_path / "out.bin"
    inp.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases.values()))
    r = subprocess.run([bam_check, "records", str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    data, at, seen = out.read_bytes(), 0, {}
    for what in cases:
        n = struct.unpack_from("<Q", data, at)[0]
        sam = data[at + 8:at + 8 + n].decode("latin-1")
        at += 8 + n
        n = struct.unpack_from("<Q", data, at)[0]
        bam = data[at + 8:at + 8 + n]
        at += 8 + n
        assert struct.unpack_from("<i", bam, 0)[0] == len(bam) - 4, what
        rec = bc.parse_record(bam[4:])
        line = bc.sam_line(rec, NAMES)
        want = sam
        if what == "a non-IUPAC byte and lower case":      # SAM keeps the byte, BAM has no code for it
            cols = sam.split("\t")
            cols[9] = "".join(ch if ch in bc.BASES16 else "N" for ch in cols[9])
            want = "\t".join(cols)
            assert want != sam and "=" in cols[9] and "R" in cols[9]
        if what == "QUAL of another length":
            cols = sam.split("\t")
            assert cols[10] == "III" and rec["qual"] == b"\xff" * 5
            cols[10] = "*"
            want = "\t".join(cols)
        assert line == want, what
        seen[what] = (rec, sam)
    assert at == len(data)
    # the fields the cases are there for
    assert seen["unmapped"][0]["bin"] == 4680 and seen["unmapped"][0]["ref_id"] == -1 and seen["unmapped"][0]["pos"] == -1
    lent = seen["lent: an unmapped mate borrows RNAME and POS"][0]
    assert (lent["ref_id"], lent["pos"], lent["next_id"], lent["cigar"], lent["name"]) == (1, 16380, 1, [], "frag")
    assert lent["bin"] == bc.reg2bin(16380, 16381)
    assert seen["more than 64 operations"][0]["cigar"] == [] and "\t*\t" in seen["more than 64 operations"][1]
    assert len(seen["exactly 64 operations"][0]["cigar"]) == 64
    assert seen["secondary, all hits"][0]["seq"] == "" and seen["secondary, all hits"][0]["flag"] == 272
    assert [t[1] for t in seen["secondary, all hits"][0]["tags"]] == ["C", "c", "Z", "C", "C", "I"]
    assert seen["reverse, odd l_seq, MD"][0]["seq"] == "NTGCAACGT" and seen["reverse, odd l_seq, MD"][0]["qual"] == bytes(
        ord(ch) - 33 for ch in "IHGFEDCBA")
    assert seen["proper pair, mate 2, reverse, rescued"][0]["tlen"] == -311 and seen["proper pair, mate 1"][0]["tlen"] == 311
    assert seen["pair on two sequences"][0]["next_id"] == 1 and "\tchrB\t8\t" in seen["pair on two sequences"][1]
    assert seen["negative XG below -128"][0]["tags"][1] == ("XG", "s", -129)
    assert seen["negative XG below -32768"][0]["tags"][1] == ("XG", "i", -40000)
    assert seen["= and X"][0]["cigar"] == [(4, "="), (1, "X"), (5, "=")] and seen["= and X"][0]["bin"] == bc.reg2bin(16381, 16391) == 585
    for v, typ in ((255, "C"), (256, "S"), (65535, "S"), (65536, "I")):
        assert [t[1] for t in seen["integer tag at %d" % v][0]["tags"] if t[0] in ("NM", "NH", "XH")] == [typ] * 3
        assert ("XP", typ, v) in seen["XP at %d" % v][0]["tags"]


def test_header_bytes_equal_the_reader_s(bam_check, tmp_path):
    """bam_header_bytes (csrc/asm_bam.h), what a BAM file call frames as the file's head, against bam_cases.encode_header"""
    cases = {
        "the hand-made references": (b"@HD\tVN:1.6\n", bc.HAND_REFS),
        "no references": (b"@HD\tVN:1.6\n", []),
        "an empty text": (b"", bc.HAND_REFS),
        "a text that ends in an empty line": (b"@HD\tVN:1.6\n@CO\tx\n\n", bc.HAND_REFS),
        "a 255-byte name": (b"@CO\tlong\n", [("n" * 255, 1), ("chrB", 0xffffffff >> 1)]),
    }
    for what, (text, refs) in cases.items():
        inp, out = tmp_path / "header.bin", tmp_path / "header.out"
        inp.write_bytes(struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs)) + b"".join(
            struct.pack("<I", len(name)) + name.encode("latin-1") + struct.pack("<I", length) for name, length in refs))
        r = subprocess.run([bam_check, "header", str(inp), str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (what, r.stderr[-3000:])
        got = out.read_bytes()
        assert got == bc.encode_header(text, refs), what
        assert got[:4] == b"BAM\x01" and struct.unpack_from("<i", got, 4)[0] == len(text), what
    # the reader takes the bytes back
    text, refs = cases["a 255-byte name"]
    assert bc.parse_bam(bc.frame_stored(bc.encode_header(text, refs)))[:2] == (text, refs)


# ---- the container's CRC on the CPU --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
def test_host_crc_and_combine_equal_zlib(bam_check, tmp_path, fill):
    rng = random.Random(11)
    for n in SIZES:
        src = {"zeros": bytes(n), "ones": b"\xff" * n, "random": rng.randbytes(n)}[fill]
        inp, out = tmp_path / "in.bin", tmp_path / "out.bgzf"
        inp.write_bytes(src)
        r = subprocess.run([bam_check, "bgzf", str(inp), str(out), "1"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        printed = [ln.split() for ln in r.stdout.split("\n") if ln]
        want = [src[a:a + bc.PAYLOAD] for a in range(0, n, bc.PAYLOAD)]
        assert [(int(ln), int(crc, 16)) for ln, crc in printed] == [(len(p), zlib.crc32(p)) for p in want], (fill, n)
        data = out.read_bytes()
        assert data == bc.frame_stored(src) and gzip.decompress(data) == src and len(data) == bc.bgzf_bound(n, True)


def test_bgzf_bound(asm):
    lib = asm.load_library()
    for n in SIZES + (3 * 65280 - 1, 1 << 32):
        for eof in (0, 1):
            assert lib.asm_bgzf_bound(n, eof) == bc.bgzf_bound(n, bool(eof)), (n, eof)
    assert asm.OUT_SAM == 0 and asm.OUT_BAM == 1 and asm.BGZF_PAYLOAD == bc.PAYLOAD
    # no device: the setter checks the value first, then the handle
    assert lib.asm_map_set_output_format(None, 2) == -1 and b"format must be" in lib.asm_last_error(None)
    assert lib.asm_map_set_output_format(None, -1) == -1 and b"format must be" in lib.asm_last_error(None)
    assert lib.asm_map_set_output_format(None, 1) == -1 and lib.asm_last_error(None) == b"asm_map_set_output_format: NULL handle"
    assert lib.asm_map_get_output_format(None) == asm.OUT_SAM
