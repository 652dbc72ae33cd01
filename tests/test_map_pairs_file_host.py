"""The device-free side of asm_map_pairs_file (docs/design/mapper.md, "Files: two FASTQ files in, paired SAM out"): the SAM formatter
the kernels compile (csrc/asm_sam.h) built for the host under ASan + UBSan, its paired branches against a formatter written here from
the contract; asm_fastq_cut_n against a Python line counter; the reader policy that keeps two files in step (FastqPairFill) through
host/asm_host_check.cpp; and the call's argument checks with a NULL handle."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

from tests.test_map_file_host import PKG, comp, pack_case, san_flags, up


# ---- the paired lines of the formatter ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sam_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sam_pairs_check") / "sam_host_check_asan")
    src = os.path.join(PKG, "host", "sam_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall"] + san_flags() + ["-o", exe, src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def pair_name(name):
    return name[:-2] if len(name) >= 2 and name[-2] == "/" and name[-1] in "12" else name


def py_pair_line(c):
    """mate x of a pair by the contract (write_pairs of host/asm_map.cpp without --all-hits); c describes record x, c["mate_*"] record y"""
    x, mapped, mate_mapped = c["mate"], bool(c["mapped"]), bool(c["mate_mapped"])
    flag = 1 | (2 if c["proper"] else 0) | (0 if mapped else 4) | (0 if mate_mapped else 8) | (64 if x == 0 else 128)
    if mapped and c["strand"]:
        flag |= 16
    if mate_mapped and c["mate_strand"]:
        flag |= 32
    own = (c["seq_id"], c["rname"], c["pos"] + 1)
    other = (c["mate_seq_id"], c["mate_rname"], c["mate_pos"] + 1)
    none = (-1, "*", 0)
    mine = own if mapped else other if mate_mapped else none  # RNAME and POS: the record's own, else its mapped mate's
    theirs = other if mate_mapped else own if mapped else none
    rnext = "*" if not mate_mapped else "=" if theirs[0] == mine[0] else theirs[1]
    plus = 0 if (mine[2] if x == 0 else theirs[2]) <= (theirs[2] if x == 0 else mine[2]) else 1
    tlen = c["tlen"] if x == plus else -c["tlen"]
    seq, qual = up(c["seq"]), c["qual"]
    cigar, mapq = "*", 0
    if mapped:
        if c["strand"]:
            seq = "".join(comp(b) for b in reversed(seq))
            qual = qual[::-1]
        if c["nops"] <= 64:
            cigar = "".join("%d%s" % (o >> 3, "MID=X???"[o & 7]) for o in c["ops"][:c["nops"]])
        mapq = min(254, 60 + c["cost"])
    line = "%s\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s" % (pair_name(c["name"]), flag, mine[1], mine[2], mapq, cigar, rnext, theirs[2], tlen,
                                                       seq or "*", qual or "*")
    if mapped:
        line += "\tNM:i:%d\tXG:i:%d" % (c["dist"], c["cost"])
    if c["proper"]:
        line += "\tXP:i:%d" % c["n_concordant"]
    if c["rescued"]:
        line += "\tXR:i:1"
    return line + "\n"


def pack_pair_case(rng, c):
    rn = c["mate_rname"].encode()
    out = pack_case(rng, c)
    out += struct.pack("<IIIIIiIIII", 1, c["mate"], c["proper"], c["rescued"], c["mate_mapped"], c["mate_seq_id"], c["mate_pos"], c["mate_strand"],
                       c["tlen"], c["n_concordant"])
    return out + struct.pack("<I", len(rn)) + rn


RNAMES = ["chrA", "chr" + "B" * 70, "c"]


def make_pair_cases(seed=23):
    rng = random.Random(seed)
    cases = []

    def case(**kw):
        m = kw.pop("m", rng.choice([1, 40, 63, 64, 65, 100, 300, 511]))
        sid, mid = rng.randrange(3), rng.randrange(3)
        c = dict(name="frag%d" % rng.randrange(10**6), seq="".join(rng.choice("ACGTNacgtn") for _ in range(m)),
                 qual="".join(chr(rng.randrange(33, 127)) for _ in range(m)), mapped=1, seq_id=sid, pos=rng.choice([0, 9, 99, 12345, 2**31, 2**32 - 2]),
                 dist=rng.randrange(16), cost=rng.randrange(0, 301), strand=rng.randrange(2), rank=0, all=0, nrep=1, nh=1, nops=rng.choice([1, 3, 31, 64]),
                 mate=rng.randrange(2), proper=0, rescued=0, mate_mapped=1, mate_seq_id=mid, mate_pos=rng.choice([0, 7, 100, 12345, 2**31 + 5]),
                 mate_strand=rng.randrange(2), tlen=rng.choice([0, 1, 250, 8192, 99999]), n_concordant=rng.choice([0, 1, 12, 4 * 10**9]))
        c.update(kw)
        c["rname"], c["mate_rname"] = RNAMES[c["seq_id"]], RNAMES[c["mate_seq_id"]]
        if c["mapped"] and c["mate_mapped"] and c["seq_id"] != c["mate_seq_id"]:
            c["tlen"] = 0  # mates on different sequences have no template length
        if not (c["mapped"] and c["mate_mapped"]):
            c["tlen"], c["proper"] = 0, 0
        c["ops"] = [(rng.choice([1, 9, 10, 100, 511]) << 3) | rng.randrange(5) for _ in range(min(c["nops"], 64))]
        cases.append(c)

    for mate in (0, 1):
        # proper pairs on both strand layouts, either mate in front
        for strand in (0, 1):
            for pos, mpos in ((1000, 1300), (1300, 1000)):
                case(mate=mate, proper=1, strand=strand, mate_strand=1 - strand, seq_id=1, mate_seq_id=1, pos=pos, mate_pos=mpos, tlen=400, n_concordant=3)
        # one mate unmapped: RNAME and POS borrowed, RNEXT '=' on that line and '*' on the other
        for strand in (0, 1):
            case(mate=mate, mapped=0, mate_mapped=1, mate_strand=strand)
            case(mate=mate, mapped=1, mate_mapped=0, strand=strand)
        # both unmapped (and the lines of an unsent pair), lengths the mapper never sees
        for m in (0, 5, 512, 600):
            case(mate=mate, mapped=0, mate_mapped=0, m=m, qual=None)
        # mates on different sequences: RNEXT is a name, TLEN 0
        case(mate=mate, seq_id=0, mate_seq_id=1)
        case(mate=mate, seq_id=2, mate_seq_id=0, strand=1)
        # equal POS: mate 1 takes '+'
        case(mate=mate, seq_id=0, mate_seq_id=0, pos=500, mate_pos=500, tlen=120, proper=1, n_concordant=1)
        case(mate=mate, seq_id=0, mate_seq_id=0, pos=500, mate_pos=500, tlen=0)
        # a rescued record, and the mate of one
        case(mate=mate, proper=1, rescued=1, seq_id=1, mate_seq_id=1, pos=100, mate_pos=350, tlen=350, n_concordant=0)
        case(mate=mate, proper=1, rescued=0, seq_id=1, mate_seq_id=1, pos=350, mate_pos=100, tlen=350, n_concordant=0)
        # a CIGAR above 64 operations
        case(mate=mate, nops=65)
        case(mate=mate, nops=255, strand=1)
        # empty SEQ and QUAL, QUAL '*'
        case(mate=mate, mapped=0, m=0, qual="")
        case(mate=mate, mapped=0, mate_mapped=0, m=7, qual="")
        case(mate=mate, qual="*", strand=1)
        # a negative Greedy cost, and MAPQ's cap
        for cost in (-1, -60, -61, -200, 193, 194, 195, 1000):
            case(mate=mate, cost=cost)
        # names: /1 and /2 go, /3 and a bare '/' stay
        for name in ("frag7/1", "frag7/2", "frag7/3", "/", "/1", "/2", "a/", "1", "x/12", "", "frag/1/2"):
            case(mate=mate, name=name)
            case(mate=mate, name=name, mapped=0)
    for _ in range(300):
        same = rng.random() < 0.6
        sid = rng.randrange(3)
        case(mapped=int(rng.random() < 0.8), mate_mapped=int(rng.random() < 0.8), proper=int(rng.random() < 0.5), rescued=int(rng.random() < 0.1),
             seq_id=sid, mate_seq_id=sid if same else rng.randrange(3))
    for c in cases:
        if c["qual"] is None:
            c["qual"] = "".join(chr(rng.randrange(33, 127)) for _ in c["seq"])
    return rng, cases


def test_paired_formatter_on_the_cpu_equals_python_under_sanitizers(sam_check, tmp_path):
    rng, cases = make_pair_cases()
    fin, fout = tmp_path / "cases.bin", tmp_path / "lines.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(pack_pair_case(rng, c))
    r = subprocess.run([sam_check, str(fin), str(fout), "--pairs"], capture_output=True, text=True, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    data = open(fout, "rb").read()
    at = 0
    for t, c in enumerate(cases):
        want = py_pair_line(c).encode("latin-1")
        (size,) = struct.unpack_from("<Q", data, at)
        got = data[at + 8:at + 8 + size]
        assert got == want, (t, c, got, want)  # the lane sink's bytes
        assert size == len(want), (t, c, size, len(want))  # the size sink's count
        at += 8 + size
    assert at == len(data)
    flags = {int(py_pair_line(c).split("\t")[1]) for c in cases}
    assert {99, 147, 83, 163, 77, 141, 73, 133, 69, 137} <= flags


# ---- asm_fastq_cut_n ----------------------------------------------------------------------------------------------------------------
def cut_n(asm, data: bytes, max_records: int):
    lib = asm.load_library()
    n = ctypes.c_int64(-1)
    buf = ctypes.create_string_buffer(data, len(data) + 1)
    size = lib.asm_fastq_cut_n(buf, len(data), max_records, ctypes.byref(n))
    return int(size), int(n.value)


def py_cut_n(data: bytes, max_records: int):
    ends = [i + 1 for i, c in enumerate(data) if c == 10]
    whole = min(len(ends) // 4, max_records)
    return (ends[4 * whole - 1] if whole else 0), whole


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_fastq_cut_n_equals_a_line_counter(asm, eol):
    rng = random.Random(31 if eol == "\n" else 32)
    for trial in range(30):
        n = rng.randrange(0, 9)
        data = "".join("@r%d%s%s%s+%s%s%s" % (t, eol, "ACGT" * rng.randrange(0, 9), eol, eol, "I" * rng.randrange(0, 30), eol) for t in range(n)).encode()
        for text in (data, data[:-len(eol)] if data else data, data[:rng.randrange(len(data) + 1)]):  # whole, no final newline, any prefix
            for k in sorted({0, 1, n - 1, n, n + 1, n + 5} - {-1}):
                assert cut_n(asm, text, k) == py_cut_n(text, k), (trial, k, text)
    lib = asm.load_library()
    assert cut_n(asm, b"\n\n\n\n\n\n\n\n", 1) == (4, 1) and cut_n(asm, b"\n\n\n\n\n\n\n\n", 2) == (8, 2) and cut_n(asm, b"\n\n\n", 1) == (0, 0)
    assert lib.asm_fastq_cut_n(None, 100, 3, None) == 0


# ---- the reader policy ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_check") / "asm_host_check_asan")
    src = os.path.join(PKG, "host", "asm_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def mates_text(rng, n, lo, hi):
    out = []
    for t in range(n):
        m = rng.randrange(lo, hi + 1)
        out.append("@frag%d\n%s\n+\n%s\n" % (t, "".join(rng.choice("ACGT") for _ in range(m)), "".join(chr(rng.randrange(33, 74)) for _ in range(m))))
    return out


def run_pairs(host_check, tmp_path, data1: bytes, data2: bytes, chunk: int):
    f1, f2, out = tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "chunks.bin"
    f1.write_bytes(data1)
    f2.write_bytes(data2)
    r = subprocess.run([host_check, "--pairs", str(f1), str(f2), str(chunk), str(out)], capture_output=True, text=True, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    data = out.read_bytes()
    chunks, at = [], 0
    while True:
        (units,) = struct.unpack_from("<Q", data, at)
        if units == 2**64 - 1:
            break
        units, bytes1, size = struct.unpack_from("<QQQ", data, at)
        chunks.append((units, bytes1, data[at + 24:at + 24 + size]))
        at += 24 + size
    failed, carry_peak, n1, n2, e1, e2, m1, m2 = struct.unpack_from("<8Q", data, at + 8)
    assert at + 72 == len(data)
    return chunks, dict(failed=failed, carry_peak=carry_peak, records=(n1, n2), extra_lines=(e1, e2), more=(m1, m2))


def regions(chunks):
    """both files as the chunks restore them; every chunk must hold `units` whole records in each region"""
    got = [b"", b""]
    for units, bytes1, data in chunks:
        for f, part in enumerate((data[:bytes1], data[bytes1:])):
            assert part.count(b"\n") == 4 * units and (part == b"" or part.endswith(b"\n")), (units, f)
            got[f] += part
    return got


def test_reader_keeps_two_files_in_step(host_check, tmp_path):
    rng = random.Random(77)
    r1, r2 = mates_text(rng, 2000, 40, 40), mates_text(rng, 2000, 300, 300)
    d1, d2 = "".join(r1).encode(), "".join(r2).encode()
    chunk = 64 << 10
    chunks, end = run_pairs(host_check, tmp_path, d1, d2, chunk)
    assert not end["failed"] and len(chunks) > 10
    assert regions(chunks) == [d1, d2]
    assert sum(c[0] for c in chunks) == 2000 and end["records"] == (2000, 2000)
    assert end["extra_lines"] == (0, 0) and end["more"] == (0, 0)
    assert 0 < end["carry_peak"] <= chunk
    # one file holds a record more: every pair in front of it comes through, then the policy says which file goes on
    for longer in (0, 1):
        a, b = (d1, "".join(r2[:1999]).encode()) if longer == 0 else ("".join(r1[:1999]).encode(), d2)
        chunks, end = run_pairs(host_check, tmp_path, a, b, chunk)
        assert not end["failed"] and regions(chunks) == [d1[:len("".join(r1[:1999]))], d2[:len("".join(r2[:1999]))]]
        assert end["more"] == ((1, 0) if longer == 0 else (0, 1)) and end["extra_lines"] == (0, 0) and min(end["records"]) == 1999
    # a truncated last record in either file (its last line is missing)
    for f in (0, 1):
        cutrec = (r1, r2)[f][1999]
        short = cutrec[:cutrec.rstrip("\n").rfind("\n") + 1].encode()
        a = "".join(r1[:1999]).encode() + (short if f == 0 else r1[1999].encode())
        b = "".join(r2[:1999]).encode() + (short if f == 1 else r2[1999].encode())
        chunks, end = run_pairs(host_check, tmp_path, a, b, chunk)
        assert not end["failed"] and sum(c[0] for c in chunks) == 1999
        assert end["extra_lines"] == ((3, 0) if f == 0 else (0, 3)) and end["records"][f] == 1999 and end["records"][1 - f] == 2000


# ---- rejections -----------------------------------------------------------------------------------------------------------------------
def test_map_pairs_file_rejections(asm):
    lib = asm.load_library()
    MP, PP = asm.MapParams, asm.PairParams
    dummy = ctypes.create_string_buffer(64)
    names = (ctypes.c_char_p * 1)(b"chr1")
    base = dict(ix=dummy, names=names, f1=b"r1.fq", f2=b"r2.fq", sam=b"out.sam", p=MP(2, 1, 0, 3), pp=PP(100, 500, -1), chunk_bytes=0)

    def call(**kw):
        a = dict(base, **kw)
        rc = lib.asm_map_pairs_file(None, a["ix"], a["names"], a["f1"], a["f2"], a["sam"], None, None if a["p"] is None else ctypes.byref(a["p"]),
                                    None if a["pp"] is None else ctypes.byref(a["pp"]), a["chunk_bytes"], None)
        return int(rc), lib.asm_last_error(None).decode()

    for kw in (dict(f1=None), dict(f2=None), dict(sam=None), dict(names=None), dict(p=None), dict(pp=None), dict(ix=None)):
        assert call(**kw) == (-1, "asm_map_pairs_file: bad arguments"), kw
    assert call(chunk_bytes=-1) == (-1, "asm_map_pairs_file: chunk_bytes must be >= 0")
    assert call(p=MP(16, 1, 0, 3)) == (-1, "asm_map_pairs_file: max_errors must be in [0, 15]")
    assert call(p=MP(2, 0, 0, 3)) == (-1, "asm_map_pairs_file: both_strands must be 1")
    assert call(p=MP(2, 1, -1, 3)) == (-1, "asm_map_pairs_file: max_occ must be >= 0")
    assert call(p=MP(2, 1, 0, 51)) == (-1, "asm_map_pairs_file: greedy_k must be in [0, 50]")
    for pp in (PP(-1, 500, -1), PP(600, 500, -1), PP(0, 8193, -1)):
        assert call(pp=pp) == (-1, "asm_map_pairs_file: need 0 <= min_insert <= max_insert <= 8192")
    for resc in (-2, 16):
        assert call(pp=PP(100, 500, resc)) == (-1, "asm_map_pairs_file: rescue_errors must be -1 (off) or in [0, 15]")
    assert call() == (-1, "asm_map_pairs_file: NULL handle")  # nothing was opened, created or touched before this
    assert not os.path.exists("out.sam")
