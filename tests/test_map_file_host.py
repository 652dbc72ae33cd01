"""The device-free side of asm_map_file (docs/design/mapper.md, "Files: FASTQ in, SAM out"): asm_fastq_cut against a Python line
splitter, the SAM formatter the kernels compile (csrc/asm_sam.h) built for the host under ASan + UBSan against a formatter written
here, and the call's argument checks with a NULL handle, whole messages pinned in tests/golden/map_file_rejections.json."""
import ctypes
import json
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "map_file_rejections.json")


# ---- asm_fastq_cut ------------------------------------------------------------------------------------------------------------
def cut(asm, data: bytes):
    lib = asm.load_library()
    n = ctypes.c_int64(-1)
    buf = ctypes.create_string_buffer(data, len(data) + 1)
    size = lib.asm_fastq_cut(buf, len(data), ctypes.byref(n))
    return int(size), int(n.value)


def py_cut(data: bytes):
    ends = [i + 1 for i, c in enumerate(data) if c == 10]
    whole = len(ends) // 4
    return (ends[4 * whole - 1] if whole else 0), whole


def py_records(data: bytes):
    """(header, seq, qual) of a buffer of whole records, CR stripped"""
    lines = data.split(b"\n")
    assert lines[-1] == b""
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines[:-1]]
    assert len(lines) % 4 == 0
    return [(lines[i], lines[i + 1], lines[i + 3]) for i in range(0, len(lines), 4)]


def random_fastq(rng, n, eol):
    out = []
    for t in range(n):
        m = rng.choice([0, 1, 5, 30, 100])
        seq = "".join(rng.choice("ACGTNacgt") for _ in range(m))
        qual = "".join(chr(rng.randrange(33, 127)) for _ in range(m))
        if m and rng.random() < 0.3:
            qual = rng.choice("@+") + qual[1:]
        out.append("@r%d %s%s%s%s+%s%s%s" % (t, "x" * rng.randrange(4), eol, seq, eol, eol, qual, eol))
    return "".join(out).encode()


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_fastq_cut_equals_a_line_splitter(asm, eol):
    rng = random.Random(5 if eol == "\n" else 6)
    for trial in range(40):
        data = random_fastq(rng, rng.randrange(0, 12), eol)
        for _ in range(8):
            k = rng.randrange(len(data) + 1)
            assert cut(asm, data[:k]) == py_cut(data[:k])
    assert cut(asm, b"") == (0, 0)
    assert cut(asm, b"\n\n\n") == (0, 0) and cut(asm, b"\n\n\n\n") == (4, 1)


def test_fastq_cut_at_every_offset_and_reassembly(asm):
    rng = random.Random(9)
    data = random_fastq(rng, 9, "\n") + random_fastq(rng, 4, "\r\n")
    want = py_records(data)
    for k in range(len(data) + 1):
        assert cut(asm, data[:k]) == py_cut(data[:k]), k
    for step in (1, 7, 64, 200, len(data)):
        # the reader's loop: the carry of the chunk before, then `step` more bytes, cut behind the last whole record
        got, carry, pos = [], b"", 0
        while pos < len(data):
            buf = carry + data[pos:pos + step]
            pos += step
            size, n = cut(asm, buf)
            recs = py_records(buf[:size])
            assert len(recs) == n
            got += recs
            carry = buf[size:]
        assert carry == b"" and got == want, step


# ---- the formatter on the CPU ---------------------------------------------------------------------------------------------------
SAN_FLAGS = None


def san_flags():
    """SAN_FLAGS of oracle/Makefile"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        for line in fh:
            if line.startswith("SAN_FLAGS :="):
                return line.split(":=", 1)[1].split()
    raise AssertionError("oracle/Makefile has no SAN_FLAGS")


@pytest.fixture(scope="module")
def sam_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sam_check") / "sam_host_check_asan")
    src = os.path.join(PKG, "host", "sam_host_check.cpp")
    assert os.path.exists(src), "host/sam_host_check.cpp: the host build of the SAM formatter"
    r = subprocess.run(["g++", "-std=c++17", "-Wall"] + san_flags() + ["-o", exe, src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def up(s):
    return "".join(chr(ord(c) - 32) if "a" <= c <= "z" else c for c in s)


def comp(c):
    return {"A": "T", "T": "A", "C": "G", "G": "C"}.get(c, c)


def py_line(c):
    """the line asm-map writes (host/asm_map.cpp) for one case"""
    name, seq, qual = c["name"], up(c["seq"]), c["qual"]
    if not c["mapped"]:
        return "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (name, seq or "*", qual or "*")
    if c["strand"]:
        seq = "".join(comp(x) for x in reversed(seq))
        qual = qual[::-1]
    rank = c["rank"]
    cigar = "*" if c["nops"] > 64 else "".join("%d%s" % (o >> 3, "MID=X???"[o & 7]) for o in c["ops"][:c["nops"]])
    line = "%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tXG:i:%d" % (
        name, (16 if c["strand"] else 0) | (256 if rank else 0), c["rname"], c["pos"] + 1, min(254, 60 + c["cost"]), cigar,
        "*" if rank else seq, "*" if rank or not qual else qual, c["dist"], c["cost"])
    if c["all"]:
        line += "\tNH:i:%d\tHI:i:%d\tXH:i:%d" % (c["nrep"], rank + 1, c["nh"])
    return line + "\n"


def pack_case(rng, c):
    """the record's fields somewhere inside a raw buffer, as the device sees them"""
    pad = lambda: "".join(rng.choice("ACGT@+\n\r") for _ in range(rng.randrange(0, 9)))  # noqa: E731
    raw, where = pad(), []
    for field in (c["name"], c["seq"], c["qual"]):
        where += [len(raw), len(field)]
        raw += field + pad()
    rawb, rname = raw.encode("latin-1"), c["rname"].encode()
    stored = c["ops"][:64]
    out = struct.pack("<I", len(rawb)) + rawb + struct.pack("<6I", *where)
    out += struct.pack("<iiIiiIIIIII", c["mapped"], c["seq_id"], c["pos"], c["dist"], c["cost"], c["strand"], c["rank"], c["nops"], c["all"],
                       c["nrep"], c["nh"])
    out += struct.pack("<I", len(stored)) + struct.pack("<%dH" % len(stored), *stored)
    return out + struct.pack("<I", len(rname)) + rname


def make_cases(seed=17):
    rng = random.Random(seed)
    positions = [0, 8, 9, 10, 98, 99, 100, 999, 1000, 99_999, 100_000, 999_999_999, 1_000_000_000, 2**31 - 1, 2**31, 2**32 - 2]
    lengths = [1, 2, 63, 64, 65, 100, 127, 128, 129, 300, 511, 512, 600, 1000]
    cases = []

    def case(**kw):
        m = kw.pop("m", rng.choice(lengths))
        c = dict(name="r%d" % rng.randrange(10**rng.randrange(1, 9)), seq="".join(rng.choice("ACGTNacgtnRYx.") for _ in range(m)),
                 qual="".join(chr(rng.randrange(33, 127)) for _ in range(m)), mapped=1, seq_id=rng.randrange(3), pos=rng.choice(positions),
                 dist=rng.randrange(16), cost=rng.randrange(0, 301), strand=rng.randrange(2), rank=0, all=0, nrep=1, nh=1,
                 rname="chr%s" % ("X" * rng.randrange(0, 70)))
        nops = rng.choice([1, 2, 3, 5, 31, 63, 64])
        c["nops"] = nops
        c.update(kw)
        c["ops"] = [(rng.choice([1, 9, 10, 99, 100, 511, 1000, 8191]) << 3) | rng.randrange(5) for _ in range(min(c["nops"], 64))]
        if c["all"] and "nrep" not in kw:
            c["nrep"] = rng.randrange(c["rank"] + 1, 257)
            c["nh"] = c["nrep"] + rng.choice([0, 0, 5, 10**6])
        cases.append(c)

    for pos in positions:  # every width of POS
        case(pos=pos)
    for cost in list(range(0, 301, 7)) + [193, 194, 195, 300]:  # MAPQ saturates at 254
        case(cost=cost)
    for nops in (64, 65, 255):  # 64 operations are written, 65 give '*'
        case(nops=nops)
        case(nops=nops, all=1, rank=3)
    for m in lengths:  # both strands at every length, and the lengths the mapper never sees (unmapped lines)
        case(m=m, strand=0)
        case(m=m, strand=1)
        case(m=m, mapped=0)
    for _ in range(40):  # secondary ranks: SEQ and QUAL '*'
        case(all=1, rank=rng.randrange(0, 256))
    case(qual="*", strand=1)  # QUAL '*' stays '*'
    case(qual="*", strand=0)
    case(qual="", strand=1)
    case(m=0, qual="", mapped=0)  # empty SEQ and QUAL
    case(m=0, qual="II", mapped=0)
    case(m=5, qual="", mapped=0)
    case(name="", mapped=0)
    case(name="", strand=1)
    case(dist=0, cost=0, pos=0)
    for _ in range(300):
        case(mapped=rng.randrange(4) > 0, all=rng.randrange(2), rank=rng.choice([0, 0, 1, 9, 10, 255]))
    for c in cases:
        if not c["all"]:
            c["rank"] = 0
    return rng, cases


def test_formatter_on_the_cpu_equals_python_under_sanitizers(sam_check, tmp_path):
    rng, cases = make_cases()
    fin, fout = tmp_path / "cases.bin", tmp_path / "lines.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(pack_case(rng, c))
    r = subprocess.run([sam_check, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    data = open(fout, "rb").read()
    at = 0
    for t, c in enumerate(cases):
        want = py_line(c).encode("latin-1")
        (size,) = struct.unpack_from("<Q", data, at)
        assert size == len(want), (t, c, size, len(want))
        got = data[at + 8:at + 8 + size]
        assert got == want, (t, c, got, want)
        at += 8 + size
    assert at == len(data)


# ---- rejections -------------------------------------------------------------------------------------------------------------------
def rejection_cases(asm):
    lib = asm.load_library()
    MP = asm.MapParams
    dummy = ctypes.create_string_buffer(64)
    names = (ctypes.c_char_p * 1)(b"chr1")
    base = dict(ix=dummy, names=names, fastq=b"reads.fq", sam=b"out.sam", p=MP(2, 1, 0, 3), max_hits=0, strata=0, chunk_bytes=0)
    out = []

    def add(label, **kw):
        a = dict(base, **kw)
        p = None if a["p"] is None else ctypes.byref(a["p"])
        out.append((label, lambda: lib.asm_map_file(None, a["ix"], a["names"], a["fastq"], a["sam"], None, p, a["max_hits"], a["strata"],
                                                    a["chunk_bytes"], None)))

    add("fastq_path=NULL", fastq=None)
    add("sam_path=NULL", sam=None)
    add("seq_names=NULL", names=None)
    add("params=NULL", p=None)
    add("index=NULL", ix=None)
    for mh in (-1, 257):
        add("max_hits=%d" % mh, max_hits=mh)
    for s in (-1, 16):
        add("strata=%d with max_hits=4" % s, max_hits=4, strata=s)
    add("chunk_bytes=-1", chunk_bytes=-1)
    for e in (-1, 16):
        add("max_errors=%d" % e, p=MP(e, 1, 0, 3))
    add("both_strands=2", p=MP(2, 2, 0, 3))
    add("max_occ=-1", p=MP(2, 1, -1, 3))
    add("greedy_k=51", p=MP(2, 1, 0, 51))
    add("max_hits and max_errors bad", max_hits=257, p=MP(16, 1, 0, 3))
    add("strata=-1 with max_hits=0: no handle", strata=-1)
    add("no handle", max_hits=0)
    add("no handle, max_hits=256 strata=15", max_hits=256, strata=15)
    return out


def replay(asm):
    lib = asm.load_library()
    return [[label, int(thunk()), lib.asm_last_error(None).decode()] for label, thunk in rejection_cases(asm)]


def test_map_file_rejections_are_pinned(asm):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = replay(asm)
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert g == w
        assert g[1] in (-1,) and g[2].startswith("asm_map_file: ")
    text = {g[0]: g[2] for g in got}
    assert text["max_hits=257"] == "asm_map_file: max_hits must be in [0, 256]"
    assert text["strata=16 with max_hits=4"] == "asm_map_file: strata must be in [0, 15]"
    assert text["chunk_bytes=-1"] == "asm_map_file: chunk_bytes must be >= 0"
    assert text["fastq_path=NULL"] == "asm_map_file: bad arguments"
    assert text["no handle"] == text["strata=-1 with max_hits=0: no handle"] == "asm_map_file: NULL handle"


if __name__ == "__main__":
    import sys

    sys.path.insert(0, ROOT)
    import approximate_string_matching_amd

    if "--record" in sys.argv:
        with open(GOLDEN, "w") as fh:
            json.dump(replay(approximate_string_matching_amd), fh, indent=1)
            fh.write("\n")
    else:
        print(json.dumps(replay(approximate_string_matching_amd), indent=1))
