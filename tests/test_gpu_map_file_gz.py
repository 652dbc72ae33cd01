"""asm_map_file / asm_map_file_sorted / asm-map --stream on a BGZF-compressed FASTQ (docs/design/mapper.md, "Compressed input"): the
SAM or BAM bytes equal those of the same call on the inflated text, whatever the member cut, chunk_bytes and ASM_MAP_CHUNK are; the
errors are the plain call's, and corrupt members, plain gzip and an EOF-only file give what the contract says.  About 2 000 reads of 30
to 150 bp against a 20 kbp reference, both strands, e = 2.  The containers are built from the corpus builder's encoders, whose members
tests/test_inflate_host.py runs through the host build of the decoder under ASan + UBSan."""
import gzip
import os
import random
import subprocess
import sys

import pytest

from tests import bgzf_in_cases as bi
from tests.test_map_host import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
NAMES, K, E, HEADER = ["chr1"], 12, 2, "@HD\tVN:1.6\n"


def make_text(n=2000, seed=5, eol="\n"):
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(20_000))
    out = []
    for t in range(n):
        m = rng.randint(30, 150)
        a = rng.randrange(len(ref) - m)
        s = list(ref[a:a + m])
        for _ in range(rng.randrange(3)):
            s[rng.randrange(m)] = rng.choice("ACGT")
        s = "".join(s)
        if t % 2:
            s = revcomp(s)
        if t % 17 == 0:
            s = "".join(rng.choice("ACGT") for _ in range(m))
        end = "\r\n" if t % 5 == 0 else eol
        out.append("@r%d extra%s%s%s+%s%s%s" % (t, end, s, end, end, "".join(chr(rng.randrange(33, 74)) for _ in range(m)), end))
    return ref, "".join(out).encode()


def cut_members(text, sizes):
    out, at, k = [], 0, 0
    while at < len(text):
        part = text[at:at + sizes[k % len(sizes)]]
        out.append(bi.good_member(bi.deflate(part, level=(1, 6, 9)[k % 3]), part))
        at, k = at + len(part), k + 1
    return b"".join(out)


@pytest.fixture(scope="module")
def data(asm, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gz")
    ref, text = make_text()
    files = {"text": text,
             "bgzip": cut_members(text, [65280]) + bi.EOF_BLOCK,
             "rotation": bi.EOF_BLOCK + cut_members(text, [1, 7, 4099]),          # an empty member in front, no EOF block
             "own": asm.bgzf_compress_host(text, eof=True, level=asm.BGZF_DEFLATE)}
    paths = {}
    for name, body in files.items():
        paths[name] = str(tmp / (name + (".fq" if name == "text" else ".fq.gz")))
        with open(paths[name], "wb") as fh:
            fh.write(body)
    (tmp / "ref.fa").write_text(">chr1\n" + ref + "\n")
    return dict(ref=ref, text=text, paths=paths, tmp=tmp, fa=str(tmp / "ref.fa"))


@pytest.fixture(scope="module")
def own(asm):
    eng = asm.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def index(own, data):
    return own.build_index([data["ref"]], k=K)


VARIANTS = {
    "best": dict(max_hits=0), "all": dict(max_hits=4, strata=1), "sorted": dict(max_hits=0, sort=True),
    "bam0": dict(max_hits=0, fmt="bam", level=0), "bam1": dict(max_hits=4, strata=1, fmt="bam", level=1), "md": dict(max_hits=0, md=True),
}


def run(own, index, src, dst, fmt="sam", level=0, md=False, **kw):
    own.set_output_format(fmt)
    own.set_bgzf_level(level)
    own.set_sam_tags(md=md)
    try:
        st = own.map_file(index, NAMES, src, str(dst), E, header=HEADER, **kw)
    finally:
        own.set_output_format("sam"), own.set_bgzf_level(0), own.set_sam_tags(md=False)
    with open(dst, "rb") as fh:
        return fh.read(), st


@pytest.fixture(scope="module")
def plain(own, index, data):
    return {v: run(own, index, data["paths"]["text"], data["tmp"] / ("plain_" + v), **kw) for v, kw in VARIANTS.items()}


@pytest.mark.parametrize("cut", ["bgzip", "rotation", "own"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bytes_equal_the_plain_call(own, index, data, plain, cut, variant):
    want, st0 = plain[variant]
    assert len(want) > 100_000 or variant.startswith("bam")
    for chunk in (512, 4096, 0):
        got, st = run(own, index, data["paths"][cut], data["tmp"] / "out", chunk_bytes=chunk, **VARIANTS[variant])
        assert got == want, (cut, variant, chunk)
        assert st["bytes_in"] == len(data["text"]) == st0["bytes_in"]
        assert (st["reads"], st["mapped"], st["records"], st["bytes_out"]) == (st0["reads"], st0["mapped"], st0["records"], st0["bytes_out"])


CHILD = """
import sys
sys.path.insert(0, %r)
import approximate_string_matching_amd as asm
eng = asm.Engine(0)
ix = eng.build_index([open(sys.argv[1]).read().split("\\n")[1]], k=%d)
eng.map_file(ix, ["chr1"], sys.argv[2], sys.argv[3], %d, max_hits=4, strata=1, header=%r, chunk_bytes=4096)
"""


def test_small_device_chunk_in_a_child(data, plain, tmp_path):
    """ASM_MAP_CHUNK is read when a handle is created: a fresh child process"""
    out = tmp_path / "child.sam"
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, K, E, HEADER), data["fa"], data["paths"]["rotation"], str(out)], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, ASM_MAP_CHUNK="7"), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == plain["all"][0]


def both_errors(asm, own, index, text, tmp_path, **kw):
    """the error of the plain call on `text` and of the call on its compressed form, in members of 1, 7 and 4 099 bytes"""
    msgs = []
    for name, body in (("t.fq", text), ("t.fq.gz", cut_members(text, [4099, 1, 7]) + bi.EOF_BLOCK)):
        (tmp_path / name).write_bytes(body)
        with pytest.raises(asm.AsmError) as err:
            own.map_file(index, NAMES, str(tmp_path / name), str(tmp_path / "o.sam"), E, **kw)
        msgs.append((err.value.code, str(err.value)))
    return msgs


def test_record_errors_are_the_plain_calls(asm, own, index, data, plain, tmp_path):
    text = data["text"]
    # a missing final newline is no error: the same bytes
    (tmp_path / "open.fq.gz").write_bytes(cut_members(text[:-1], [4099, 1, 7]) + bi.EOF_BLOCK)
    got, _ = run(own, index, str(tmp_path / "open.fq.gz"), tmp_path / "o.sam", max_hits=0, chunk_bytes=4096)
    assert got == plain["best"][0]
    lines = text.split(b"\n")
    truncated = b"\n".join(lines[:-3]) + b"\n"                   # the last record loses two lines
    a, b = both_errors(asm, own, index, truncated, tmp_path, chunk_bytes=4096)
    assert a == b and "is truncated" in a[1] and "record 2000 " in a[1]
    k = 4 * 1990
    malformed = b"\n".join(lines[:k] + [b"x" + lines[k][1:]] + lines[k + 1:])
    a, b = both_errors(asm, own, index, malformed, tmp_path, chunk_bytes=4096)
    assert a == b and "record 1991 is malformed" in a[1]


def test_truncated_end_behind_a_malformed_record(asm, own, index, data, tmp_path):
    """Which of two errors wins (docs/design/mapper.md, "Compressed input", File calls).  In one chunk the truncated end is reported
    first, as by the plain call.  With the malformed record in the chunk in front of the last one, the compressed call reports that
    record, since it learns the line count only when it reaches the last chunk; the plain call knows the count when the last chunk
    is read and reports the truncation."""
    lines = data["text"].split(b"\n")
    body = lines[:-3]                                            # the last record loses two lines
    n = len(b"\n".join(body)) + 1
    # members of 4 099, 1 and 7 bytes under chunk_bytes 4 096: chunk 0 is 4 099 bytes of text, every later one 4 107
    bounds = list(range(4099, n, 4107))
    at, k = 0, None
    for i in range(0, len(body), 4):                             # the record that ends 2 000 bytes in front of the last chunk's start
        at += sum(len(ln) + 1 for ln in body[i:i + 4])
        if at > bounds[-1] - 2000:
            k = i
            break
    assert bounds[-2] < at <= bounds[-1]
    bad = b"\n".join(body[:k] + [b"x" + body[k][1:]] + body[k + 1:]) + b"\n"
    (plain_code, plain_msg), (gz_code, gz_msg) = both_errors(asm, own, index, bad, tmp_path, chunk_bytes=4096)
    assert plain_code == gz_code == -1
    assert "record %d is malformed" % (k // 4 + 1) in gz_msg
    assert "is truncated" in plain_msg or "record %d is malformed" % (k // 4 + 1) in plain_msg
    (_, plain_msg), (_, gz_msg) = both_errors(asm, own, index, bad, tmp_path, chunk_bytes=0)
    assert plain_msg == gz_msg and "record 2000 is truncated" in gz_msg


def test_contract_errors_and_empty_files(asm, own, index, data, tmp_path):
    parts = bi.split_members(data["paths"] and open(data["paths"]["bgzip"], "rb").read())
    body = bytearray(open(data["paths"]["bgzip"], "rb").read())
    at = parts[1][0] + len(parts[1][1]) - 8
    body[at] ^= 1                                                # the CRC of member 1
    (tmp_path / "bad.fq.gz").write_bytes(bytes(body))
    for chunk in (4096, 0):
        with pytest.raises(asm.AsmError) as err:
            own.map_file(index, NAMES, str(tmp_path / "bad.fq.gz"), str(tmp_path / "o.sam"), E, chunk_bytes=chunk)
        assert err.value.code == -1 and "BGZF member 1 at offset %d: CRC-32 mismatch" % parts[1][0] in str(err.value)
    (tmp_path / "cut.fq.gz").write_bytes(bytes(body[:parts[2][0] + 40]))      # member 2 reaches past the end; member 1 is reported first
    with pytest.raises(asm.AsmError) as err:
        own.map_file(index, NAMES, str(tmp_path / "cut.fq.gz"), str(tmp_path / "o.sam"), E)
    assert "BGZF member 1 at offset" in str(err.value)
    good = open(data["paths"]["bgzip"], "rb").read()
    (tmp_path / "tail.fq.gz").write_bytes(good + b"junk")
    with pytest.raises(asm.AsmError) as err:
        own.map_file(index, NAMES, str(tmp_path / "tail.fq.gz"), str(tmp_path / "o.sam"), E)
    assert err.value.code == -1 and "BGZF member %d at offset %d: not a BGZF member header" % (len(parts), len(good)) in str(err.value)
    (tmp_path / "plain.fq.gz").write_bytes(gzip.compress(data["text"]))
    with pytest.raises(asm.AsmError) as err:
        own.map_file(index, NAMES, str(tmp_path / "plain.fq.gz"), str(tmp_path / "o.sam"), E)
    assert err.value.code == -4 and "plain gzip" in str(err.value) and "bgzip" in str(err.value)
    (tmp_path / "eof.fq.gz").write_bytes(bi.EOF_BLOCK)
    got, st = run(own, index, str(tmp_path / "eof.fq.gz"), tmp_path / "o.sam", max_hits=0)
    assert got == HEADER.encode() and st["reads"] == 0 and st["bytes_in"] == 0


def test_tool_takes_the_gz_file(data, tmp_path):
    outs = []
    for src in (data["paths"]["text"], data["paths"]["rotation"]):
        out = tmp_path / "tool.sam"
        r = subprocess.run([EXE, "-r", data["fa"], "-q", src, "-o", str(out), "-e", str(E), "--both-strands", "--stream", "--chunk-bytes", "4096"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([ln for ln in out.read_bytes().split(b"\n") if not ln.startswith(b"@PG")])      # @PG names the command line
    assert outs[0] == outs[1] and len(outs[0]) > 2000
