"""Deflate-compressed BAM from the device (docs/design/mapper.md, "Deflate"): asm_bgzf_compress on the corpus of
tests/deflate_cases.py against the host build of the same encoder, then the four file calls at ASM_BGZF_DEFLATE on the inputs of
tests/test_gpu_bam.py (1,500 reads and 760 pairs: every record stream is at least three blocks long).  The SAM file and the level-0
BAM file of the same call are the references; zlib inflates every block."""
import os
import subprocess
import sys

import pytest

from tests import bam_cases as bc
from tests import deflate_cases as dc
from tests.test_gpu_bam import E, EXE, HEADER, LIMIT, header_stream, inputs, own, run  # noqa: F401 (inputs, own: fixtures)
from tests.test_gpu_md import K, NAMES, ref, write_reference  # noqa: F401 (ref: fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = (("best", "plain"), ("best", "sorted"), ("pairs", "plain"), ("pairs", "sorted"))      # the four file calls
TAGS = ("plain", "md")


def run_level(own, inputs, path, kind, sort, md=False, level=1, fmt="bam", **kw):
    """test_gpu_bam.run with the MD tag and the container's level as handle state"""
    eng = own[0]
    eng.set_bgzf_level(level)
    try:
        if not md:
            return run(own, inputs, path, kind, fmt, "sorted" if sort == "sorted" else "plain", **kw)
        eng.set_output_format(fmt), eng.set_sam_tags(md=True)
        try:
            ix = own[1]
            if kind == "pairs":
                from tests.test_gpu_md import INSERT
                st = eng.map_pairs_file(ix, NAMES, inputs["f1"], inputs["f2"], str(path), E, *INSERT, rescue_errors=8, header=HEADER,
                                        sort=sort == "sorted", **kw)
            else:
                st = eng.map_file(ix, NAMES, inputs["fq"], str(path), E, header=HEADER, sort=sort == "sorted", **kw)
        finally:
            eng.set_output_format("sam"), eng.set_sam_tags(md=False)
        return open(path, "rb").read(), st
    finally:
        eng.set_bgzf_level(0)


@pytest.fixture(scope="module")
def outputs(own, inputs, tmp_path_factory):
    """every call's SAM file and its BAM file at both levels, computed once"""
    d = tmp_path_factory.mktemp("deflate_out")
    out = {}
    for kind, sort in CALLS:
        for tags in TAGS:
            md = tags == "md"
            sam, _ = run_level(own, inputs, d / "x.sam", kind, sort, md, level=1, fmt="sam")       # the level has no effect on SAM
            bam0, st0 = run_level(own, inputs, d / "x0.bam", kind, sort, md, level=0)
            bam1, st1 = run_level(own, inputs, d / "x1.bam", kind, sort, md, level=1)
            out[kind, sort, tags] = dict(sam=sam, bam0=bam0, bam1=bam1, st0=st0, st1=st1)
    return out


# ---- the stand-alone call ---------------------------------------------------------------------------------------------------------------
def test_device_equals_host_on_the_corpus(asm, own):
    eng = own[0]
    for name, src in dc.corpus().items():
        want = asm.bgzf_compress_host(src, level=asm.BGZF_DEFLATE)
        got = eng.bgzf_compress(src)
        assert got == want, name
        assert eng.bgzf_compress(src) == got, name                              # twice in a row
        assert eng.bgzf_compress(src, level=asm.BGZF_STORED) == eng.bgzf_frame(src), name
        dc.check_container(got, src)
    assert eng.bgzf_compress(b"") == bc.EOF_BLOCK and eng.bgzf_compress(b"", eof=False) == b""
    src = dc.corpus()["records %d" % (2 * dc.P + 1)]
    assert eng.bgzf_compress(src, eof=False) + bc.EOF_BLOCK == eng.bgzf_compress(src)


def test_stand_alone_arguments(asm, own):
    import ctypes
    eng = own[0]
    src = dc.corpus()["text 1025"]
    with pytest.raises(asm.AsmError) as exc:
        eng.bgzf_compress(src, level=2)
    assert exc.value.code == -1 and "level must be" in str(exc.value)
    bound = int(eng.lib.asm_bgzf_bound(len(src), 1))
    out, got = ctypes.create_string_buffer(b"\x55" * bound, bound), ctypes.c_size_t(0)
    assert eng.lib.asm_bgzf_compress(eng.h, src, len(src), 1, 1, out, bound - 1, ctypes.byref(got)) == -1
    assert out.raw == b"\x55" * bound and b"dst_cap is below asm_bgzf_bound" in eng.lib.asm_last_error(eng.h)


# ---- the file calls -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tags", TAGS)
@pytest.mark.parametrize("kind,sort", CALLS)
def test_level_1_says_what_sam_says(asm, ref, outputs, kind, sort, tags):
    o = outputs[kind, sort, tags]
    sam, bam0, bam1 = o["sam"], o["bam0"], o["bam1"]
    assert dc.decode(bam1) == sam and bc.decode(bam0) == sam
    assert (b"\tMD:Z:" in sam) == (tags == "md")
    b0, b1 = bc.bgzf_blocks(bam0), bc.bgzf_blocks(bam1)
    assert [b["payload"] for b in b1] == [b["payload"] for b in b0]             # the same stream, cut at the same places
    assert len(b1) >= 5
    for b in b1:
        assert b["bsize"] <= len(b["payload"]) + 31
        assert len(b["payload"]) < dc.P or b["bsize"] < dc.P + 31, "a full block of records is smaller than its stored form"
    # the header's blocks are the host encoder's at level 1, and bytes_out counts what was written behind them
    head = dc.header_bytes(bam1)
    bgzf_compress_host = asm.bgzf_compress_host
    assert bam1[:head] == bgzf_compress_host(header_stream(ref), eof=False, level=1)
    assert o["st1"]["bytes_out"] == len(bam1) - head and o["st0"]["bytes_out"] == len(bam0) - dc.header_bytes(bam0)
    # the record blocks are the stand-alone call's
    records = b"".join(b["payload"] for b in b0)[len(header_stream(ref)):]
    assert bam1[head:] == bgzf_compress_host(records, level=1)
    for field in ("records", "bytes_in", "chunks"):
        assert o["st1"][field] == o["st0"][field], field
    if sort == "sorted":
        assert o["st1"]["sort"] == dict(o["st0"]["sort"], seconds_sort=o["st1"]["sort"]["seconds_sort"])


def test_the_file_does_not_depend_on_chunking(own, inputs, outputs, tmp_path):
    for kind, sort in CALLS:
        want = outputs[kind, sort, "plain"]["bam1"]
        for chunk_bytes in (3000, 70000, 1 << 20):           # no chunk fills a block; a block boundary in most chunks; one chunk
            got, _ = run_level(own, inputs, tmp_path / "c.bam", kind, sort, chunk_bytes=chunk_bytes)
            assert got == want, (kind, sort, chunk_bytes)
    got, _ = run_level(own, inputs, tmp_path / "m.bam", "pairs", "sorted", max_device_bytes=64 << 20)
    assert got == outputs["pairs", "sorted", "plain"]["bam1"]
    again, _ = run_level(own, inputs, tmp_path / "again.bam", "best", "plain")              # two runs give the same file
    assert again == outputs["best", "plain", "plain"]["bam1"]


CHILD = """
import sys
sys.path.insert(0, %r)
import approximate_string_matching_amd as asm
from tests.test_gpu_md import K, NAMES
ref = open(sys.argv[1]).read().split("\\n")[:3]
eng = asm.Engine(0)
ix = eng.build_index(ref, k=K)
eng.set_output_format("bam")
eng.set_bgzf_level("deflate")
st = eng.map_file(ix, NAMES, sys.argv[2], sys.argv[3], %d, header=%r)
print(st["chunks"])
"""


@pytest.mark.parametrize("map_chunk", [16, 333])
def test_the_file_does_not_depend_on_the_device_chunk(ref, inputs, outputs, tmp_path, map_chunk):
    """ASM_MAP_CHUNK is read when a handle is created: a fresh child process"""
    seqs = tmp_path / "ref.txt"
    seqs.write_text("\n".join(ref) + "\n")
    out = tmp_path / "child.bam"
    env = dict(os.environ, ASM_MAP_CHUNK=str(map_chunk))
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, E, HEADER), str(seqs), inputs["fq"], str(out)], capture_output=True, text=True,
                       timeout=LIMIT, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.split()[-1]) == (inputs["n"] + map_chunk - 1) // map_chunk
    assert out.read_bytes() == outputs["best", "plain", "plain"]["bam1"]


def test_empty_input(asm, own, ref, tmp_path):
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    files = dict(fq=str(empty), f1=str(empty), f2=str(empty))
    want = asm.bgzf_compress_host(header_stream(ref), eof=False, level=1) + bc.EOF_BLOCK
    assert want != bc.frame_stored(header_stream(ref))
    for kind, sort in CALLS:
        got, st = run_level(own, files, tmp_path / "e.bam", kind, sort)
        assert got == want and st["bytes_out"] == 28 and st["records"] == 0, (kind, sort)


def test_interface(asm, engine, own):
    eng = own[0]
    assert engine.get_bgzf_level() == asm.BGZF_STORED and eng.get_bgzf_level() == asm.BGZF_STORED
    eng.set_bgzf_level("deflate")
    assert eng.get_bgzf_level() == asm.BGZF_DEFLATE
    for bad in (2, -1):
        with pytest.raises(asm.AsmError) as exc:
            eng.set_bgzf_level(bad)
        assert exc.value.code == -1 and "level must be" in str(exc.value) and eng.get_bgzf_level() == asm.BGZF_DEFLATE
    eng.set_bgzf_level(asm.BGZF_STORED)
    assert eng.get_bgzf_level() == asm.BGZF_STORED and eng.lib.asm_map_get_bgzf_level(None) == asm.BGZF_STORED
    assert eng.lib.asm_map_set_bgzf_level(None, 1) == -1


def test_tool(own, ref, inputs, tmp_path):
    """asm-map --stream --bam --bam-level 1 writes the library's file; --bam-level without --bam is refused with a message"""
    fa = tmp_path / "ref.fa"
    write_reference(fa, ref)
    common = ["-r", str(fa), "-q", inputs["fq"], "-e", str(E), "--both-strands", "--k", str(K)]
    bam = tmp_path / "t.bam"
    r = subprocess.run([EXE] + common + ["--stream", "--bam", "--bam-level", "1", "-o", str(bam)], capture_output=True, text=True, timeout=LIMIT)
    assert r.returncode == 0, r.stderr[-2000:]
    data = bam.read_bytes()
    stream = b"".join(b["payload"] for b in bc.bgzf_blocks(data))
    text = bc.parse_header(stream)[0]
    assert b" --bam-level 1" in text.split(b"@PG")[1]
    got, _ = run_level(own, inputs, tmp_path / "lib.bam", "best", "plain", header=text.decode("latin-1"))
    assert got == data and len(data) < len(stream)
    r = subprocess.run([EXE] + common + ["--stream", "--bam-level", "1", "-o", str(tmp_path / "no.bam")], capture_output=True, text=True,
                       timeout=LIMIT)
    assert r.returncode == 2 and "--bam-level needs --bam" in r.stderr and "usage: asm-map" in r.stderr
    assert not (tmp_path / "no.bam").exists()
