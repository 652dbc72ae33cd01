"""BAM from the file calls (docs/design/mapper.md, "BAM output"): asm_map_set_output_format / Engine.set_output_format / asm-map
--bam.  The SAM path is the reference: every call runs once as SAM and once as BAM, and the BAM file, decoded by the reader of
tests/bam_cases.py, must be the SAM file byte for byte.  On top of that the BAM header, the container's structure, the sorted order,
the file's independence of every chunking, the QNAME limit and the interface.

The shapes: three sequences of about 2 kbp (tests/test_gpu_md.py's reference: a run of N, a lower-case stretch, a copied stretch that
gives secondaries), k = 8, e = 3; 1,500 single-end reads (1,450 of 100 bp with 0..3 edits on both strands, 40 random ones, and the 46
of test_gpu_md.reads_for: every kernel width up to 511, lower case, N, over-long, empty) and 760 pairs (700 proper ones of 100 bp,
12 with mates on different sequences, and the 48 of test_gpu_md.pair_records: rescued, one mate mapped, junk), so that every record
stream is several BGZF blocks long."""
import os
import random
import subprocess
import sys

import pytest

from tests import bam_cases as bc
from tests.map_cases import mid_edit
from tests.test_gpu_map_file import quals, write_fastq
from tests.test_gpu_md import INSERT, K, NAMES, bases, pair_records, reads_for, records, ref, write_reference  # noqa: F401 (ref: fixture)
from tests.test_map_host import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
E = 3
HEADER = "@HD\tVN:1.6\tSO:unknown\n@CO\ta header the library does not edit\n"
LIMIT = 120
KINDS = ("best", "all", "pairs")
VARIANTS = ("plain", "md", "gap", "sorted")


@pytest.fixture(scope="module")
def inputs(ref, tmp_path_factory):
    """the FASTQ files; a read never carries the reference's '*' or '-' (SAM would keep the byte, BAM has no code for it: that
    difference is the host test's, tests/test_bam_host.py)"""
    clean = lambda recs: [(h, q.replace("*", "A").replace("-", "C"), ql) for h, q, ql in recs]
    d = tmp_path_factory.mktemp("bam_in")
    rng = random.Random(29)
    up = [s.upper() for s in ref]
    reads = []
    for t in range(1450):
        s = up[t % 3]
        a = rng.randrange(1, len(s) - 150)
        q = mid_edit(rng, s[a:a + 150], 100, t % 4, ("ins", "del", "sub")[t % 3])[0] if not set("N*-") & set(s[a:a + 150]) else s[a:a + 100]
        reads.append(revcomp(q) if t % 2 else q)
    reads += [bases(rng, 100) for _ in range(40)] + reads_for(ref, E, seed=103)
    rng3 = random.Random(43)
    # 512 bytes: ASM_MAP_MAX_READ + 1, the first length that is written unmapped; its SEQ packs to 256 bytes, a whole number of the
    # lane sink's 64-byte rounds, so QUAL starts on a round's edge
    reads.append(up[1][200:712] if not set("N*-") & set(up[1][200:712]) else bases(rng3, 512))
    recs = clean(records(reads, seed=3))
    fq = d / "reads.fq"
    write_fastq(fq, recs)
    r1, r2 = [], []
    for t in range(712):
        s = up[1 + t % 2]
        a = rng.randrange(len(s) - 400)
        f = s[a:a + 250 + rng.randrange(150)]
        q1, q2 = mid_edit(rng, f, 100, t % 3, "sub")[0], mid_edit(rng, revcomp(f), 100, (t + 1) % 3, "sub")[0]
        if t >= 700:                               # the mates on different sequences
            o = up[2 - t % 2]
            b = rng.randrange(len(o) - 200)
            q2 = revcomp(o[b:b + 100])
        r1.append(q1), r2.append(q2)
    rng2 = random.Random(31)
    p1, p2 = pair_records(ref, E, seed=23)
    recs1 = clean([("f%d/1" % t, q, quals(rng2, len(q))) for t, q in enumerate(r1)] + p1)
    recs2 = clean([("f%d/2" % t, q, quals(rng2, len(q))) for t, q in enumerate(r2)] + p2)
    long_mate = up[2][600:1112]                  # a mate of 512 bytes: its pair is not sent, both lines are unmapped
    recs1.append(("long512/1", long_mate, quals(rng3, 512)))
    recs2.append(("long512/2", revcomp(up[2][1200:1300]), quals(rng3, 100)))
    f1, f2 = d / "r1.fq", d / "r2.fq"
    write_fastq(f1, recs1), write_fastq(f2, recs2)
    return dict(fq=str(fq), f1=str(f1), f2=str(f2), n=len(recs), pairs=len(recs1))


@pytest.fixture(scope="module")
def own(asm, ref):
    """an engine of its own (the session's engine never touches the setter) and its index"""
    eng = asm.Engine(0)
    assert eng.output_format == asm.OUT_SAM
    ix = eng.build_index(ref, k=K)
    yield eng, ix
    ix.free()
    eng.close()


def run(own, inputs, path, kind, fmt, variant="plain", header=HEADER, **kw):
    """one file call under the format and the variant's handle state -> (the file's bytes, the stats)"""
    eng, ix = own
    eng.set_output_format(fmt)
    eng.set_sam_tags(md=variant == "md")
    eng.set_mapq_model("gap" if variant == "gap" else "reference")
    try:
        if kind == "pairs":
            st = eng.map_pairs_file(ix, NAMES, inputs["f1"], inputs["f2"], str(path), E, *INSERT, rescue_errors=8, header=header,
                                    sort=variant == "sorted", **kw)
        else:
            st = eng.map_file(ix, NAMES, inputs["fq"], str(path), E, max_hits=4 if kind == "all" else 0, strata=1, header=header,
                              sort=variant == "sorted", **kw)
    finally:
        eng.set_output_format("sam"), eng.set_sam_tags(md=False), eng.set_mapq_model("reference")
    return open(path, "rb").read(), st


@pytest.fixture(scope="module")
def outputs(own, inputs, tmp_path_factory):
    """every mode's SAM and BAM file, computed once"""
    d = tmp_path_factory.mktemp("bam_out")
    out = {}
    for kind in KINDS:
        for variant in VARIANTS:
            sam, st_sam = run(own, inputs, d / "x.sam", kind, "sam", variant)
            bam, st_bam = run(own, inputs, d / "x.bam", kind, "bam", variant)
            out[kind, variant] = dict(sam=sam, bam=bam, st_sam=st_sam, st_bam=st_bam)
    return out


def header_stream(ref):
    return bc.encode_header(HEADER.encode(), [(nm, len(s)) for nm, s in zip(NAMES, ref)])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_bam_says_what_sam_says(ref, inputs, outputs, kind, variant):
    o = outputs[kind, variant]
    sam, bam = o["sam"], o["bam"]
    assert sam.startswith(HEADER.encode()) and bam[:4] == b"\x1f\x8b\x08\x04"
    text, refs, recs, blocks = bc.parse_bam(bam)                       # the container's structure, every CRC, every bin
    names = [n for n, _ in refs]
    assert text == HEADER.encode() and refs == [(nm, len(s)) for nm, s in zip(NAMES, ref)]
    decoded = text + "".join(bc.sam_line(r, names) for r in recs).encode("latin-1")
    assert decoded == sam
    # the header has blocks of its own; the record stream starts a fresh block and is cut every PAYLOAD bytes
    head = bc.frame_stored(header_stream(ref), eof=False)
    assert bam.startswith(head) and bam.endswith(bc.EOF_BLOCK)
    body = bc.bgzf_blocks(bam[len(head):])
    record_bytes = sum(len(b["payload"]) for b in body)
    assert len(bc.check_stored(body)) == (record_bytes + bc.PAYLOAD - 1) // bc.PAYLOAD >= 3
    # the stats keep their meaning
    st_sam, st_bam = o["st_sam"], o["st_bam"]
    assert st_bam["bytes_out"] == len(bam) - len(head) and st_sam["bytes_out"] == len(sam) - len(HEADER)
    for field in ("records", "bytes_in", "chunks") + (("pairs", "proper", "rescued", "unsent") if kind == "pairs" else ("reads", "mapped", "too_long")):
        assert st_bam[field] == st_sam[field], field
    lines = sam[len(HEADER):].decode("latin-1").split("\n")[:-1]
    assert st_bam["records"] == len(recs) == len(lines) and (kind == "all" or len(lines) == (2 * inputs["pairs"] if kind == "pairs" else inputs["n"]))
    # the read of 512 bytes: unmapped, SEQ and QUAL whole, in both files
    long_lines = [ln for ln in lines if len(ln.split("\t")[9]) == 512]
    long_recs = [r for r in recs if len(r["seq"]) == 512]
    assert len(long_lines) == len(long_recs) == 1 and int(long_lines[0].split("\t")[1]) & 4 and long_recs[0]["flag"] & 4
    assert long_recs[0]["ref_id"] == -1 and len(long_recs[0]["qual"]) == 512 and long_recs[0]["seq"] == long_lines[0].split("\t")[9]
    assert bytes(q + 33 for q in long_recs[0]["qual"]).decode("latin-1") == long_lines[0].split("\t")[10]
    flags = [int(ln.split("\t")[1]) for ln in lines]
    assert any(f & 16 for f in flags) and any(f & 4 for f in flags) and any("I" in ln.split("\t")[5] for ln in lines)
    if kind == "all":
        assert sum(1 for f in flags if f & 256) >= 3 and all(r["seq"] == "" for r in recs if r["flag"] & 256)
    if kind == "pairs":
        assert sum(1 for ln in lines if "\tXR:i:1" in ln) >= 3
        assert sum(1 for ln, f in zip(lines, flags) if f & 4 and ln.split("\t")[2] != "*") >= 3          # a borrowed RNAME
        assert sum(1 for ln in lines if ln.split("\t")[6] in NAMES) >= 4                                 # mates on two sequences
    else:
        assert any(len(ln.split("\t")[9]) == 511 for ln in lines) and any(ln.split("\t")[9] == "*" and not int(ln.split("\t")[1]) & 256 for ln in lines)
    if variant == "md":
        assert sum(1 for r in recs if any(t[:2] == ("MD", "Z") for t in r["tags"])) == sum(1 for ln in lines if "\tMD:Z:" in ln) > 100
    if variant == "sorted":
        keys = [(len(NAMES) if r["ref_id"] < 0 else r["ref_id"], r["pos"]) for r in recs]
        assert keys == sorted(keys) and keys[-1][0] == len(NAMES) and keys[0][0] == 0
        assert st_bam["sort"]["bytes_held"] == record_bytes and st_bam["sort"]["lines"] == len(recs)
        assert st_sam["sort"]["bytes_held"] == len(sam) - len(HEADER)
        assert bam != outputs[kind, "plain"]["bam"]


def test_the_file_does_not_depend_on_chunking(own, inputs, outputs, tmp_path):
    want = outputs["best", "plain"]["bam"]
    got, st = run(own, inputs, tmp_path / "small.bam", "best", "bam", chunk_bytes=2000)      # no chunk fills a block
    assert got == want and st["chunks"] > 100
    got, st = run(own, inputs, tmp_path / "mid.bam", "best", "bam", chunk_bytes=70000)       # a block boundary in most chunks
    assert got == want and st["chunks"] > 3
    got, _ = run(own, inputs, tmp_path / "pairs.bam", "pairs", "bam", chunk_bytes=3000)
    assert got == outputs["pairs", "plain"]["bam"]
    # sorted: slabs smaller than a block, slabs with a boundary, and a max_device_bytes that still fits
    for kind in ("all", "pairs"):
        want = outputs[kind, "sorted"]["bam"]
        for kw in (dict(chunk_bytes=5000), dict(chunk_bytes=100000), dict(max_device_bytes=64 << 20)):
            got, st = run(own, inputs, tmp_path / "sorted.bam", kind, "bam", "sorted", **kw)
            assert got == want, (kind, kw)
        assert st["sort"]["slabs"] >= 1


CHILD = """
import sys
sys.path.insert(0, %r)
import approximate_string_matching_amd as asm
from tests.test_gpu_md import K, NAMES
ref = open(sys.argv[1]).read().split("\\n")[:3]
eng = asm.Engine(0)
ix = eng.build_index(ref, k=K)
eng.set_output_format("bam")
st = eng.map_file(ix, NAMES, sys.argv[2], sys.argv[3], %d, max_hits=4, strata=1, header=%r)
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
    assert out.read_bytes() == outputs["all", "plain"]["bam"]


def test_empty_input(own, ref, tmp_path):
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    files = dict(fq=str(empty), f1=str(empty), f2=str(empty))
    want = bc.frame_stored(header_stream(ref), eof=False) + bc.EOF_BLOCK
    for kind in ("best", "pairs"):
        for variant in ("plain", "sorted"):
            got, st = run(own, files, tmp_path / "e.bam", kind, "bam", variant)
            assert got == want and st["bytes_out"] == 28 and st["records"] == 0
    # no header text at all
    got, _ = run(own, files, tmp_path / "e.bam", "best", "bam", header=None)
    assert got == bc.frame_stored(bc.encode_header(b"", [(nm, len(s)) for nm, s in zip(NAMES, ref)]), eof=False) + bc.EOF_BLOCK


def test_qname_limit(asm, own, ref, tmp_path):
    rng = random.Random(41)
    read = ref[1].upper()[300:400]
    mk = lambda names: [(nm, read, quals(rng, 100)) for nm in names]
    ok, long_ = tmp_path / "ok.fq", tmp_path / "long.fq"
    write_fastq(ok, mk(["a", "n" * 254, "b"]))
    write_fastq(long_, mk(["a", "b", "n" * 254, "m" * 255, "c", "x" * 300]))
    got, _ = run(own, dict(fq=str(ok)), tmp_path / "ok.bam", "best", "bam")
    sam, _ = run(own, dict(fq=str(ok)), tmp_path / "ok.sam", "best", "sam")
    assert bc.decode(got) == sam and ("n" * 254 + "\t").encode() in sam
    for variant in ("plain", "sorted"):
        with pytest.raises(asm.AsmError) as exc:
            run(own, dict(fq=str(long_)), tmp_path / "long.bam", "best", "bam", variant)
        assert exc.value.code == -1 and "record 4 has a QNAME of more than 254 bytes" in str(exc.value)
        sam, st = run(own, dict(fq=str(long_)), tmp_path / "long.sam", "best", "sam", variant)      # SAM: nothing changes
        assert st["records"] == 6 and ("m" * 255 + "\t").encode() in sam
    # among the errors of one chunk: behind a malformed record, before a name mismatch; pairs name the file, and /1 /2 do not count
    p1, p2, bad = tmp_path / "p1.fq", tmp_path / "p2.fq", tmp_path / "bad.fq"
    write_fastq(p1, mk(["q" * 254 + "/1", "b", "d"]))
    write_fastq(p2, mk(["q" * 254 + "/2", "m" * 255, "other"]))
    with pytest.raises(asm.AsmError) as exc:
        run(own, dict(f1=str(p1), f2=str(p2)), tmp_path / "p.bam", "pairs", "bam")
    assert "record 2 of file 2 has a QNAME of more than 254 bytes" in str(exc.value)
    with pytest.raises(asm.AsmError) as exc:
        run(own, dict(f1=str(p1), f2=str(p2)), tmp_path / "p.sam", "pairs", "sam")
    assert "the mates of record 2 have different names" in str(exc.value)
    bad.write_bytes(open(long_, "rb").read() + b"no at sign\nACGT\n+\nIIII\n")
    with pytest.raises(asm.AsmError) as exc:
        run(own, dict(fq=str(bad)), tmp_path / "bad.bam", "best", "bam")
    assert "record 7 is malformed" in str(exc.value)


def test_interface(asm, engine, own, ref, inputs, outputs, tmp_path):
    eng, ix = own
    assert engine.output_format == asm.OUT_SAM          # the session's engine was never touched
    for bad in (2, -1):
        eng.set_output_format("bam")
        with pytest.raises(asm.AsmError) as exc:
            eng.set_output_format(bad)
        assert exc.value.code == -1 and "format must be" in str(exc.value) and eng.output_format == asm.OUT_BAM
        eng.set_output_format(asm.OUT_SAM)
        with pytest.raises(asm.AsmError):
            eng.set_output_format(bad)
        assert eng.output_format == asm.OUT_SAM
    # back on "sam" (every SAM run of `outputs` came after a BAM run on the same handle): the bytes of a handle that never set it
    sam = tmp_path / "never.sam"
    engine_ix = engine.build_index(ref, k=K)
    try:
        engine.map_file(engine_ix, NAMES, inputs["fq"], str(sam), E, header=HEADER)
    finally:
        engine_ix.free()
    assert sam.read_bytes() == outputs["best", "plain"]["sam"]
    again, _ = run(own, inputs, tmp_path / "again.sam", "best", "sam")
    assert again == sam.read_bytes()


def tool(args, **kw):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=LIMIT, **kw)


def test_tool(own, ref, inputs, tmp_path):
    """asm-map --stream --bam writes the library's bytes (the tool only sets the handle's format, so the modes are the library
    tests'); --bam without a streamed mode is a usage error that says so"""
    fa = tmp_path / "ref.fa"
    write_reference(fa, ref)
    common = ["-r", str(fa), "-q", inputs["fq"], "-e", str(E), "--both-strands", "--k", str(K)]
    bam = tmp_path / "t.bam"
    r = tool(common + ["--stream", "--bam", "-o", str(bam)])
    assert r.returncode == 0, r.stderr[-2000:]
    text, refs, recs, _ = bc.parse_bam(bam.read_bytes())
    assert refs == [(nm, len(s)) for nm, s in zip(NAMES, ref)] and len(recs) == inputs["n"]
    assert text.startswith(b"@HD") and b"@SQ\tSN:chrA" in text and b" --bam" in text.split(b"@PG")[1]
    got, _ = run(own, inputs, tmp_path / "lib.bam", "best", "bam", header=text.decode("latin-1"))
    assert got == bam.read_bytes()
    r = tool(common + ["--bam", "-o", str(tmp_path / "no.bam")])
    assert r.returncode == 2 and "--bam needs --stream or --stream-pairs" in r.stderr and "usage: asm-map" in r.stderr
    assert not (tmp_path / "no.bam").exists()
