"""asm_map_pairs_file / asm_map_pairs_file_sorted / asm-map --stream-pairs on two BGZF-compressed FASTQ files (docs/design/mapper.md,
"Compressed input for pairs"): the SAM or BAM bytes equal those of the same call on the two inflated texts, whatever the member cuts,
chunk_bytes and ASM_MAP_CHUNK are; the record errors are the plain call's, and corrupt members, mixed kinds, plain gzip and EOF-only
files give what the contract says.  About 2 000 pairs of 36 and 150 bp (a few mates of 6 000 bp, so that chunks without a whole pair
occur) against a 20 kbp reference, e = 2.  The fill policy and the cut's rule by themselves: tests/test_bgzf_pair_fill_host.py."""
import ctypes
import gzip
import os
import random
import struct
import subprocess
import sys

import pytest

from tests import bgzf_in_cases as bi
from tests import bgzf_pair_cases as pc
from tests.test_map_host import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
EXE = os.path.join(PKG, "asm-map")
FILL_CHECK = os.path.join(PKG, "bgzf_pair_fill_host_check")
NAMES, K, E, HEADER, INSERT = ["chr1"], 12, 2, "@HD\tVN:1.6\n", (150, 500)
LEN = (36, 150)


def make_texts(n=2000, seed=5, long_every=400):
    """FR pairs out of fragments of 200 to 400 bp, up to 2 substitutions a mate (every 11th mate 2: 4, for rescue), every 17th pair
    random, every 400th with a mate 2 of 6 000 bp; file 1 CRLF in every fifth record"""
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(20_000))
    out = ([], [])
    for t in range(n):
        frag = rng.randint(200, 400)
        a = rng.randrange(len(ref) - frag)
        f = ref[a:a + frag]
        if t % 2:
            f = revcomp(f)
        m = [f[:LEN[0]], revcomp(f[-LEN[1]:])]
        for x in (0, 1):
            s = list(m[x])
            for _ in range(4 if x == 1 and t % 11 == 0 else rng.randrange(3)):
                s[rng.randrange(len(s))] = rng.choice("ACGT")
            m[x] = "".join(s)
        if t % 17 == 0:
            m = ["".join(rng.choice("ACGT") for _ in range(ln)) for ln in LEN]
        if long_every and t % long_every == long_every - 1:
            m[1] = "".join(rng.choice("ACGT") for _ in range(6000))
        for x in (0, 1):
            end = "\r\n" if x == 0 and t % 5 == 0 else "\n"
            out[x].append("@p%d/%d%s%s%s+%s%s%s" % (t, x + 1, end, m[x], end, end, "".join(chr(rng.randrange(33, 74)) for _ in range(len(m[x]))), end))
    return ref, "".join(out[0]).encode(), "".join(out[1]).encode()


def cut_members(text, sizes):
    out, at, k = [], 0, 0
    while at < len(text):
        part = text[at:at + sizes[k % len(sizes)]]
        out.append(bi.good_member(bi.deflate(part, level=(1, 6, 9)[k % 3]), part))
        at, k = at + len(part), k + 1
    return b"".join(out)


def write(path, body):
    with open(path, "wb") as fh:
        fh.write(body)
    return str(path)


@pytest.fixture(scope="module")
def data(asm, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gzpairs")
    ref, t1, t2 = make_texts()
    cuts = {"text": (t1, t2),
            "bgzip": (cut_members(t1, [65280]) + bi.EOF_BLOCK, cut_members(t2, [65280]) + bi.EOF_BLOCK),
            # file 2 with an empty member in front and no EOF block; file 1 as bgzip writes it
            "rotation": (cut_members(t1, [65280]) + bi.EOF_BLOCK, bi.EOF_BLOCK + cut_members(t2, [1, 7, 4099])),
            "own": tuple(asm.bgzf_compress_host(t, eof=True, level=asm.BGZF_DEFLATE) for t in (t1, t2))}
    paths = {name: tuple(write(tmp / ("%s_%d%s" % (name, x + 1, ".fq" if name == "text" else ".fq.gz")), body[x]) for x in (0, 1))
             for name, body in cuts.items()}
    (tmp / "ref.fa").write_text(">chr1\n" + ref + "\n")
    return dict(ref=ref, texts=(t1, t2), paths=paths, tmp=tmp, fa=str(tmp / "ref.fa"))


@pytest.fixture(scope="module")
def own(asm):
    eng = asm.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def index(own, data):
    return own.build_index([data["ref"]], k=K)


VARIANTS = {
    "sam": dict(), "sorted": dict(sort=True), "bam0": dict(fmt="bam", level=0), "bam1": dict(fmt="bam", level=1), "md": dict(md=True),
    "gap": dict(mapq="gap"), "rescue": dict(rescue_errors=5),
}


def run(own, index, srcs, dst, fmt="sam", level=0, md=False, mapq="reference", **kw):
    own.set_output_format(fmt)
    own.set_bgzf_level(level)
    own.set_sam_tags(md=md)
    own.set_mapq_model(mapq)
    try:
        st = own.map_pairs_file(index, NAMES, srcs[0], srcs[1], str(dst), E, *INSERT, header=HEADER, **kw)
    finally:
        own.set_output_format("sam"), own.set_bgzf_level(0), own.set_sam_tags(md=False), own.set_mapq_model("reference")
    with open(dst, "rb") as fh:
        return fh.read(), st


@pytest.fixture(scope="module")
def plain(own, index, data):
    """the reference of every test below: the plain call on the two texts, once per variant"""
    return {v: run(own, index, data["paths"]["text"], data["tmp"] / ("plain_" + v), **kw) for v, kw in VARIANTS.items()}


SAME = ("pairs", "proper", "rescued", "unsent", "records", "bytes_out")


@pytest.mark.parametrize("cut", ["bgzip", "rotation", "own"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bytes_equal_the_plain_call(own, index, data, plain, cut, variant):
    want, st0 = plain[variant]
    assert len(want) > 400_000 or variant.startswith("bam")
    assert st0["pairs"] == 2000 and st0["proper"] > 1500 and st0["unsent"] == 5
    assert variant != "rescue" or st0["rescued"] > 0
    for chunk in (4096, 0):
        got, st = run(own, index, data["paths"][cut], data["tmp"] / "out", chunk_bytes=chunk, **VARIANTS[variant])
        assert got == want, (cut, variant, chunk)
        assert st["bytes_in"] == len(data["texts"][0]) + len(data["texts"][1]) == st0["bytes_in"]
        assert [st[k] for k in SAME] == [st0[k] for k in SAME]


def test_chunks_without_a_pair_occur(data, tmp_path):
    """at chunk_bytes 4 096 a mate of 6 000 bp spans three chunks: the reader's policy and the cut's rule, run on the host over the
    files of the test above, meet chunks with R = 0 in front of the end"""
    assert os.path.exists(FILL_CHECK), "build() makes host/bgzf_pair_fill_host_check.cpp"
    out = tmp_path / "chunks.bin"
    r = subprocess.run([FILL_CHECK, *data["paths"]["rotation"], "4096", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    tail = struct.unpack("<11Q", out.read_bytes()[-88:])
    assert tail[0] == 2**64 - 1 and tail[1] == 0 and tail[3:5] == (2000, 2000)
    assert tail[9] > 0


CHILD = """
import sys
sys.path.insert(0, %r)
import approximate_string_matching_amd as asm
eng = asm.Engine(0)
ix = eng.build_index([open(sys.argv[1]).read().split("\\n")[1]], k=%d)
eng.map_pairs_file(ix, ["chr1"], sys.argv[2], sys.argv[3], sys.argv[4], %d, %d, %d, header=%r, chunk_bytes=4096)
"""


def test_small_device_chunk_in_a_child(data, plain, tmp_path):
    """ASM_MAP_CHUNK is read when a handle is created: a fresh child process"""
    out = tmp_path / "child.sam"
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, K, E, INSERT[0], INSERT[1], HEADER), data["fa"], *data["paths"]["rotation"], str(out)],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, ASM_MAP_CHUNK="7"), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == plain["sam"][0]


# ---- errors: one test per input; the handle maps afterwards ---------------------------------------------------------------------------
def small(data, n=300):
    return tuple(pc.whole_records(t, n) for t in data["texts"])


def gz(text, sizes=(4099, 1, 7)):
    return cut_members(text, list(sizes)) + bi.EOF_BLOCK


def error_of(asm, own, index, f1, f2, tmp_path, **kw):
    with pytest.raises(asm.AsmError) as err:
        own.map_pairs_file(index, NAMES, f1, f2, str(tmp_path / "o.sam"), E, *INSERT, **kw)
    return err.value.code, str(err.value)


def still_maps(own, index, data, plain):
    got, _ = run(own, index, data["paths"]["own"], data["tmp"] / "after", chunk_bytes=0)
    assert got == plain["sam"][0]


def both_errors(asm, own, index, t1, t2, tmp_path, **kw):
    """the error of the plain call on the two texts and of the call on their compressed forms, cut differently"""
    a = error_of(asm, own, index, write(tmp_path / "a1.fq", t1), write(tmp_path / "a2.fq", t2), tmp_path, **kw)
    b = error_of(asm, own, index, write(tmp_path / "b1.fq.gz", gz(t1)), write(tmp_path / "b2.fq.gz", gz(t2, (7, 1, 4099))), tmp_path, **kw)
    return a, b


def flip_crc(container, k):
    parts = bi.split_members(container)
    body = bytearray(container)
    body[parts[k][0] + len(parts[k][1]) - 8] ^= 1
    return bytes(body), parts[k][0]


def test_corrupt_member_in_file_2(asm, own, index, data, plain, tmp_path):
    t1, t2 = small(data)
    bad, at = flip_crc(gz(t2), 5)
    for chunk in (4096, 0):
        code, msg = error_of(asm, own, index, write(tmp_path / "1.fq.gz", gz(t1)), write(tmp_path / "2.fq.gz", bad), tmp_path, chunk_bytes=chunk)
        assert code == -1 and "file 2: BGZF member 5 at offset %d: CRC-32 mismatch" % at in msg, msg
    still_maps(own, index, data, plain)


def test_corrupt_members_in_both_files_name_file_1(asm, own, index, data, plain, tmp_path):
    t1, t2 = small(data)
    bad1, at1 = flip_crc(gz(t1), 4)
    bad2, _ = flip_crc(gz(t2), 0)
    code, msg = error_of(asm, own, index, write(tmp_path / "1.fq.gz", bad1), write(tmp_path / "2.fq.gz", bad2), tmp_path, chunk_bytes=0)
    assert code == -1 and "file 1: BGZF member 4 at offset %d: CRC-32 mismatch" % at1 in msg, msg
    # a bad header in file 1 behind sound members: its own index and offset
    junk = gz(t1) + b"junk"
    code, msg = error_of(asm, own, index, write(tmp_path / "1.fq.gz", junk), write(tmp_path / "2.fq.gz", gz(t2)), tmp_path, chunk_bytes=4096)
    assert code == -1 and "file 1: BGZF member %d at offset %d: not a BGZF member header" % (len(bi.split_members(gz(t1))), len(gz(t1))) in msg, msg
    still_maps(own, index, data, plain)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_mixed_kinds_are_refused(asm, own, index, data, plain, tmp_path, order):
    t1, t2 = small(data)
    files = [write(tmp_path / "1.fq", t1), write(tmp_path / "2.fq.gz", gz(t2))] if order == (0, 1) else \
        [write(tmp_path / "1.fq.gz", gz(t1)), write(tmp_path / "2.fq", t2)]
    code, msg = error_of(asm, own, index, files[0], files[1], tmp_path)
    zipped = 2 if order == (0, 1) else 1
    assert code == -4 and "file %d (%s) is BGZF and file %d (%s) is plain text" % (zipped, files[zipped - 1], 3 - zipped, files[2 - zipped]) in msg, msg
    still_maps(own, index, data, plain)


@pytest.mark.parametrize("which", [0, 1])
def test_plain_gzip_is_refused(asm, own, index, data, plain, tmp_path, which):
    texts = small(data)
    files = [write(tmp_path / ("%d.fq.gz" % (x + 1)), gzip.compress(texts[x]) if x == which else gz(texts[x])) for x in (0, 1)]
    code, msg = error_of(asm, own, index, files[0], files[1], tmp_path)
    assert code == -4 and files[which] + " is plain gzip" in msg and "recompress it with bgzip" in msg, msg
    still_maps(own, index, data, plain)


def test_name_mismatch_is_the_plain_calls(asm, own, index, data, plain, tmp_path):
    t1, t2 = small(data)
    a, b = both_errors(asm, own, index, t1, t2.replace(b"@p250/2", b"@q250/2"), tmp_path, chunk_bytes=4096)
    assert a == b and a[0] == -1 and "the mates of record 251 have different names" in a[1], (a, b)
    still_maps(own, index, data, plain)


def test_malformed_record_in_file_2_is_the_plain_calls(asm, own, index, data, plain, tmp_path):
    t1, t2 = small(data)
    a, b = both_errors(asm, own, index, t1, t2.replace(b"@p260/2", b"xp260/2"), tmp_path, chunk_bytes=4096)
    assert a == b and a[0] == -1 and "record 261 of file 2 is malformed" in a[1], (a, b)
    still_maps(own, index, data, plain)


def test_truncated_file_1_is_the_plain_calls(asm, own, index, data, plain, tmp_path):
    t1, t2 = small(data)
    for chunk in (4096, 0):
        a, b = both_errors(asm, own, index, t1[:-50], t2, tmp_path, chunk_bytes=chunk)
        assert a == b and a[0] == -1 and "record 300 of file 1 is truncated" in a[1], (a, b)
    still_maps(own, index, data, plain)


def test_file_2_longer_by_one_record(asm, own, index, data, plain, tmp_path):
    t1, t2 = small(data)
    for chunk in (4096, 0):
        a, b = both_errors(asm, own, index, pc.whole_records(t1, 299), t2, tmp_path, chunk_bytes=chunk)
        assert a == b and a[0] == -1 and "record 300 of file 2 has no mate" in a[1], (a, b)
    still_maps(own, index, data, plain)


def test_file_1_longer_by_500_records_stops_at_once(asm, own, index, data, plain, tmp_path):
    """file 1 here holds the mates of 150 bp (the names' /1 and /2 do not matter to the pairing), so its surplus is 500 records of more
    than 300 bytes; the call must report the missing mate when file 2 has run dry, not inflate and hold the surplus first: carry_peak,
    which a failed call on compressed input leaves in its stats, stays below the surplus"""
    _, t1, t2 = make_texts(1000, seed=8, long_every=0)
    long_file, short_file = t2, pc.whole_records(t1, 500)
    surplus = len(long_file) - len(pc.whole_records(long_file, 500))
    a, b = both_errors(asm, own, index, long_file, short_file, tmp_path, chunk_bytes=4096)
    assert a == b and a[0] == -1 and "record 501 of file 1 has no mate" in a[1], (a, b)
    st = asm.MapPairsFileStats()
    p, pp = asm.MapParams(E, 1, 0, 3), asm.PairParams(INSERT[0], INSERT[1], -1)
    arr = (ctypes.c_char_p * 1)(b"chr1")
    rc = own.lib.asm_map_pairs_file(own.h, index.ptr, arr, os.fsencode(str(tmp_path / "b1.fq.gz")), os.fsencode(str(tmp_path / "b2.fq.gz")),
                                    os.fsencode(str(tmp_path / "o.sam")), None, ctypes.byref(p), ctypes.byref(pp), 4096, ctypes.byref(st))
    assert rc == -1 and st.pairs == 0
    print("carry_peak %d, surplus %d" % (st.carry_peak, surplus))
    assert 0 < st.carry_peak < surplus      # holding the surplus would have made it the carry
    still_maps(own, index, data, plain)


def test_two_eof_only_files_give_the_header(own, index, data, tmp_path):
    for a, b in ((bi.EOF_BLOCK, bi.EOF_BLOCK), (bi.EOF_BLOCK, bi.EOF_BLOCK * 2)):
        got, st = run(own, index, (write(tmp_path / "1.fq.gz", a), write(tmp_path / "2.fq.gz", b)), tmp_path / "o.sam")
        assert got == HEADER.encode() and st["pairs"] == 0 and st["bytes_in"] == 0


def test_tool_takes_gz_mates(data, tmp_path):
    outs = []
    for srcs in (data["paths"]["text"], data["paths"]["rotation"]):
        out = tmp_path / "tool.sam"
        r = subprocess.run([EXE, "-r", data["fa"], "-1", srcs[0], "-2", srcs[1], "-o", str(out), "-e", str(E), "--insert", "%d,%d" % INSERT,
                            "--stream-pairs", "--chunk-bytes", "4096"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([ln for ln in out.read_bytes().split(b"\n") if not ln.startswith(b"@PG")])      # @PG names the command line
    assert outs[0] == outs[1] and len(outs[0]) > 4000
