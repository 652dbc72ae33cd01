"""The deflate encoder on the device at its edges (docs/design/mapper.md, "Deflate"): asm_bgzf_compress on the adversarial corpus of
tests/deflate_cases.py against the host build of the same encoder, twice in a row, with the contract read back from the device's
bytes token by token (deflate_cases.check_tokens) and every entry's own property asserted on them.  Then a container of 300 blocks
of eight kinds, more blocks than the device has CUs and of very different sizes and types, and a small call behind it through the
same scratch.

What of this only the device can get wrong: the prefix sum of the tokens' bits over the window's 16 waves (`before`) moves every
token of the later waves, so a wrong one breaks the bytes of every entry here that has a window of more than 64 tokens, the "f length"
text fills first of all; a wrong `off[b]` of the compaction shows where blocks of different sizes follow each other, which is the
mixed container: its blocks range from under 100 to 65 311 bytes in a seeded order."""
import ctypes
import os
import struct
import subprocess
import sys

import pytest

from tests import bam_cases as bc
from tests import deflate_cases as dc
from tests.test_gpu_bam import E, HEADER, LIMIT, header_stream, inputs, own  # noqa: F401 (inputs, own: fixtures)
from tests.test_gpu_deflate import CHILD, ROOT, run_level
from tests.test_gpu_map_file import write_fastq
from tests.test_gpu_md import ref  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("letter", "abcdefg")
def test_device_equals_host_at_the_edges(asm, own, letter):
    eng = own[0]
    names = [n for n in dc.adversarial() if n[0] == letter]
    assert names
    for name in names:
        src, prop = dc.adversarial()[name]
        want = asm.bgzf_compress_host(src, level=asm.BGZF_DEFLATE)
        got = eng.bgzf_compress(src)
        assert got == want, name
        assert eng.bgzf_compress(src) == got, name                              # twice in a row
        blocks = dc.check_container(got, src)
        prop([dc.check_tokens(b, b["payload"]) for b in blocks])


def test_the_old_corpus_keeps_the_contract(own):
    eng = own[0]
    for name, src in dc.corpus().items():
        for b in dc.check_container(eng.bgzf_compress(src), src):
            dc.check_tokens(b, b["payload"])


def test_mixed_container_and_a_small_call_behind_it(asm, own):
    eng = own[0]
    kinds, order = dc.mixed_blocks()
    assert len(order) == 300 and set(order) == set(range(8))
    host = [asm.bgzf_compress_host(k, eof=False, level=1) for k in kinds]           # the host encoder runs on eight blocks, not on 300
    types = [dc.btype(bc.bgzf_blocks(h)[0]) for h in host]
    assert set(types) == {0, 1, 2}
    print("mixed container: block bytes", [len(h) for h in host], "types", types)
    src = b"".join(kinds[k] for k in order)
    want = b"".join(host[k] for k in order)
    got = eng.bgzf_compress(src)
    assert got == want + bc.EOF_BLOCK
    assert eng.bgzf_compress(src, eof=False) == want
    for k, h in zip(kinds, host):
        b, = bc.bgzf_blocks(h)
        dc.check_tokens(b, k)
    # a 3-block payload through the same engine: the scratch of the larger call is reused, and nothing behind dst_len is touched
    small = kinds[3][:1000] + kinds[0] + kinds[2][:dc.P + 5]
    small_want = asm.bgzf_compress_host(small, level=1)
    cap = int(eng.lib.asm_bgzf_bound(len(small), 1))
    out, n = ctypes.create_string_buffer(b"\x55" * cap, cap), ctypes.c_size_t(0)
    assert eng.lib.asm_bgzf_compress(eng.h, small, len(small), 1, 1, out, cap, ctypes.byref(n)) == 0
    assert out.raw[:n.value] == small_want and n.value < cap and out.raw[n.value:] == b"\x55" * (cap - n.value)
    assert len(bc.bgzf_blocks(small_want)) == 4


# ---- the file path: a device chunk that ends next to a block boundary ----------------------------------------------------------------
def record_sizes(bam, ref):
    """the bytes of every record of a level-0 file's record stream, and the stream"""
    stream = b"".join(b["payload"] for b in bc.bgzf_blocks(bam))[len(header_stream(ref)):]
    sizes, at = [], 0
    while at < len(stream):
        sizes.append(4 + struct.unpack_from("<i", stream, at)[0])
        at += sizes[-1]
    assert at == len(stream)
    return sizes, stream


def test_a_chunk_that_ends_beside_a_block_boundary(asm, own, ref, inputs, tmp_path):
    """map_file at level 1 with a device chunk whose records end two bytes in front of a 65 280-byte block boundary, so that the block
    is completed from the carry buffer by the first two bytes of the next chunk.  The reads are those of tests/test_gpu_bam.py under
    names of their own: a record's size grows by one with every byte of its name, so padding the names of the chunk's reads moves the
    chunk's end to the byte.  The reference is the host encoding of the level-0 file's record stream."""
    lines = open(inputs["fq"]).read().split("\n")
    recs = [(lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]
    assert len(recs) == inputs["n"]
    plain = tmp_path / "plain.fq"
    write_fastq(plain, [("q%05d" % t, q, ql) for t, (q, ql) in enumerate(recs)])
    bam0, st = run_level(own, dict(inputs, fq=str(plain)), tmp_path / "plain.bam", "best", "plain", level=0)
    sizes, _ = record_sizes(bam0, ref)
    assert len(sizes) == len(recs) == st["records"], "one record per read, in the reads' order"
    # the chunk: the fewest reads, from 200 on, whose names can take the padding that puts its end at a boundary less two
    chunk = pad = None
    for c in range(200, len(recs)):
        d = (dc.P - 2 - sum(sizes[:c])) % dc.P
        if d <= 100 * c:
            chunk, pad = c, d
            break
    assert chunk is not None
    padded = tmp_path / "padded.fq"
    write_fastq(padded, [("q%05d" % t + "x" * ((pad // chunk + (1 if t < pad % chunk else 0)) if t < chunk else 0), q, ql)
                         for t, (q, ql) in enumerate(recs)])
    files = dict(inputs, fq=str(padded))
    bam0, st0 = run_level(own, files, tmp_path / "padded0.bam", "best", "plain", level=0)
    sizes, stream = record_sizes(bam0, ref)
    end = sum(sizes[:chunk])
    assert dc.P - end % dc.P == 2, "the chunk ends two bytes in front of a block boundary"
    seqs = tmp_path / "ref.txt"
    seqs.write_text("\n".join(ref) + "\n")
    out = tmp_path / "child.bam"
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, E, HEADER), str(seqs), str(padded), str(out)], capture_output=True, text=True,
                       timeout=LIMIT, env=dict(os.environ, ASM_MAP_CHUNK=str(chunk)), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.split()[-1]) == (len(recs) + chunk - 1) // chunk >= 2
    bam1 = out.read_bytes()
    head = dc.header_bytes(bam1)
    assert bam1[:head] == asm.bgzf_compress_host(header_stream(ref), eof=False, level=1)
    assert bam1[head:] == asm.bgzf_compress_host(stream, level=1)
    for b in bc.bgzf_blocks(bam1[head:])[:-1]:
        dc.check_tokens(b, b["payload"])
    # and the same file from one chunk
    again, _ = run_level(own, files, tmp_path / "padded1.bam", "best", "plain", level=1)
    assert again == bam1
