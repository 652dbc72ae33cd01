"""asm_map_file / Engine.map_file / asm-map --stream (docs/design/mapper.md, "Files: FASTQ in, SAM out"): a FASTQ file parsed, mapped
and formatted on the device must give, byte for byte, the SAM lines formatted here in Python from Engine.map_reads /
Engine.map_reads_all, and the lines the non-streamed asm-map writes, whatever the chunking."""
import os
import random
import signal
import subprocess

import pytest

from tests.test_gpu_map import make_reads, make_reference
from tests.test_map_host import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
NAMES = ["chrA", "chrB", "chrC"]
LIMIT = 300  # seconds per test


@pytest.fixture(autouse=True)
def time_limit():
    def over(signum, frame):
        raise TimeoutError("test ran longer than %d s" % LIMIT)

    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(LIMIT)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def ref():
    return make_reference()


@pytest.fixture(scope="module")
def index(engine, ref):
    return engine.build_index(ref, k=12)


def quals(rng, m):
    return "".join(chr(rng.randrange(33, 74)) for _ in range(m))


def write_fastq(path, recs, eol="\n", final_newline=True):
    """recs: (header line without '@', seq, qual)"""
    text = "".join("@%s%s%s%s+%s%s%s" % (h, eol, s, eol, eol, q, eol) for h, s, q in recs)
    if not final_newline and text.endswith(eol):
        text = text[:-len(eol)]
    with open(path, "wb") as fh:
        fh.write(text.encode("latin-1"))


def records_for(reads, seed=1):
    rng = random.Random(seed)
    return [("r%d" % t, q, quals(rng, len(q))) for t, q in enumerate(reads)]


def first_word(h):
    h = h.lstrip(" \t")
    for i, c in enumerate(h):
        if c in " \t":
            return h[:i]
    return h


def unmapped_line(name, seq, qual):
    return "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s" % (name, seq.upper() or "*", qual or "*")


def cigar_text(cigar, nops):
    return "*" if nops > 64 else cigar


def expected_lines(engine, index, recs, e, both=True, max_hits=0, strata=None):
    """the SAM lines of the records, formatted from Engine.map_reads / map_reads_all"""
    sent = [t for t, (h, s, q) in enumerate(recs) if 1 <= len(s) <= 511]
    reads = [recs[t][1] for t in sent]
    lines = []
    if max_hits == 0:
        out = engine.map_reads(index, reads, e, both_strands=both) if reads else None
        slot = {t: i for i, t in enumerate(sent)}
        for t, (h, s, q) in enumerate(recs):
            name = first_word(h)
            i = slot.get(t)
            if i is None or not out["mapped"][i]:
                lines.append(unmapped_line(name, s, q))
                continue
            st = int(out["strand"][i])
            seq = revcomp(s.upper()) if st else s.upper()
            qual = (q[::-1] if st else q) or "*"
            lines.append("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tXG:i:%d" % (
                name, 16 * st, NAMES[int(out["seq_id"][i])], int(out["pos"][i]) + 1, int(out["mapq"][i]),
                cigar_text(out["cigar"][i], int(out["cigar_nops"][i])), seq, qual, int(out["dist"][i]), int(out["greedy_cost"][i])))
        return lines
    out = engine.map_reads_all(index, reads, e, max_hits=max_hits, strata=strata, both_strands=both) if reads else None
    slot = {t: i for i, t in enumerate(sent)}
    first = {}
    if out is not None:
        for x, rd in enumerate(out["read"]):
            first.setdefault(int(rd), x)
    for t, (h, s, q) in enumerate(recs):
        name = first_word(h)
        i = slot.get(t)
        if i is None or int(out["n_reported"][i]) == 0:
            lines.append(unmapped_line(name, s, q))
            continue
        nrep, nh = int(out["n_reported"][i]), int(out["n_hits"][i])
        for rank in range(nrep):
            x = first[i] + rank
            assert int(out["read"][x]) == i and int(out["rank"][x]) == rank
            st = int(out["strand"][x])
            seq = "*" if rank else (revcomp(s.upper()) if st else s.upper())
            qual = "*" if rank else ((q[::-1] if st else q) or "*")
            cig = out["cigar"][x]
            import re

            nops = len(re.findall(r"[MID]", cig))
            lines.append("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tXG:i:%d\tNH:i:%d\tHI:i:%d\tXH:i:%d" % (
                name, 16 * st + (256 if rank else 0), NAMES[int(out["seq_id"][x])], int(out["pos"][x]) + 1, int(out["mapq"][x]),
                cigar_text(cig, nops), seq, qual, int(out["dist"][x]), int(out["greedy_cost"][x]), nrep, rank + 1, nh))
    return lines


def sam_lines(path):
    data = open(path, "rb").read().decode("latin-1")
    assert data == "" or data.endswith("\n")
    return data.split("\n")[:-1]


def compare(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.split("\t") == w.split("\t"), (t, g, w)
        assert g == w


def check_stats(st, lines, recs):
    body = [ln for ln in lines if not ln.startswith("@")]
    assert st["reads"] == len(recs)
    assert st["records"] == len(body)
    assert st["mapped"] == sum(1 for ln in body if not (int(ln.split("\t")[1]) & (4 | 256)))
    assert st["too_long"] == sum(1 for h, s, q in recs if len(s) > 511)
    assert st["bytes_out"] == sum(len(ln) + 1 for ln in body)


@pytest.mark.parametrize("both", [True, False])
def test_best_hit_lines_equal_the_library(engine, ref, index, tmp_path, both):
    recs = records_for(make_reads(ref, 2, 320, seed=41), seed=2)
    fq, sam = tmp_path / "r.fq", tmp_path / "o.sam"
    write_fastq(fq, recs)
    st = engine.map_file(index, NAMES, str(fq), str(sam), 2, both_strands=both, header="@HD\tVN:1.6\n")
    got = sam_lines(sam)
    assert got[0] == "@HD\tVN:1.6"
    compare(got[1:], expected_lines(engine, index, recs, 2, both=both))
    check_stats(st, got, recs)
    # 9 reads in 10 come from the reference, half of them reverse-complemented
    assert st["mapped"] > (200 if both else 100) and st["chunks"] >= 1 and st["bytes_in"] == os.path.getsize(fq)


@pytest.mark.parametrize("max_hits", [1, 4])
@pytest.mark.parametrize("strata", [0, 2])
def test_all_hits_lines_equal_the_library(engine, ref, index, tmp_path, max_hits, strata):
    recs = records_for(make_reads(ref, 2, 320, seed=43), seed=3)
    fq, sam = tmp_path / "r.fq", tmp_path / "o.sam"
    write_fastq(fq, recs)
    st = engine.map_file(index, NAMES, str(fq), str(sam), 2, max_hits=max_hits, strata=strata)
    got = sam_lines(sam)
    want = expected_lines(engine, index, recs, 2, max_hits=max_hits, strata=strata)
    compare(got, want)
    check_stats(st, got, recs)
    if max_hits > 1:
        assert any(int(ln.split("\t")[1]) & 256 for ln in got)  # the duplicated segment gives secondary records


def write_reference(path, seqs):
    with open(path, "w") as fh:
        for nm, s in zip(NAMES, seqs):
            fh.write(">%s some description\n" % nm)
            for a in range(0, len(s), 70):
                fh.write(s[a:a + 70] + "\n")


@pytest.mark.parametrize("flags", [["-e", "2", "--both-strands"], ["-e", "2"], ["-e", "2", "--both-strands", "--all-hits", "4", "--strata", "1"]])
def test_streamed_tool_writes_the_tools_bytes(asm, engine, ref, tmp_path, flags):
    assert os.path.exists(EXE), "asm-map is built by build()"
    recs = records_for(make_reads(ref, 2, 300, seed=47), seed=4)
    recs.append(("long", "ACGT" * 150, "I" * 600))
    fa, fq = tmp_path / "ref.fa", tmp_path / "r.fq"
    write_reference(fa, ref)
    write_fastq(fq, recs)
    outs = []
    for extra in ([], ["--stream"]):
        sam = tmp_path / ("o%d.sam" % len(outs))
        r = subprocess.run([EXE, "-r", str(fa), "-q", str(fq), "-o", str(sam)] + flags + extra, capture_output=True, text=True, timeout=LIMIT)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append((sam_lines(sam), r.stderr))
    (plain, err0), (streamed, err1) = outs
    assert len(plain) == len(streamed) > len(recs)
    for a, b in zip(plain, streamed):
        if a.startswith("@PG"):
            assert b.startswith("@PG") and a.split("\tCL:")[0] == b.split("\tCL:")[0] and b.endswith(" --stream")
        else:
            assert a == b
    assert err0.splitlines()[0] == err1.splitlines()[0]  # the summary line


def test_streamed_tool_usage(ref, tmp_path):
    fa, fq, fasta = tmp_path / "ref.fa", tmp_path / "r.fq", tmp_path / "r.fa"
    write_reference(fa, ref)
    write_fastq(fq, records_for(make_reads(ref, 1, 8, seed=1)))
    fasta.write_text(">r0\nACGTACGTACGTACGTACGTACGTACGT\n")
    r = subprocess.run([EXE, "-r", str(fa), "-1", str(fq), "-2", str(fq), "-e", "1", "--insert", "100,500", "--stream"],
                       capture_output=True, text=True, timeout=LIMIT)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([EXE, "-r", str(fa), "-q", str(fasta), "-o", str(tmp_path / "x.sam"), "--stream"], capture_output=True, text=True,
                       timeout=LIMIT)
    assert r.returncode == 1 and r.stderr.strip() == "asm-map: --stream needs FASTQ reads"


def test_chunking_does_not_change_the_output(asm, engine, ref, index, tmp_path, monkeypatch):
    recs = records_for(make_reads(ref, 2, 260, seed=53), seed=5)
    fq = tmp_path / "r.fq"
    write_fastq(fq, recs)
    one_record = len("@%s\n%s\n+\n%s\n" % recs[0])
    for max_hits in (0, 4):
        base = tmp_path / "base.sam"
        st0 = engine.map_file(index, NAMES, str(fq), str(base), 2, max_hits=max_hits)
        want = open(base, "rb").read()
        assert want == ("\n".join(expected_lines(engine, index, recs, 2, max_hits=max_hits, strata=2 if max_hits else None)) + "\n").encode()
        for chunk_bytes in (one_record, 1000, 7777):
            sam = tmp_path / ("c%d.sam" % chunk_bytes)
            st = engine.map_file(index, NAMES, str(fq), str(sam), 2, max_hits=max_hits, chunk_bytes=chunk_bytes)
            assert open(sam, "rb").read() == want, chunk_bytes
            assert st["chunks"] > st0["chunks"] and st["records"] == st0["records"] and st["mapped"] == st0["mapped"]
        # several device chunks per file chunk: a fresh engine reads ASM_MAP_CHUNK
        monkeypatch.setenv("ASM_MAP_CHUNK", "37")
        eng2 = asm.Engine(0)
        try:
            ix2 = eng2.build_index(ref, k=12)
            sam = tmp_path / "small.sam"
            st = eng2.map_file(ix2, NAMES, str(fq), str(sam), 2, max_hits=max_hits)
            assert open(sam, "rb").read() == want
            assert st["chunks"] == (len(recs) + 36) // 37
            ix2.free()
        finally:
            eng2.close()
            monkeypatch.delenv("ASM_MAP_CHUNK")


@pytest.mark.parametrize("at", [0, 6])
def test_record_longer_than_the_pinned_slot(engine, ref, index, tmp_path, at):
    """chunk_bytes=1000 gives pinned slots of 1000 + 1000 / 4 + 4096 = 5,346 bytes; a record whose sequence and quality are 6,000
    bytes each does not fit one, so the reader has the slot replaced by a larger one: as the file's first record, and in the middle
    of it behind a carry.  The bytes are those of the library's calls and those of the default chunk, which holds the whole file."""
    rng = random.Random(73)
    recs = records_for(make_reads(ref, 2, 12, seed=79), seed=7)
    recs.insert(at, ("long", "".join(rng.choice("ACGT") for _ in range(6000)), quals(rng, 6000)))
    fq = tmp_path / "r.fq"
    write_fastq(fq, recs)
    want = expected_lines(engine, index, recs, 2)
    out = {}
    for chunk_bytes in (0, 1000):
        sam = tmp_path / ("c%d.sam" % chunk_bytes)
        st = engine.map_file(index, NAMES, str(fq), str(sam), 2, chunk_bytes=chunk_bytes)
        got = sam_lines(sam)
        compare(got, want)
        check_stats(st, got, recs)
        assert st["too_long"] == 1 and st["bytes_in"] == os.path.getsize(fq)
        out[chunk_bytes] = (open(sam, "rb").read(), st["chunks"])
    assert out[1000][0] == out[0][0]
    assert out[0][1] == 1 and out[1000][1] > 1


def test_format_corners(engine, ref, index, tmp_path):
    rng = random.Random(61)
    good = make_reads(ref, 2, 40, seed=59)
    recs = [("c%d  description here\tand more" % t, q, quals(rng, len(q))) for t, q in enumerate(good)]
    src = ref[1][20_000:20_700].upper()
    recs.append(("len511", src[:511], quals(rng, 511)))
    recs.append(("len512", src[:512], quals(rng, 512)))
    recs.append(("len600", src[:600].lower(), quals(rng, 600)))
    recs.append(("empty", "", ""))
    recs.append(("atqual", src[100:200], "@" + quals(rng, 98) + "+"))
    recs.append(("plusqual", src[200:300], "+" + quals(rng, 99)))
    recs.append(("lower", src[300:400].lower(), quals(rng, 100)))
    recs.append(("withN", src[400:450] + "N" + src[451:500], quals(rng, 100)))
    recs.append(("starqual", src[500:600], "*"))
    recs.append((" \tblankfirst tail", src[50:150], quals(rng, 100)))
    # a stretch of unmappable reads long enough to fill whole chunks
    recs += [("junk%d" % t, "".join(rng.choice("ACGT") for _ in range(80)), quals(rng, 80)) for t in range(60)]
    recs += [("z%d" % t, q, quals(rng, len(q))) for t, q in enumerate(make_reads(ref, 1, 20, seed=67))]
    for max_hits in (0, 3):
        want = expected_lines(engine, index, recs, 2, max_hits=max_hits)
        assert sum(1 for ln in want if ln.split("\t")[1] == "4") >= 62
        for eol, final in (("\n", True), ("\r\n", True), ("\n", False), ("\r\n", False)):
            fq, sam = tmp_path / "r.fq", tmp_path / "o.sam"
            write_fastq(fq, recs, eol=eol, final_newline=final)
            for chunk_bytes in (0, 2500):  # 2500 bytes: the junk stretch fills chunks of its own
                st = engine.map_file(index, NAMES, str(fq), str(sam), 2, max_hits=max_hits, chunk_bytes=chunk_bytes)
                got = sam_lines(sam)
                compare(got, want)
                check_stats(st, got, recs)
                assert st["too_long"] == 2
    # an empty file: the header alone
    fq, sam = tmp_path / "empty.fq", tmp_path / "empty.sam"
    fq.write_bytes(b"")
    st = engine.map_file(index, NAMES, str(fq), str(sam), 2, header="@HD\tVN:1.6\n")
    assert open(sam, "rb").read() == b"@HD\tVN:1.6\n"
    assert st["reads"] == st["records"] == st["mapped"] == st["chunks"] == 0


def test_errors_leave_the_handle_usable(asm, engine, ref, index, tmp_path):
    recs = records_for(make_reads(ref, 1, 30, seed=71), seed=6)
    text = "".join("@%s\n%s\n+\n%s\n" % r for r in recs)
    lines = text.split("\n")[:-1]
    sam = tmp_path / "o.sam"

    def run(data, **kw):
        fq = tmp_path / "bad.fq"
        fq.write_bytes(data.encode())
        with pytest.raises(asm.AsmError) as exc:
            engine.map_file(index, NAMES, str(fq), str(sam), 1, **kw)
        return exc.value

    bad0 = list(lines)
    bad0[4 * 17] = "x" + bad0[4 * 17][1:]
    bad2 = list(lines)
    bad2[4 * 5 + 2] = "-"
    for kw in ({}, {"chunk_bytes": 600}):
        err = run("\n".join(bad0) + "\n", **kw)
        assert err.code == -1 and "asm_map_file: record 18 is malformed" in str(err)
        err = run("\n".join(bad2) + "\n", **kw)
        assert err.code == -1 and "asm_map_file: record 6 is malformed" in str(err)
        err = run("\n".join(lines[:-1]) + "\n", **kw)
        assert err.code == -1 and "asm_map_file: record 30 is truncated" in str(err)
    err = run(">r0\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    assert err.code == -4 and "asm_map_file: FASTA reads are not supported" in str(err)
    with pytest.raises(asm.AsmError) as exc:
        engine.map_file(index, NAMES, str(tmp_path / "missing.fq"), str(sam), 1)
    assert exc.value.code == -1 and "cannot open" in str(exc.value)
    # the handle maps a good file afterwards
    fq = tmp_path / "good.fq"
    fq.write_bytes(text.encode())
    engine.map_file(index, NAMES, str(fq), str(sam), 1)
    compare(sam_lines(sam), expected_lines(engine, index, recs, 1))
