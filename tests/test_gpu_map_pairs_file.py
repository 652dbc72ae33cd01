"""asm_map_pairs_file / Engine.map_pairs_file / asm-map --stream-pairs (docs/design/mapper.md, "Files: two FASTQ files in, paired SAM
out"): two FASTQ files parsed, paired, mapped and formatted on the device must give, byte for byte, the SAM lines formatted here in
Python from Engine.map_pairs on the same reads, and the lines the non-streamed asm-map -1 -2 writes, whatever the chunking."""
import os
import random
import subprocess

import pytest

from tests.test_gpu_map import make_reference
from tests.test_gpu_map_file import NAMES, compare, quals, sam_lines, write_fastq, write_reference
from tests.test_gpu_map_pairs import INSERT, make_pairs
from tests.test_map_host import revcomp
from tests.test_map_pairs_file_host import pair_name

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
E = 2
LIMIT = 300


@pytest.fixture(scope="module")
def ref():
    return make_reference()


@pytest.fixture(scope="module")
def index(engine, ref):
    ix = engine.build_index(ref, k=12)
    yield ix
    ix.free()


def first_word(h):
    return (h.lstrip(" \t").replace("\t", " ").split(" ") + [""])[0]


def mates_for(r1s, r2s, seed, tags=("/1", "/2")):
    """(header, seq, qual) records of the two files; every third pair carries the /1 and /2 tags, the others bare names"""
    rng = random.Random(seed)
    a, b = [], []
    for t, (q1, q2) in enumerate(zip(r1s, r2s)):
        tag = tags if t % 3 == 0 else ("", "")
        a.append(("frag%d%s first mate" % (t, tag[0]), q1, quals(rng, len(q1))))
        b.append(("frag%d%s" % (t, tag[1]), q2, quals(rng, len(q2))))
    return a, b


def expected_lines(engine, index, recs1, recs2, e, rescue):
    """the paired SAM lines by the contract, from Engine.map_pairs on the pairs whose mates both have 1..511 bytes"""
    sent = [t for t in range(len(recs1)) if 1 <= len(recs1[t][1]) <= 511 and 1 <= len(recs2[t][1]) <= 511]
    out = engine.map_pairs(index, [recs1[t][1].upper() for t in sent], [recs2[t][1].upper() for t in sent], e, *INSERT,
                           rescue_errors=rescue) if sent else None
    slot = {t: i for i, t in enumerate(sent)}
    lines, proper, rescued = [], 0, 0
    for t in range(len(recs1)):
        i = slot.get(t)
        recs = (recs1[t], recs2[t])
        mapped = [i is not None and bool(out["mapped"][i, x]) for x in (0, 1)]
        is_proper = i is not None and bool(out["proper"][i])
        proper += is_proper
        where = []
        for x in (0, 1):
            y = x if mapped[x] else 1 - x if mapped[1 - x] else None
            where.append((-1, 0) if y is None else (int(out["seq_id"][i, y]), int(out["pos"][i, y]) + 1))
        tl = int(out["tlen"][i]) if i is not None else 0
        plus = 0 if where[0][1] <= where[1][1] else 1
        for x in (0, 1):
            y = 1 - x
            h, s, q = recs[x]
            flag = 1 | (2 if is_proper else 0) | (0 if mapped[x] else 4) | (0 if mapped[y] else 8) | (128 if x else 64)
            seq, qual, cigar, mapq = s.upper(), q, "*", 0
            if mapped[x]:
                st = int(out["strand"][i, x])
                flag |= 16 if st else 0
                seq, qual = (revcomp(seq), q[::-1]) if st else (seq, q)
                cigar = "*" if int(out["cigar_nops"][i, x]) > 64 else out["cigar"][i][x]
                mapq = int(out["mapq"][i, x])
            if mapped[y] and int(out["strand"][i, y]):
                flag |= 32
            rnext = "*" if not mapped[y] else "=" if where[y][0] == where[x][0] else NAMES[where[y][0]]
            line = "%s\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s" % (
                pair_name(first_word(h)), flag, "*" if where[x][0] < 0 else NAMES[where[x][0]], where[x][1], mapq, cigar, rnext, where[y][1],
                tl if x == plus else -tl, seq or "*", qual or "*")
            if mapped[x]:
                line += "\tNM:i:%d\tXG:i:%d" % (int(out["dist"][i, x]), int(out["greedy_cost"][i, x]))
            if is_proper:
                line += "\tXP:i:%d" % int(out["n_concordant"][i])
            if i is not None and bool(out["rescued"][i, x]):
                line += "\tXR:i:1"
                rescued += 1
            lines.append(line)
    return lines, dict(pairs=len(recs1), proper=proper, rescued=rescued, unsent=len(recs1) - len(sent))


def check_stats(st, want, body, header_bytes, sam):
    for k, v in want.items():
        assert st[k] == v, (k, st[k], v)
    assert st["records"] == 2 * want["pairs"] == len(body)
    assert st["bytes_out"] == os.path.getsize(sam) - header_bytes == sum(len(ln) + 1 for ln in body)


def run_file(engine, index, tmp_path, recs1, recs2, rescue, tag="o", e=E, eol=("\n", "\n"), final=(True, True), **kw):
    f1, f2, sam = tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / (tag + ".sam")
    write_fastq(f1, recs1, eol=eol[0], final_newline=final[0])
    write_fastq(f2, recs2, eol=eol[1], final_newline=final[1])
    st = engine.map_pairs_file(index, NAMES, str(f1), str(f2), str(sam), e, *INSERT, rescue_errors=rescue, **kw)
    size = os.path.getsize(f1) + os.path.getsize(f2)
    assert size <= st["bytes_in"] <= size + 2  # a missing final newline is added
    return st, sam


@pytest.mark.parametrize("rescue", [-1, 4])
def test_lines_equal_the_library(engine, ref, index, tmp_path, rescue):
    r1s, r2s, kinds = make_pairs(ref, E, 320, seed=901)
    recs1, recs2 = mates_for(r1s, r2s, seed=5)
    header = "@HD\tVN:1.6\n@CO\tpairs\n"
    st, sam = run_file(engine, index, tmp_path, recs1, recs2, rescue, header=header)
    got = sam_lines(sam)
    assert got[:2] == header.split("\n")[:2]
    want, counts = expected_lines(engine, index, recs1, recs2, E, rescue)
    compare(got[2:], want)
    check_stats(st, counts, got[2:], len(header), sam)
    flags = [int(ln.split("\t")[1]) for ln in want]
    assert counts["proper"] >= 80 and (counts["rescued"] > 0) == (rescue >= 0) and st["chunks"] >= 1
    assert any(f & 4 and not f & 8 for f in flags) and any(f & 4 and f & 8 for f in flags)  # one mate unmapped; both
    assert any(not f & 2 and not f & 12 for f in flags)  # both mapped, not proper (too far apart, same strand, other sequence)
    assert any(ln.split("\t")[6] not in "*=" for ln in want)  # mates on different sequences


def test_streamed_tool_writes_the_tools_bytes(asm, ref, tmp_path):
    assert os.path.exists(EXE), "asm-map is built by build()"
    r1s, r2s, _ = make_pairs(ref, E, 240, seed=907)
    recs1, recs2 = mates_for(r1s, r2s, seed=7)
    recs1.append(("long/1", "ACGT" * 150, "I" * 600))
    recs2.append(("long/2", "ACGT" * 25, "I" * 100))
    fa, f1, f2 = tmp_path / "ref.fa", tmp_path / "r1.fq", tmp_path / "r2.fq"
    write_reference(fa, ref)
    write_fastq(f1, recs1)
    write_fastq(f2, recs2)
    for rescue in ([], ["--rescue", "4"]):
        outs = []
        for extra in ([], ["--stream-pairs"], ["--stream-pairs", "--chunk-bytes", "20000"]):
            sam = tmp_path / ("o%d.sam" % len(outs))
            r = subprocess.run([EXE, "-r", str(fa), "-1", str(f1), "-2", str(f2), "-o", str(sam), "-e", str(E), "--insert", "%d,%d" % INSERT]
                               + rescue + extra, capture_output=True, text=True, timeout=LIMIT)
            assert r.returncode == 0, r.stderr[-2000:]
            outs.append((sam_lines(sam), r.stderr.splitlines()))
        plain, err0 = outs[0]
        assert len(plain) > 2 * len(recs1) and err0[0].startswith("asm-map: %d pairs, " % len(recs1))
        for streamed, err in outs[1:]:
            assert len(plain) == len(streamed)
            for a, b in zip(plain, streamed):
                if a.startswith("@PG"):
                    assert b.startswith("@PG") and a.split("\tCL:")[0] == b.split("\tCL:")[0] and " --stream-pairs" in b
                else:
                    assert a == b
            assert err[0] == err0[0] and err[1].startswith("asm-map: streamed ")


def test_chunking_does_not_change_the_output(asm, engine, ref, index, tmp_path, monkeypatch):
    """mates of 30-60 bp in file 1 and 200-300 bp in file 2: the two files cut at different bytes"""
    rng = random.Random(911)
    up = [s.upper().replace("N", "A") for s in ref]
    r1s, r2s = [], []
    for t in range(300):
        m1, m2, f = rng.randint(30, 60), rng.randint(200, 300), rng.randint(320, 480)
        r = rng.randrange(len(up))
        a = rng.randrange(len(up[r]) - f)
        frag = up[r][a:a + f]
        # the mates face each other in both layouts: mate 1 forward at the fragment's left end, or reverse at its right end
        q1, q2 = (frag[:m1], revcomp(frag[f - m2:])) if t % 2 else (revcomp(frag[f - m1:]), frag[:m2])
        if t % 7 == 3:
            q2 = "".join(rng.choice("ACGT") for _ in range(m2))
        r1s.append(q1)
        r2s.append(q2)
    recs1, recs2 = mates_for(r1s, r2s, seed=9)
    want, counts = expected_lines(engine, index, recs1, recs2, E, 4)
    want_bytes = ("\n".join(want) + "\n").encode()
    # 257 of the 300 pairs are exact, inward-facing and 320..480 apart, inside INSERT; the loose bound leaves room for fragments
    # over the run of N and for mates 1 below (E + 1) * k = 36 bp, which cannot be seeded and depend on rescue
    assert counts["proper"] > 150
    monkeypatch.setenv("ASM_MAP_CHUNK", "16")  # 8 pairs per device chunk
    small = asm.Engine(0)
    monkeypatch.delenv("ASM_MAP_CHUNK")
    try:
        ix2 = small.build_index(ref, k=12)
        for eng, ix, per_chunk in ((engine, index, None), (small, ix2, 8)):
            for chunk_bytes in (4096, 65536, 0):
                st, sam = run_file(eng, ix, tmp_path, recs1, recs2, 4, tag="c%d" % chunk_bytes, chunk_bytes=chunk_bytes)
                assert open(sam, "rb").read() == want_bytes, (chunk_bytes, per_chunk)
                check_stats(st, counts, want, 0, sam)
                if chunk_bytes:
                    assert 0 < st["carry_peak"] <= chunk_bytes, (chunk_bytes, st["carry_peak"])
                if chunk_bytes == 4096:
                    assert st["chunks"] > 1
                if per_chunk and chunk_bytes == 0:
                    assert st["chunks"] == (len(recs1) + per_chunk - 1) // per_chunk
        ix2.free()
    finally:
        small.close()


@pytest.mark.parametrize("at", [0, 6])
def test_record_longer_than_the_pinned_slot(engine, ref, index, tmp_path, at):
    """chunk_bytes=1000 gives pinned slots of 1000 + 1000 / 4 + 4096 = 5,346 bytes; a mate 1 whose sequence and quality are 6,000
    bytes each does not fit one, so the reader has the slot replaced by a larger one: as the files' first pair, and in the middle of
    them behind the carries.  The bytes are those of the library's call and those of the default chunk, which holds both files."""
    rng = random.Random(923)
    r1s, r2s, _ = make_pairs(ref, E, 12, seed=929)
    recs1, recs2 = mates_for(r1s, r2s, seed=15)
    recs1.insert(at, ("long/1", "".join(rng.choice("ACGT") for _ in range(6000)), quals(rng, 6000)))
    recs2.insert(at, ("long/2", ref[1][30_000:30_100].upper(), quals(rng, 100)))
    want, counts = expected_lines(engine, index, recs1, recs2, E, 4)
    assert counts["unsent"] == 1
    out = {}
    for chunk_bytes in (0, 1000):
        st, sam = run_file(engine, index, tmp_path, recs1, recs2, 4, tag="c%d" % chunk_bytes, chunk_bytes=chunk_bytes)
        got = sam_lines(sam)
        compare(got, want)
        check_stats(st, counts, got, 0, sam)
        assert st["unsent"] == 1
        out[chunk_bytes] = (open(sam, "rb").read(), st["chunks"])
    assert out[1000][0] == out[0][0]
    assert out[0][1] == 1 and out[1000][1] > 1


def test_format_corners(engine, ref, index, tmp_path):
    rng = random.Random(919)
    r1s, r2s, _ = make_pairs(ref, E, 48, seed=913)
    recs1, recs2 = mates_for(r1s, r2s, seed=11)
    src = ref[1][20_000:20_900].upper().replace("N", "A")

    def add(name1, q1, name2, q2, qual1=None, qual2=None):
        recs1.append((name1, q1, quals(rng, len(q1)) if qual1 is None else qual1))
        recs2.append((name2, q2, quals(rng, len(q2)) if qual2 is None else qual2))

    add("emptymate/1", "", "emptymate/2", revcomp(src[300:400]), qual1="")
    add("bothempty", "", "bothempty", "", qual1="", qual2="")
    add("len512/1", src[:512], "len512/2", revcomp(src[600:700]))
    add("len511", src[:511], "len511", revcomp(src[520:820]))
    add("lower", src[100:200].lower(), "lower", revcomp(src[400:500]).lower())
    add("withN/1 x", src[100:150] + "N" + src[151:200], "withN/2\ty", revcomp(src[400:500]))
    add("atqual", src[120:220], "atqual", revcomp(src[420:520]), qual1="@" + quals(rng, 98) + "+", qual2="+" + quals(rng, 99))
    add("slash/3", src[100:200], "slash/3", revcomp(src[400:500]))
    add("bare/", src[100:200], "bare/", revcomp(src[400:500]))
    add("cross/2", src[100:200], "cross/1", revcomp(src[400:500]))  # the tags go in either file
    add("starqual", src[100:200], "starqual", revcomp(src[400:500]), qual1="*")
    for rescue in (-1, 4):
        want, counts = expected_lines(engine, index, recs1, recs2, E, rescue)
        assert counts["unsent"] == 3
        for eol, final in ((("\n", "\n"), (True, True)), (("\r\n", "\r\n"), (True, True)), (("\n", "\r\n"), (False, True)),
                           (("\n", "\n"), (True, False))):
            for chunk_bytes in (0, 3000):
                st, sam = run_file(engine, index, tmp_path, recs1, recs2, rescue, eol=eol, final=final, chunk_bytes=chunk_bytes)
                got = sam_lines(sam)
                compare(got, want)
                check_stats(st, counts, got, 0, sam)
    by_name = {ln.split("\t")[0]: ln.split("\t") for ln in want[::2]}
    assert by_name["len512"][1] == "77" and by_name["len512"][5] == "*" and len(by_name["len512"][9]) == 512
    assert by_name["emptymate"][9] == "*" and by_name["emptymate"][10] == "*" and by_name["bothempty"][1] == "77"
    assert {"slash/3", "bare/", "cross", "withN", "len511", "lower"} <= set(by_name)
    # two empty files: the header alone
    f1, f2, sam = tmp_path / "e1.fq", tmp_path / "e2.fq", tmp_path / "e.sam"
    f1.write_bytes(b"")
    f2.write_bytes(b"")
    st = engine.map_pairs_file(index, NAMES, str(f1), str(f2), str(sam), E, *INSERT, header="@HD\tVN:1.6\n")
    assert open(sam, "rb").read() == b"@HD\tVN:1.6\n"
    assert st["pairs"] == st["records"] == st["proper"] == st["chunks"] == st["bytes_out"] == 0


# ---- errors: after every one a correct call on the same handle succeeds ----------------------------------------------------------------
@pytest.fixture(scope="module")
def good(engine, ref, index):
    r1s, r2s, _ = make_pairs(ref, E, 30, seed=921)
    recs1, recs2 = mates_for(r1s, r2s, seed=13)
    want, _ = expected_lines(engine, index, recs1, recs2, E, -1)
    return recs1, recs2, want


def text_of(recs):
    return "".join("@%s\n%s\n+\n%s\n" % r for r in recs)


def expect_error(asm, engine, index, tmp_path, good, data1, data2, code, message, eng=None, ix=None, **kw):
    f1, f2, sam = tmp_path / "bad1.fq", tmp_path / "bad2.fq", tmp_path / "bad.sam"
    f1.write_bytes(data1.encode())
    f2.write_bytes(data2.encode())
    with pytest.raises(asm.AsmError) as exc:
        (eng or engine).map_pairs_file(ix or index, NAMES, str(f1), str(f2), str(sam), E, *INSERT, **kw)
    assert exc.value.code == code and message in str(exc.value), str(exc.value)
    recs1, recs2, want = good
    st, sam = run_file(eng or engine, ix or index, tmp_path, recs1, recs2, -1, tag="after")
    compare(sam_lines(sam), want)


def test_error_malformed_record_in_file_2(asm, engine, index, tmp_path, good):
    recs1, recs2, _ = good
    lines = text_of(recs2).split("\n")[:-1]
    lines[4 * 17] = "x" + lines[4 * 17][1:]
    for kw in ({}, {"chunk_bytes": 2000}):
        expect_error(asm, engine, index, tmp_path, good, text_of(recs1), "\n".join(lines) + "\n", -1,
                     "asm_map_pairs_file: record 18 of file 2 is malformed", **kw)
    # in one chunk a malformed record of file 1 comes first, whatever its number
    bad1 = text_of(recs1).split("\n")[:-1]
    bad1[4 * 25 + 2] = "-"
    expect_error(asm, engine, index, tmp_path, good, "\n".join(bad1) + "\n", "\n".join(lines) + "\n", -1,
                 "asm_map_pairs_file: record 26 of file 1 is malformed")


def test_error_truncated_file_1(asm, engine, index, tmp_path, good):
    recs1, recs2, _ = good
    lines = text_of(recs1).split("\n")[:-1]
    for kw in ({}, {"chunk_bytes": 2000}):
        expect_error(asm, engine, index, tmp_path, good, "\n".join(lines[:-1]) + "\n", text_of(recs2), -1,
                     "asm_map_pairs_file: record 30 of file 1 is truncated", **kw)


def test_error_file_2_one_record_longer(asm, engine, index, tmp_path, good):
    recs1, recs2, _ = good
    for kw in ({}, {"chunk_bytes": 2000}):
        expect_error(asm, engine, index, tmp_path, good, text_of(recs1), text_of(recs2 + [("extra", "ACGTACGT", "IIIIIIII")]), -1,
                     "asm_map_pairs_file: record 31 of file 2 has no mate", **kw)
    expect_error(asm, engine, index, tmp_path, good, text_of(recs1), text_of(recs2[:-1]), -1, "asm_map_pairs_file: record 30 of file 1 has no mate")


def test_error_names_differ_in_the_second_device_chunk(asm, ref, tmp_path, good, monkeypatch, engine, index):
    recs1, recs2, _ = good
    other = list(recs2)
    other[21] = ("someone_else/2",) + other[21][1:]
    other[27] = ("another",) + other[27][1:]
    monkeypatch.setenv("ASM_MAP_CHUNK", "32")  # 16 pairs per device chunk: pair 22 lies in the second one
    small = asm.Engine(0)
    monkeypatch.delenv("ASM_MAP_CHUNK")
    try:
        ix2 = small.build_index(ref, k=12)
        expect_error(asm, engine, index, tmp_path, good, text_of(recs1), text_of(other), -1,
                     "asm_map_pairs_file: the mates of record 22 have different names", eng=small, ix=ix2)
        ix2.free()
    finally:
        small.close()


def test_error_fasta_in_file_2(asm, engine, index, tmp_path, good):
    recs1, _, _ = good
    expect_error(asm, engine, index, tmp_path, good, text_of(recs1), ">r0\nACGTACGTACGTACGTACGTACGTACGTACGT\n", -4,
                 "asm_map_pairs_file: FASTA reads are not supported (file 2")


def test_error_arguments(asm, engine, index, tmp_path, good):
    recs1, recs2, want = good
    f1, f2, sam = tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "o.sam"
    f1.write_text(text_of(recs1))
    f2.write_text(text_of(recs2))

    def bad(message, **kw):
        a = dict(max_errors=E, min_insert=INSERT[0], max_insert=INSERT[1])
        a.update(kw)
        with pytest.raises(asm.AsmError) as exc:
            engine.map_pairs_file(index, NAMES, str(f1), str(f2), str(sam), **a)
        assert exc.value.code == -1 and message in str(exc.value), str(exc.value)

    bad("asm_map_pairs_file: max_errors must be in [0, 15]", max_errors=16)
    bad("asm_map_pairs_file: need 0 <= min_insert <= max_insert <= 8192", min_insert=600)
    bad("asm_map_pairs_file: need 0 <= min_insert <= max_insert <= 8192", max_insert=9000)
    bad("asm_map_pairs_file: rescue_errors must be -1 (off) or in [0, 15]", rescue_errors=16)
    bad("asm_map_pairs_file: chunk_bytes must be >= 0", chunk_bytes=-1)
    bad("asm_map_pairs_file: greedy_k must be in [0, 50]", greedy_k=51)
    assert not sam.exists()  # the checks come before any file is touched
    lib = asm.load_library()
    p, pp = asm.MapParams(E, 1, 0, 3), asm.PairParams(INSERT[0], INSERT[1], -1)
    import ctypes

    arr = (ctypes.c_char_p * 3)(*[n.encode() for n in NAMES])
    for args in ((None, os.fsencode(f2), os.fsencode(sam)), (os.fsencode(f1), None, os.fsencode(sam)), (os.fsencode(f1), os.fsencode(f2), None)):
        assert lib.asm_map_pairs_file(engine.h, index.ptr, arr, args[0], args[1], args[2], None, ctypes.byref(p), ctypes.byref(pp), 0, None) == -1
        assert lib.asm_last_error(engine.h).decode() == "asm_map_pairs_file: bad arguments"
    with pytest.raises(asm.AsmError) as exc:
        engine.map_pairs_file(index, NAMES, str(tmp_path / "missing.fq"), str(f2), str(sam), E, *INSERT)
    assert exc.value.code == -1 and "cannot open" in str(exc.value)
    st = engine.map_pairs_file(index, NAMES, str(f1), str(f2), str(sam), E, *INSERT)
    compare(sam_lines(sam), want)


def test_streamed_pairs_tool_usage(ref, tmp_path):
    fa, fq, fasta = tmp_path / "ref.fa", tmp_path / "r.fq", tmp_path / "r.fa"
    write_reference(fa, ref)
    fq.write_text("@frag0\n%s\n+\n%s\n" % (ref[0][1000:1100].upper(), "I" * 100))
    fasta.write_text(">frag0\nACGTACGTACGTACGTACGTACGTACGT\n")
    base = [EXE, "-r", str(fa), "-o", str(tmp_path / "x.sam"), "-e", "1"]
    r = subprocess.run(base + ["-q", str(fq), "--stream-pairs"], capture_output=True, text=True, timeout=LIMIT)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run(base + ["-1", str(fq), "-2", str(fq), "--insert", "100,500", "--all-hits", "4", "--stream-pairs"], capture_output=True,
                       text=True, timeout=LIMIT)
    assert r.returncode == 2 and "usage" in r.stderr
    for one, two in ((fq, fasta), (fasta, fq)):
        r = subprocess.run(base + ["-1", str(one), "-2", str(two), "--insert", "100,500", "--stream-pairs"], capture_output=True, text=True,
                           timeout=LIMIT)
        assert r.returncode == 1 and r.stderr.strip() == "asm-map: --stream-pairs needs FASTQ reads"
