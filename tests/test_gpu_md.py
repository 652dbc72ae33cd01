"""MD:Z in the file calls' SAM (docs/design/mapper.md, "MD tag"): asm_map_set_sam_tags / Engine.set_sam_tags / asm-map --md.  With the
tag off every byte is the one an engine writes that never touched the setter; with it on, the file is the tag-off file plus one MD
behind XG on every line that shows a CIGAR, and every tag equals ref_md (tests/md_cases.py) of that line's own CIGAR, SEQ, POS and
the reference.  Single-end, all hits, pairs with rescue, both sorted calls, every chunking, the tool's ways to the same file and
Python's md_format on the in-memory records.

The shapes: three sequences of about 2 kbp, k = 8, and per e in {0, 3, 15} a file of 46 reads (138 in all): four recipes at each
of the lengths 31, 64, 65, 128, 129, 256, 257 and 511, both strands, then reads over the run of N, the lower-case stretch, the copied
stretch, '*' and '-', and five that stay unmapped (random, over-long, empty); the pairs are 48 fragments of the same lengths.

A read with more than 64 CIGAR operations (CIGAR '*', no MD) cannot be built: a row of more than 64 runs needs more than 31 edits and
the mapper allows 15.  The kernel's branch for it is the one that leaves the lines with CIGAR '*' without a tag."""
import os
import random
import subprocess

import pytest

from tests.md_cases import MD_FIELD, check_sam_md, ref_md, strip_md
from tests.map_cases import mid_edit
from tests.test_gpu_map_file import quals, write_fastq
from tests.test_map_host import BASES, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
NAMES = ["chrA", "chrB", "chrC"]
K = 8
LENGTHS = (31, 64, 65, 128, 129, 256, 257, 511)  # both sides of every kernel width and word edge
ERRORS = (0, 3, 15)
INSERT = (100, 900)
LIMIT = 120


def bases(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


@pytest.fixture(scope="module")
def ref():
    """three sequences of about 2 kbp: a run of N and a lower-case stretch in the first, a copy of a stretch of the first in the
    second (hits on two sequences: secondary lines), a '*' and a '-' in the third"""
    rng = random.Random(17)
    a, b, c = bases(rng, 2200), bases(rng, 2000), bases(rng, 1900)
    a = a[:700] + "N" * 40 + a[740:1200] + a[1200:1400].lower() + a[1400:]
    b = b[:600] + a[1500:1900] + b[1000:]
    c = c[:500] + "*" + c[501:520] + "-" + c[521:]
    return [a, b, c]


def del_spread(rng, src, m, x):
    """x single deleted reference bases at spaced read offsets, each between two bases that differ from it: 2x + 1 operations"""
    q, at = [], 0
    for p in [int((t + 0.5) * m / x) for t in range(x)]:
        while len(q) < p or src[at] == src[at - 1] or src[at] == src[at + 1]:
            q.append(src[at])
            at += 1
        at += 1
    return ("".join(q) + src[at:at + m])[:m]


def reads_for(ref, e, seed):
    """46 reads: every length, 0 / min(3, e) / e edits in a run of inserted or deleted bases, spaced substitutions or spaced
    deletions, both strands; then reads over the run of N, the lower-case stretch, the copied stretch and the bytes that are no
    letters; then what does not map: random reads, a read of 600 bases, an empty one"""
    rng = random.Random(seed)
    up = [s.upper() for s in ref]
    out = []
    for m in LENGTHS:
        for v, kind in enumerate(("ins", "del", "sub", "spread")):
            x = (0, min(3, e), e, e)[(v + m) % 4]
            s = up[rng.randrange(3)]
            for _ in range(200):
                a = rng.randrange(1, len(s) - m - x - 42)
                if not set("N*-") & set(s[a - 1:a + m + x + 42]):
                    break
            src = s[a:a + m + x + 42]
            q = del_spread(rng, src, m, x) if kind == "spread" and x else mid_edit(rng, src, m, x, kind if kind != "spread" else "sub")[0]
            out.append(revcomp(q) if (v + m) % 2 else q)
    a0 = ref[0].index("N")
    out += [up[0][a0 + 2 - 128:a0 + 2], revcomp(up[0][a0 + 39:a0 + 39 + 100]), ref[0][1180:1310], revcomp(up[0][1250:1500]).lower()]
    out += [up[0][1550:1650], revcomp(up[0][1600:1800]), up[1][650:800]]                  # on both chrA and chrB
    out += [up[2][450:500] + "A" + up[2][501:520] + "C" + up[2][521:600], revcomp(up[2][380:520] + "G" + up[2][521:560])]
    out += [bases(rng, 128), bases(rng, 300), bases(rng, 31), "ACGT" * 150, ""]
    return out


def records(reads, seed, tag="r"):
    rng = random.Random(seed)
    return [("%s%d comment" % (tag, t), q, quals(rng, len(q))) for t, q in enumerate(reads)]


def key_of(line):
    cols = line.split("\t")
    return (len(NAMES) if cols[2] == "*" else NAMES.index(cols[2]), int(cols[3]))


def py_sorted(data: bytes) -> bytes:
    return "".join(ln + "\n" for ln in sorted(data.decode("latin-1").split("\n")[:-1], key=key_of)).encode("latin-1")


def single_reader(recs):
    by = {h.split(" ")[0]: q for h, q, _ in recs}
    return lambda qname, flag: by[qname]


def pair_reader(recs1, recs2):
    by1 = {h.split(" ")[0].split("/")[0]: q for h, q, _ in recs1}
    by2 = {h.split(" ")[0].split("/")[0]: q for h, q, _ in recs2}
    return lambda qname, flag: (by2 if flag & 128 else by1)[qname]


@pytest.fixture(scope="module")
def md_engine(asm, ref):
    """an engine of its own with the tag on, and its index (the session's engine never touches the setter)"""
    eng = asm.Engine(0)
    assert eng.sam_tags == 0
    eng.set_sam_tags(md=True)
    assert eng.sam_tags == asm.SAM_TAG_MD
    ix = eng.build_index(ref, k=K)
    yield eng, ix
    ix.free()
    eng.close()


@pytest.fixture(scope="module")
def index(engine, ref):
    ix = engine.build_index(ref, k=K)
    yield ix
    ix.free()


@pytest.fixture(scope="module")
def singles(engine, index, md_engine, ref, tmp_path_factory):
    """per e: the records, the FASTQ file, and the best-hit file with the tag off (the session's engine) and on; computed once"""
    d = tmp_path_factory.mktemp("md_single")
    eng, ix = md_engine
    out = {}
    for e in ERRORS:
        recs = records(reads_for(ref, e, seed=100 + e), seed=e)
        fq = d / ("e%d.fq" % e)
        write_fastq(fq, recs)
        off, on = d / ("off%d.sam" % e), d / ("on%d.sam" % e)
        engine.map_file(index, NAMES, str(fq), str(off), e)
        eng.map_file(ix, NAMES, str(fq), str(on), e)
        out[e] = dict(recs=recs, fq=fq, off=open(off, "rb").read(), on=open(on, "rb").read())
    return out


def check_on_off(on: bytes, off: bytes, read_of, ref):
    """the tag-on file is the tag-off file plus the tags, and every line's tag, or its absence, is right; -> the tags"""
    assert strip_md(on) == off
    lines = on.decode("latin-1").split("\n")[:-1]
    tagged = check_sam_md(lines, read_of, ref, NAMES)
    assert tagged == len(MD_FIELD.findall(on.decode("latin-1"))) == sum(1 for ln in lines if ln.split("\t")[5] != "*") > 0
    return [ln.split("\tMD:Z:")[1].split("\t")[0] for ln in lines if "\tMD:Z:" in ln]


def test_tag_off_is_the_untouched_engine(asm, engine, index, ref, singles, tmp_path):
    assert engine.sam_tags == 0
    eng = asm.Engine(0)
    try:
        ix = eng.build_index(ref, k=K)
        eng.set_sam_tags(md=True)
        eng.set_sam_tags(md=False)
        assert eng.sam_tags == 0
        a, b = tmp_path / "a.sam", tmp_path / "b.sam"
        eng.map_file(ix, NAMES, str(singles[3]["fq"]), str(b), 3)
        assert open(b, "rb").read() == singles[3]["off"]
        engine.map_file(index, NAMES, str(singles[3]["fq"]), str(a), 3, max_hits=4)
        eng.map_file(ix, NAMES, str(singles[3]["fq"]), str(b), 3, max_hits=4)
        assert open(a, "rb").read() == open(b, "rb").read() and b"MD:Z" not in open(b, "rb").read()
        with pytest.raises(asm.AsmError):
            eng._chk(eng.lib.asm_map_set_sam_tags(eng.h, 2))
        assert eng.sam_tags == 0
        ix.free()
    finally:
        eng.close()
    assert b"MD:Z" not in singles[3]["off"]


@pytest.mark.parametrize("e", ERRORS)
def test_single_end_tags(ref, singles, e):
    s = singles[e]
    tags = check_on_off(s["on"], s["off"], single_reader(s["recs"]), ref)
    lines = s["on"].decode("latin-1").split("\n")[:-1]
    assert len(lines) == len(s["recs"])
    assert sum(1 for ln in lines if ln.split("\t")[1] == "4") >= 5                      # unmapped lines, without a tag
    assert sum(1 for ln in lines if ln.split("\t")[1] == "16" and "MD:Z" in ln) >= 8   # strand 1
    assert {len(ln.split("\t")[9]) for ln in lines if "MD:Z" in ln} >= set(LENGTHS) - ({31} if e else set()) - ({64, 65} if e == 15 else set())
    if e:
        assert any("^" in t for t in tags) and any("I" in ln.split("\t")[5] and "MD:Z" in ln for ln in lines)
        assert any("N" in t for t in tags)                                              # N against N, '*' and '-'
        assert any("0" + c in t for t in tags for c in "ACGTN")                          # a letter right behind a letter or a deletion
    if e == 15:
        assert max(t.count("^") for t in tags) >= 14 and max(len(t) for t in tags) >= 50
    if e == 0:
        assert all(t.isdigit() for t in tags)


def test_all_hits_tags(engine, index, md_engine, ref, singles, tmp_path):
    eng, ix = md_engine
    s = singles[3]
    off, on = tmp_path / "off.sam", tmp_path / "on.sam"
    engine.map_file(index, NAMES, str(s["fq"]), str(off), 3, max_hits=4)
    eng.map_file(ix, NAMES, str(s["fq"]), str(on), 3, max_hits=4)
    on_b, off_b = open(on, "rb").read(), open(off, "rb").read()
    check_on_off(on_b, off_b, single_reader(s["recs"]), ref)
    sec = [ln for ln in on_b.decode("latin-1").split("\n")[:-1] if int(ln.split("\t")[1]) & 256]
    assert len(sec) >= 3 and all(ln.split("\t")[9] == "*" and "\tMD:Z:" in ln and "\tNH:i:" in ln.split("\tMD:Z:")[1] for ln in sec)
    assert any(int(ln.split("\t")[1]) & 16 for ln in sec)
    # sorted: the stable sort of the unsorted tag-on file
    srt = tmp_path / "sorted.sam"
    eng.map_file(ix, NAMES, str(s["fq"]), str(srt), 3, max_hits=4, sort=True)
    assert open(srt, "rb").read() == py_sorted(on_b) != on_b


def pair_records(ref, e, seed):
    """FR pairs of every length: concordant ones with up to e edits per mate, pairs whose second mate needs the rescue (more than e
    edits, or too short to seed), pairs whose second mate maps nowhere (it borrows its mate's position), junk pairs"""
    rng = random.Random(seed)
    up = [s.upper() for s in ref]
    r1, r2 = [], []
    for t in range(48):
        m1, m2 = LENGTHS[t % 8], LENGTHS[(t // 2 + 3) % 8]
        s = up[1 + t % 2]  # chrB and chrC: no run of N
        length = max(m1, m2) + 120 + rng.randrange(150)
        a = rng.randrange(len(s) - length)
        f = s[a:a + length]
        kind = t % 6
        x1, x2 = rng.randint(0, e), (e + 2 if kind == 3 else rng.randint(0, e))
        q1 = mid_edit(rng, f, m1, x1, ("ins", "del", "sub")[t % 3])[0] if m1 >= (e + 1) * K else f[:m1]
        q2 = mid_edit(rng, revcomp(f), m2, x2, ("sub", "ins", "del")[t % 3])[0]
        if kind == 4:
            q2 = bases(rng, m2)
        if kind == 5:
            q1, q2 = bases(rng, m1), bases(rng, m2)
        if t % 4 >= 2:
            q1, q2 = q2, q1
        r1.append(q1), r2.append(q2)
    rng2 = random.Random(seed + 1)
    recs1 = [("p%d%s first" % (t, "/1" if t % 3 == 0 else ""), q, quals(rng2, len(q))) for t, q in enumerate(r1)]
    recs2 = [("p%d%s" % (t, "/2" if t % 3 == 0 else ""), q, quals(rng2, len(q))) for t, q in enumerate(r2)]
    return recs1, recs2


def test_pairs_with_rescue_tags(engine, index, md_engine, ref, tmp_path):
    eng, ix = md_engine
    e = 3
    recs1, recs2 = pair_records(ref, e, seed=23)
    f1, f2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    write_fastq(f1, recs1), write_fastq(f2, recs2)
    off, on, srt = tmp_path / "off.sam", tmp_path / "on.sam", tmp_path / "sorted.sam"
    args = (str(f1), str(f2))
    engine.map_pairs_file(index, NAMES, *args, str(off), e, *INSERT, rescue_errors=8)
    st = eng.map_pairs_file(ix, NAMES, *args, str(on), e, *INSERT, rescue_errors=8)
    on_b = open(on, "rb").read()
    check_on_off(on_b, open(off, "rb").read(), pair_reader(recs1, recs2), ref)
    lines = on_b.decode("latin-1").split("\n")[:-1]
    assert len(lines) == 2 * len(recs1) and st["rescued"] >= 3
    resc = [ln for ln in lines if "\tXR:i:1" in ln]
    assert len(resc) >= 3 and all("\tMD:Z:" in ln and ln.index("\tMD:Z:") < ln.index("\tXR:i:1") for ln in resc)
    lent = [ln for ln in lines if int(ln.split("\t")[1]) & 4 and ln.split("\t")[2] != "*"]
    assert len(lent) >= 3 and not any("MD:Z" in ln for ln in lent)   # an unmapped mate that borrows RNAME and POS
    assert sum(1 for ln in lines if "\tXP:i:" in ln and "\tMD:Z:" in ln and ln.index("\tMD:Z:") < ln.index("\tXP:i:")) >= 20
    eng.map_pairs_file(ix, NAMES, *args, str(srt), e, *INSERT, rescue_errors=8, sort=True)
    assert open(srt, "rb").read() == py_sorted(on_b) != on_b
    small = tmp_path / "small.sam"
    eng.map_pairs_file(ix, NAMES, *args, str(small), e, *INSERT, rescue_errors=8, chunk_bytes=2000)
    assert open(small, "rb").read() == on_b


def test_chunking_does_not_change_the_tags(asm, md_engine, ref, singles, tmp_path, monkeypatch):
    eng, ix = md_engine
    s = singles[15]
    for chunk_bytes in (1500, 7777):
        sam = tmp_path / ("c%d.sam" % chunk_bytes)
        st = eng.map_file(ix, NAMES, str(s["fq"]), str(sam), 15, chunk_bytes=chunk_bytes)
        assert open(sam, "rb").read() == s["on"] and st["chunks"] > 1
    # several device chunks per file chunk, and a read's items spanning them: a fresh engine reads ASM_MAP_CHUNK
    monkeypatch.setenv("ASM_MAP_CHUNK", "16")
    eng2 = asm.Engine(0)
    try:
        eng2.set_sam_tags(md=True)
        ix2 = eng2.build_index(ref, k=K)
        sam = tmp_path / "small.sam"
        st = eng2.map_file(ix2, NAMES, str(s["fq"]), str(sam), 15)
        assert open(sam, "rb").read() == s["on"] and st["chunks"] == (len(s["recs"]) + 15) // 16
        want, got = tmp_path / "all.sam", tmp_path / "all16.sam"
        eng.map_file(ix, NAMES, str(singles[3]["fq"]), str(want), 3, max_hits=4)
        eng2.map_file(ix2, NAMES, str(singles[3]["fq"]), str(got), 3, max_hits=4)
        assert open(got, "rb").read() == open(want, "rb").read()
        ix2.free()
    finally:
        eng2.close()
        monkeypatch.delenv("ASM_MAP_CHUNK")


def test_python_md_format_on_the_in_memory_records(asm, engine, index, ref, singles):
    """md_format on map_reads' records gives the tags the file carries for the same reads"""
    s = singles[3]
    sent = [(h.split(" ")[0], q.upper()) for h, q, _ in s["recs"] if 1 <= len(q) <= 511]
    out = engine.map_reads(index, [q for _, q in sent], 3)
    in_file = {ln.split("\t")[0]: ln.split("\tMD:Z:")[1].split("\t")[0] for ln in s["on"].decode("latin-1").split("\n")[:-1] if "\tMD:Z:" in ln}
    seen = 0
    for t, (name, q) in enumerate(sent):
        if not out["mapped"][t]:
            assert name not in in_file
            continue
        window = ref[int(out["seq_id"][t])].upper()[int(out["pos"][t]):int(out["end"][t])]
        qs = revcomp(q) if out["strand"][t] else q
        assert asm.md_format(out["cigar"][t], qs, window) == in_file[name] == ref_md(out["cigar"][t], qs, window)
        seen += 1
    assert seen == len(in_file) >= 30


def write_reference(path, seqs):
    with open(path, "w") as fh:
        for nm, s in zip(NAMES, seqs):
            fh.write(">%s some description\n" % nm)
            for a in range(0, len(s), 70):
                fh.write(s[a:a + 70] + "\n")


def run_tool(tmp_path, tag, args):
    sam = tmp_path / (tag + ".sam")
    r = subprocess.run([EXE] + args + ["-o", str(sam), "--k", str(K)], capture_output=True, text=True, timeout=LIMIT)
    assert r.returncode == 0, r.stderr[-2000:]
    data = open(sam, "rb").read().decode("latin-1")
    lines = data.split("\n")[:-1]
    pg = [ln for ln in lines if ln.startswith("@PG")]
    assert len(pg) == 1 and " --md" in pg[0].split("\tCL:")[1]
    return [ln for ln in lines if not ln.startswith("@PG")]


def test_tool_single_end(ref, singles, tmp_path):
    """asm-map --md: streamed = non-streamed, --stream --sort = non-streamed --sort, --ref-stream; with --all-hits, so that the
    tool's own secondary lines carry their tags"""
    s = singles[3]
    fa = tmp_path / "ref.fa"
    write_reference(fa, ref)
    common = ["-r", str(fa), "-q", str(s["fq"]), "-e", "3", "--both-strands", "--all-hits", "4", "--md"]
    plain = run_tool(tmp_path, "plain", common)
    assert run_tool(tmp_path, "stream", common + ["--stream"]) == plain
    hsort = run_tool(tmp_path, "hsort", common + ["--sort", "--ref-stream"])
    assert run_tool(tmp_path, "dsort", common + ["--stream", "--sort"]) == hsort
    rows = [ln for ln in plain if not ln.startswith("@")]
    assert sorted(rows, key=key_of) == [ln for ln in hsort if not ln.startswith("@")] != rows
    assert check_sam_md(rows, single_reader(s["recs"]), ref, NAMES) >= 35 and any(int(ln.split("\t")[1]) & 256 for ln in rows)


def test_tool_pairs(ref, tmp_path):
    """asm-map -1 -2 --md = --stream-pairs --md; paired --all-hits --md, the tool's own path, against ref_md"""
    recs1, recs2 = pair_records(ref, 3, seed=23)
    fa, f1, f2 = tmp_path / "ref.fa", tmp_path / "r1.fq", tmp_path / "r2.fq"
    write_reference(fa, ref), write_fastq(f1, recs1), write_fastq(f2, recs2)
    common = ["-r", str(fa), "-1", str(f1), "-2", str(f2), "-e", "3", "--insert", "%d,%d" % INSERT, "--rescue", "8", "--md"]
    plain = run_tool(tmp_path, "plain", common)
    assert run_tool(tmp_path, "stream", common + ["--stream-pairs", "--ref-stream"]) == plain
    rows = [ln for ln in plain if not ln.startswith("@")]
    assert check_sam_md(rows, pair_reader(recs1, recs2), ref, NAMES) >= 60
    every = [ln for ln in run_tool(tmp_path, "all", common + ["--all-hits", "3"]) if not ln.startswith("@")]
    assert check_sam_md(every, pair_reader(recs1, recs2), ref, NAMES) >= 60
