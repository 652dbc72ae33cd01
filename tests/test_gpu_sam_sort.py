"""asm_map_file_sorted / asm_map_pairs_file_sorted / Engine.map_file(sort=True) / asm-map --sort (docs/design/mapper.md, "Sorted
output"): the sorted file is the header and then the unsorted call's lines, byte for byte, in the order of Python's stable
sorted(..., key=(tid, POS)), whatever the chunking and the slabs; the copy's edges, the degenerate inputs, the stats, the memory cap
and the tool's two ways to the same file."""
import os
import random
import signal
import subprocess

import pytest

from tests.test_gpu_map import mutate
from tests.test_gpu_map_file import quals, write_fastq, write_reference
from tests.test_map_host import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
NAMES = ["chrA", "chrB", "chrC"]
HEADER = "@HD\tVN:1.6\tSO:coordinate\n@CO\tthe caller's header, as it is\n"
E = 2
INSERT = (100, 500)
LIMIT = 120  # seconds per test


@pytest.fixture(autouse=True)
def time_limit():
    def over(signum, frame):
        raise TimeoutError("test ran longer than %d s" % LIMIT)

    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(LIMIT)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


@pytest.fixture(scope="module")
def ref():
    """about 12 kbp, about 6 kbp with a segment of the first (hits on two sequences, secondary lines), and 40 bp nothing maps to"""
    rng = random.Random(101)
    a, b = bases(rng, 12_000), bases(rng, 6_000)
    b = b[:1000] + a[3000:3700] + b[1700:]
    return [a, b, bases(rng, 40)]


@pytest.fixture(scope="module")
def index(engine, ref):
    ix = engine.build_index(ref, k=12)
    yield ix
    ix.free()


def name_of(rng, t, tag="r"):
    """a QNAME of 1 to 40 bytes, distinct per t"""
    base = "%s%d" % (tag, t)
    return base + "x" * rng.randrange(0, 41 - len(base))


def mapped_read(rng, ref, m):
    s = ref[rng.randrange(2)]
    a = rng.randrange(len(s) - m)
    q = mutate(rng, s[a:a + m], rng.randint(0, E))
    return revcomp(q) if rng.random() < 0.5 else q


def euler_residues():
    """256 residues mod 16 such that a run of lines with these lengths mod 16, laid back to back from any offset, puts every
    residue at every offset mod 16: the labels of an Euler circuit of the graph on Z16 with the 16 edges a -> a + r at every a"""
    left = {a: list(range(16)) for a in range(16)}
    stack, circuit = [(0, None)], []
    while stack:
        a, r = stack[-1]
        if left[a]:
            step = left[a].pop()
            stack.append(((a + step) % 16, step))
        else:
            circuit.append(r)
            stack.pop()
    return [r for r in reversed(circuit) if r is not None]


def single_records(ref, seed=7, n_mapped=420, n_dup=30, junk=True):
    """(header, seq, qual): reads of 30-511 bp from both long sequences, exact duplicates under distinct names (equal keys), and
    unmappable reads at the end whose line lengths walk through every (offset, length) residue pair"""
    rng = random.Random(seed)
    recs = []
    lengths = [30, 40, 63, 64, 65, 100, 127, 150, 200, 255, 256, 300, 400, 511]
    for t in range(n_mapped):
        q = mapped_read(rng, ref, lengths[t % len(lengths)])
        recs.append((name_of(rng, t), q, quals(rng, len(q))))
    for t in range(n_mapped // 20):  # from the segment both sequences hold: a hit on each, so secondary lines with all hits
        a = 3000 + rng.randrange(600)
        recs.insert(rng.randrange(len(recs)), (name_of(rng, t, "seg"), ref[0][a:a + 100], quals(rng, 100)))
    for t in range(n_dup):
        q = mapped_read(rng, ref, rng.choice([80, 150, 301]))
        ql = quals(rng, len(q))
        recs.append((name_of(rng, t, "dupa"), q, ql))
        recs.insert(rng.randrange(len(recs)), (name_of(rng, t, "dupb"), q, ql))
    if junk:
        # the unmapped line is QNAME + 19 bytes + SEQ + QUAL; its length mod 16 is set through the name.  They end the file, so
        # they end the sorted file too, back to back and in this order (every '*' line before them comes before them)
        for t, r in enumerate(euler_residues()):
            m = rng.randrange(60, 200)
            base = "j%d" % t
            pad = (r - (len(base) + 19 + 2 * m)) % 16
            recs.append((base + "y" * pad, bases(rng, m), quals(rng, m)))
    return recs


def key_of(line):
    cols = line.split("\t")
    return (len(NAMES) if cols[2] == "*" else NAMES.index(cols[2]), int(cols[3]))


def lines_of(data: bytes):
    text = data.decode("latin-1")
    assert text == "" or text.endswith("\n")
    return text.split("\n")[:-1]


def py_sorted(unsorted: bytes) -> bytes:
    """the oracle: Python's stable sort of the unsorted call's lines"""
    return "".join(ln + "\n" for ln in sorted(lines_of(unsorted), key=key_of)).encode("latin-1")


def check_preconditions(unsorted: bytes, paired=False):
    """on the unsorted output, so that a sorted file cannot be right vacuously"""
    lines = lines_of(unsorted)
    keys = [key_of(ln) for ln in lines]
    assert keys != sorted(keys), "the input is in coordinate order already"
    assert len({k[0] for k in keys if k[0] < len(NAMES)}) >= 2, "hits on fewer than 2 sequences"
    groups = {}
    for k in keys:
        groups[k] = groups.get(k, 0) + 1
    assert sum(1 for k, c in groups.items() if c >= 2 and k[0] < len(NAMES)) >= 20, "fewer than 20 groups of equal keys"
    assert sum(1 for k in keys if k[0] == len(NAMES)) >= 10, "fewer than 10 lines with RNAME '*'"
    if paired:
        flags = [(int(ln.split("\t")[1]), ln.split("\t")[2]) for ln in lines]
        assert sum(1 for f, rn in flags if f & 4 and not f & 8 and rn != "*") >= 5, "fewer than 5 unmapped mates that borrow a position"
        assert sum(1 for f, rn in flags if f & 4 and f & 8 and f & 64) >= 5, "fewer than 5 pairs with both mates unmapped"


def run_single(engine, index, tmp_path, fq, tag, sort, **kw):
    sam = tmp_path / (tag + ".sam")
    st = engine.map_file(index, NAMES, str(fq), str(sam), E, header=HEADER, sort=sort, **kw)
    data = open(sam, "rb").read()
    assert data.startswith(HEADER.encode())
    return data[len(HEADER):], st


@pytest.fixture(scope="module")
def single(engine, ref, index, tmp_path_factory):
    """the single-end input and, once, its unsorted best-hit lines"""
    d = tmp_path_factory.mktemp("single")
    recs = single_records(ref)
    fq = d / "r.fq"
    write_fastq(fq, recs)
    unsorted, st = run_single(engine, index, d, fq, "unsorted", False)
    return dict(recs=recs, fq=fq, unsorted=unsorted, want=py_sorted(unsorted), stats=st)


# ---- permutation and order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["best", "all"])
def test_single_end_sorted_is_the_python_sort_of_unsorted(engine, index, tmp_path, single, mode):
    kw = dict(max_hits=4, strata=1) if mode == "all" else {}
    unsorted = single["unsorted"] if mode == "best" else run_single(engine, index, tmp_path, single["fq"], "u", False, **kw)[0]
    check_preconditions(unsorted)
    if mode == "all":
        assert sum(1 for ln in lines_of(unsorted) if int(ln.split("\t")[1]) & 256) >= 10  # secondary lines, each under its own key
    got, st = run_single(engine, index, tmp_path, single["fq"], "s", True, **kw)
    assert got == py_sorted(unsorted)
    # the stats: the unsorted call's, and the sort's
    assert st["records"] == len(lines_of(unsorted)) and st["bytes_out"] == len(unsorted) and st["reads"] == len(single["recs"])
    assert st["sort"]["lines"] == st["records"] and st["sort"]["bytes_held"] == st["bytes_out"]
    assert st["sort"]["slabs"] >= 1 and st["sort"]["seconds_sort"] > 0


def pair_records(ref, seed=13):
    rng = random.Random(seed)
    r1, r2 = [], []

    def fragment():
        s = ref[rng.randrange(2)]
        length = rng.randrange(INSERT[0] + 60, INSERT[1] - 20)
        a = rng.randrange(len(s) - length)
        f = s[a:a + length]
        if rng.random() < 0.5:
            f = revcomp(f)
        m1, m2 = rng.randrange(50, 151), rng.randrange(50, 151)
        return mutate(rng, f[:m1], rng.randint(0, E)), mutate(rng, revcomp(f[-m2:]), rng.randint(0, E))

    def add(name, q1, q2, at=None):
        at = len(r1) if at is None else at
        r1.insert(at, (name + "/1 first mate", q1, quals(rng, len(q1))))
        r2.insert(at, (name + "/2", q2, quals(rng, len(q2))))

    for t in range(220):
        add(name_of(rng, t, "f"), *fragment())
    for t in range(25):  # exact duplicate fragments under distinct names
        q1, q2 = fragment()
        add(name_of(rng, t, "da"), q1, q2)
        add(name_of(rng, t, "db"), q1, q2, rng.randrange(len(r1)))
    for t in range(12):  # one mate of random bases: unmapped, and nothing to rescue; it borrows its mate's RNAME and POS
        q1, q2 = fragment()
        junk = bases(rng, rng.randrange(80, 150))
        add(name_of(rng, t, "h"), *((q1, junk) if t % 2 else (junk, q2)), rng.randrange(len(r1)))
    for t in range(12):  # both mates of random bases
        add(name_of(rng, t, "n"), bases(rng, 100), bases(rng, 120), rng.randrange(len(r1)))
    return r1, r2


def run_pairs(engine, index, tmp_path, f1, f2, tag, sort, **kw):
    sam = tmp_path / (tag + ".sam")
    st = engine.map_pairs_file(index, NAMES, str(f1), str(f2), str(sam), E, INSERT[0], INSERT[1], rescue_errors=4, header=HEADER, sort=sort, **kw)
    data = open(sam, "rb").read()
    assert data.startswith(HEADER.encode())
    return data[len(HEADER):], st


def test_paired_sorted_is_the_python_sort_of_unsorted(engine, ref, index, tmp_path):
    r1, r2 = pair_records(ref)
    f1, f2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    write_fastq(f1, r1)
    write_fastq(f2, r2)
    unsorted, st0 = run_pairs(engine, index, tmp_path, f1, f2, "u", False)
    check_preconditions(unsorted, paired=True)
    assert st0["rescued"] >= 0 and st0["proper"] >= 100
    for chunk_bytes in (0, 2048):
        got, st = run_pairs(engine, index, tmp_path, f1, f2, "s%d" % chunk_bytes, True, chunk_bytes=chunk_bytes)
        assert got == py_sorted(unsorted), chunk_bytes
        assert st["pairs"] == len(r1) and st["proper"] == st0["proper"] and st["rescued"] == st0["rescued"]
        assert st["sort"]["lines"] == st["records"] == 2 * len(r1) and st["sort"]["bytes_held"] == st["bytes_out"] == len(unsorted)
    assert st["chunks"] >= 3 and st["sort"]["slabs"] >= 3


# ---- copy edges ---------------------------------------------------------------------------------------------------------------------------
def test_copy_edges_and_a_line_longer_than_the_slab(engine, ref, index, tmp_path):
    recs = single_records(ref, seed=19, n_mapped=200, n_dup=0)
    rng = random.Random(23)
    src = ref[0][5000:5511]
    recs.insert(len(recs) // 2, ("L" * 200, src, quals(rng, 511)))  # a 511 bp read under a 200-byte name: more than 1024 bytes of SAM
    recs.insert(3, ("q", ref[1][4000:4090], quals(rng, 90)))  # and the shortest name
    fq = tmp_path / "r.fq"
    write_fastq(fq, recs)
    unsorted, _ = run_single(engine, index, tmp_path, fq, "u", False)
    got, st = run_single(engine, index, tmp_path, fq, "s", True, chunk_bytes=1024)
    assert got == py_sorted(unsorted)
    lines = lines_of(got)
    assert max(len(ln) + 1 for ln in lines) > 1024 and st["sort"]["slabs"] >= 3
    # every destination alignment together with every length mod 16, in the run that writes one slab: the slab buffer starts
    # aligned, so a line's destination alignment is its offset in the file's body
    got0, st0 = run_single(engine, index, tmp_path, fq, "s0", True)
    assert got0 == got and st0["sort"]["slabs"] == 1
    assert len({len(ln.split("\t")[0]) for ln in lines}) >= 30 and min(len(ln.split("\t")[0]) for ln in lines) == 1
    seen, at = set(), 0
    for ln in lines:
        seen.add((at % 16, (len(ln) + 1) % 16))
        at += len(ln) + 1
    assert len(seen) == 256, sorted(set((a, r) for a in range(16) for r in range(16)) - seen)


# ---- chunk and slab independence ---------------------------------------------------------------------------------------------------------
def test_chunks_and_slabs_do_not_change_the_output(asm, engine, ref, index, tmp_path, single, monkeypatch):
    want = single["want"]
    for chunk_bytes in (1024, 4096, 0):
        got, st = run_single(engine, index, tmp_path, single["fq"], "c%d" % chunk_bytes, True, chunk_bytes=chunk_bytes)
        assert got == want, chunk_bytes
        if chunk_bytes:
            assert st["chunks"] >= 3 and st["sort"]["slabs"] >= 3
            assert st["sort"]["slabs"] >= len(want) // chunk_bytes
    monkeypatch.setenv("ASM_MAP_CHUNK", "7")  # several device chunks per file chunk: a fresh engine reads it
    eng2 = asm.Engine(0)
    try:
        ix2 = eng2.build_index(ref, k=12)
        for chunk_bytes in (0, 4096):
            got, st = run_single(eng2, ix2, tmp_path, single["fq"], "m%d" % chunk_bytes, True, chunk_bytes=chunk_bytes)
            assert got == want, chunk_bytes
            assert st["chunks"] >= (len(single["recs"]) + 6) // 7
        ix2.free()
    finally:
        eng2.close()
        monkeypatch.delenv("ASM_MAP_CHUNK")


# ---- degenerate inputs ----------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(engine, ref, index, tmp_path):
    fq = tmp_path / "empty.fq"
    fq.write_bytes(b"")
    got, st = run_single(engine, index, tmp_path, fq, "empty", True)
    assert got == b"" and st["records"] == st["sort"]["lines"] == st["sort"]["slabs"] == st["sort"]["bytes_held"] == 0
    f2 = tmp_path / "empty2.fq"
    f2.write_bytes(b"")
    got, st = run_pairs(engine, index, tmp_path, fq, f2, "emptyp", True)
    assert got == b"" and st["records"] == st["sort"]["lines"] == 0
    # only unmappable reads: every key is the same, so the order is the file's
    rng = random.Random(3)
    recs = [("u%d" % t, bases(rng, 70 + t), quals(rng, 70 + t)) for t in range(40)]
    fq = tmp_path / "junk.fq"
    write_fastq(fq, recs)
    unsorted, _ = run_single(engine, index, tmp_path, fq, "ju", False)
    assert all(ln.split("\t")[2] == "*" for ln in lines_of(unsorted)) and len(lines_of(unsorted)) == 40
    for chunk_bytes in (0, 1024):
        got, st = run_single(engine, index, tmp_path, fq, "js", True, chunk_bytes=chunk_bytes)
        assert got == unsorted
    # one read
    fq = tmp_path / "one.fq"
    write_fastq(fq, [("only", ref[1][200:300], quals(rng, 100))])
    unsorted, _ = run_single(engine, index, tmp_path, fq, "ou", False)
    got, st = run_single(engine, index, tmp_path, fq, "os", True)
    assert got == unsorted and st["sort"]["lines"] == 1 and st["sort"]["slabs"] == 1 and st["mapped"] == 1


# ---- the memory cap ---------------------------------------------------------------------------------------------------------------------------
def test_memory_cap_is_an_error_and_the_handle_stays_usable(asm, engine, index, tmp_path, single):
    assert len(single["unsorted"]) > 100_000
    for kw in (dict(), dict(chunk_bytes=4096)):
        with pytest.raises(asm.AsmError) as exc:
            run_single(engine, index, tmp_path, single["fq"], "cap", True, max_device_bytes=4096, **kw)
        assert exc.value.code == -3  # ASM_ENOMEM
        text = str(exc.value)
        assert "asm_map_file_sorted: sorted output keeps the whole SAM text on the device: " in text
        assert " bytes reached (max_device_bytes = 4096)" in text
        reached = int(text.split("on the device: ")[1].split(" ")[0])
        assert reached > 4096
    got, _ = run_single(engine, index, tmp_path, single["fq"], "after_u", False)
    assert got == single["unsorted"]
    got, _ = run_single(engine, index, tmp_path, single["fq"], "after_s", True, max_device_bytes=0)
    assert got == single["want"]
    # a cap that is large enough is no error
    got, st = run_single(engine, index, tmp_path, single["fq"], "roomy", True, max_device_bytes=64 << 20)
    assert got == single["want"]
    with pytest.raises(asm.AsmError) as exc:
        run_single(engine, index, tmp_path, single["fq"], "neg", True, max_device_bytes=-1)
    assert exc.value.code == -1 and "max_device_bytes must be >= 0" in str(exc.value)


def test_input_error_comes_before_any_sorted_byte(asm, engine, index, tmp_path, single):
    data = open(single["fq"], "rb").read().decode("latin-1").split("\n")
    data[4 * 300] = "x" + data[4 * 300][1:]  # record 301 loses its '@'
    fq = tmp_path / "bad.fq"
    fq.write_bytes("\n".join(data).encode("latin-1"))
    for kw in (dict(), dict(chunk_bytes=4096)):
        sam = tmp_path / "bad.sam"
        with pytest.raises(asm.AsmError) as exc:
            engine.map_file(index, NAMES, str(fq), str(sam), E, header=HEADER, sort=True, **kw)
        assert exc.value.code == -1 and "asm_map_file_sorted: record 301 is malformed" in str(exc.value)
        assert open(sam, "rb").read() == HEADER.encode()  # the 300 good records in front of it were held, not written


# ---- the tool -------------------------------------------------------------------------------------------------------------------------------
def run_tool(args, sam):
    r = subprocess.run([EXE] + [str(a) for a in args] + ["-o", str(sam)], capture_output=True, text=True, timeout=LIMIT)
    assert r.returncode == 0, r.stderr[-2000:]
    return lines_of(open(sam, "rb").read()), r.stderr


def same_but_for_the_command_line(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x.startswith("@PG"):
            assert y.startswith("@PG") and x.split("\tCL:")[0] == y.split("\tCL:")[0]
        else:
            assert x == y


@pytest.mark.parametrize("flags", [["--both-strands"], ["--both-strands", "--all-hits", "4", "--strata", "1"]])
def test_tool_sorts_the_same_on_the_device_and_on_the_host(engine, ref, index, tmp_path, single, flags):
    assert os.path.exists(EXE), "asm-map is built by build()"
    fa = tmp_path / "ref.fa"
    write_reference(fa, ref)
    base = ["-r", fa, "-q", single["fq"], "-e", E] + flags
    host, _ = run_tool(base + ["--sort"], tmp_path / "host.sam")
    streamed, err = run_tool(base + ["--stream", "--sort", "--chunk-bytes", "4096"], tmp_path / "dev.sam")
    assert host[0] == streamed[0] == "@HD\tVN:1.6\tSO:coordinate"
    same_but_for_the_command_line(host, streamed)
    body = [ln for ln in host if not ln.startswith("@")]
    assert [key_of(ln) for ln in body] == sorted(key_of(ln) for ln in body) and len(body) >= len(single["recs"])
    assert "asm-map: sorted %d lines" % len(body) in err
    if len(flags) == 1:
        # without --sort nothing changes: the unsorted library call's lines under the unsorted header
        assert "".join(ln + "\n" for ln in body).encode("latin-1") == single["want"]
        plain, _ = run_tool(base + ["--stream"], tmp_path / "plain.sam")
        assert plain[0] == "@HD\tVN:1.6\tSO:unsorted"
        assert "".join(ln + "\n" for ln in plain if not ln.startswith("@")).encode("latin-1") == single["unsorted"]


def test_paired_tool_sorts_the_same_on_the_device_and_on_the_host(engine, ref, index, tmp_path):
    r1, r2 = pair_records(ref, seed=17)
    fa, f1, f2 = tmp_path / "ref.fa", tmp_path / "r1.fq", tmp_path / "r2.fq"
    write_reference(fa, ref)
    write_fastq(f1, r1)
    write_fastq(f2, r2)
    base = ["-r", fa, "-1", f1, "-2", f2, "-e", E, "--insert", "%d,%d" % INSERT, "--rescue", "4"]
    host, _ = run_tool(base + ["--sort"], tmp_path / "host.sam")
    streamed, _ = run_tool(base + ["--stream-pairs", "--sort", "--sort-mem", str(64 << 20)], tmp_path / "dev.sam")
    assert host[0] == streamed[0] == "@HD\tVN:1.6\tSO:coordinate"
    same_but_for_the_command_line(host, streamed)
    body = [ln for ln in host if not ln.startswith("@")]
    assert len(body) == 2 * len(r1) and [key_of(ln) for ln in body] == sorted(key_of(ln) for ln in body)
    unsorted, _ = run_pairs(engine, index, tmp_path, f1, f2, "lib", False)
    assert "".join(ln + "\n" for ln in body).encode("latin-1") == py_sorted(unsorted)
    r = subprocess.run([EXE] + [str(a) for a in base] + ["--sort-mem", "4096", "-o", str(tmp_path / "x.sam")], capture_output=True, text=True,
                       timeout=LIMIT)
    assert r.returncode == 2 and "usage" in r.stderr  # --sort-mem belongs to the device-side sort
