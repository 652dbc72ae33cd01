"""The device-free side of the sorted file calls (docs/design/mapper.md, "Sorted output"): sam_sort_key against the key a parser
written here reads from the line sam_format writes, the slab cutter against its four properties, the per-lane copy of
sam_line_gather_kernel at every alignment, all three from host/sort_host_check.cpp built under ASan + UBSan and run as a program;
and the argument checks of asm_map_file_sorted and asm_map_pairs_file_sorted with a NULL handle, which must be the unsorted calls'
under the sorted calls' names."""
import ctypes
import json
import os
import random
import struct
import subprocess

import pytest

from tests.test_map_file_host import GOLDEN, PKG, pack_case, san_flags

NAMES = ["chrA", "chr" + "B" * 70, "c", "chrD"]  # n_seqs = 4: tid takes three bits, '*' sorts as 4


@pytest.fixture(scope="module")
def sort_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sort_check") / "sort_host_check_asan")
    src = os.path.join(PKG, "host", "sort_host_check.cpp")
    assert os.path.exists(src), "host/sort_host_check.cpp: the host build of the sort key, the slab cutter and the line copy"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_clean(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


# ---- the key equals the text -------------------------------------------------------------------------------------------------------
def make_key_cases(seed=29):
    """SamLine cases shaped like make_cases of tests/test_map_file_host.py and make_pair_cases of tests/test_map_pairs_file_host.py:
    single and paired; own, lent and unmapped; ranks; the first and the last sequence; POS 0 and 2^32 - 2"""
    rng = random.Random(seed)
    positions = [0, 8, 9, 99, 100, 12345, 999_999_999, 2**31 - 1, 2**31, 2**32 - 2]
    cases = []

    def case(**kw):
        m = kw.pop("m", rng.choice([1, 40, 64, 65, 300, 511]))
        c = dict(name="q%d" % rng.randrange(10**rng.randrange(1, 9)), seq="".join(rng.choice("ACGTNacgt") for _ in range(m)),
                 qual="".join(chr(rng.randrange(33, 127)) for _ in range(m)), mapped=1, seq_id=rng.randrange(len(NAMES)),
                 pos=rng.choice(positions), dist=rng.randrange(16), cost=rng.randrange(0, 301), strand=rng.randrange(2), rank=0, all=0,
                 nrep=1, nh=1, nops=rng.choice([1, 3, 31, 64, 65]), paired=0, mate=rng.randrange(2), proper=0, rescued=0, mate_mapped=0,
                 mate_seq_id=rng.randrange(len(NAMES)), mate_pos=rng.choice(positions), mate_strand=rng.randrange(2), tlen=0, n_concordant=0)
        c.update(kw)
        if c["all"]:
            c["nrep"], c["nh"] = max(c["nrep"], c["rank"] + 1), max(c["nh"], c["rank"] + 1)
        else:
            c["rank"] = 0
        c["rname"], c["mate_rname"] = NAMES[c["seq_id"]], NAMES[c["mate_seq_id"]]
        c["ops"] = [(rng.choice([1, 9, 10, 100, 511]) << 3) | rng.randrange(5) for _ in range(min(c["nops"], 64))]
        cases.append(c)

    for sid in (0, len(NAMES) - 1):
        for pos in positions:
            case(seq_id=sid, pos=pos)  # single-end, own
            case(seq_id=sid, pos=pos, all=1, rank=rng.choice([1, 9, 255]))  # a secondary line: its own key
            for mate in (0, 1):
                case(paired=1, mate=mate, seq_id=sid, pos=pos, mate_mapped=1)  # paired, own, the mate elsewhere
                case(paired=1, mate=mate, seq_id=sid, pos=pos, mate_mapped=0)  # paired, own, the mate unmapped
                case(paired=1, mate=mate, mapped=0, mate_mapped=1, mate_seq_id=sid, mate_pos=pos)  # lent: the mate's RNAME and POS
    for mate in (0, 1):
        for m in (0, 5, 600):
            case(paired=1, mate=mate, mapped=0, mate_mapped=0, m=m)  # both unmapped: '*'
    for m in (0, 5, 600):
        case(mapped=0, m=m)  # single-end unmapped: '*', whatever the hit fields hold
    case(mapped=0, mate_mapped=1, mate_seq_id=0, mate_pos=77)  # single-end lines never borrow
    for _ in range(300):
        case(paired=rng.randrange(2), mapped=int(rng.random() < 0.7), mate_mapped=int(rng.random() < 0.7), all=rng.randrange(2),
             rank=rng.choice([0, 0, 1, 7]))
    for c in cases:
        if c["paired"]:
            c["all"], c["rank"] = 0, 0  # the file calls write no secondary pairs
    return rng, cases


def pack_key_case(rng, c):
    rn = c["mate_rname"].encode()
    out = pack_case(rng, c)
    out += struct.pack("<IIIIIiIIII", c["paired"], c["mate"], c["proper"], c["rescued"], c["mate_mapped"], c["mate_seq_id"], c["mate_pos"],
                       c["mate_strand"], c["tlen"], c["n_concordant"])
    return out + struct.pack("<I", len(rn)) + rn


def key_of_line(line: bytes) -> int:
    """what a consumer of the SAM text sorts by"""
    cols = line.decode("latin-1").split("\t")
    tid = len(NAMES) if cols[2] == "*" else NAMES.index(cols[2])
    return tid << 32 | int(cols[3])


def test_sort_key_equals_the_key_read_from_the_text(sort_check, tmp_path):
    rng, cases = make_key_cases()
    fin, fout = tmp_path / "cases.bin", tmp_path / "keys.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<II", len(cases), len(NAMES)))
        for c in cases:
            fh.write(pack_key_case(rng, c))
    run_clean([sort_check, "keys", str(fin), str(fout)])
    data = open(fout, "rb").read()
    at, seen, keys = 0, set(), set()
    for t, c in enumerate(cases):
        key, size = struct.unpack_from("<QQ", data, at)
        keys.add(key)
        line = data[at + 16:at + 16 + size]
        at += 16 + size
        assert line.endswith(b"\n") and line.count(b"\n") == 1, (t, c)
        assert key == key_of_line(line), (t, c, key, line)
        own, lent = bool(c["mapped"]), bool(c["paired"] and not c["mapped"] and c["mate_mapped"])
        want = (c["seq_id"] << 32 | c["pos"] + 1) if own else (c["mate_seq_id"] << 32 | c["mate_pos"] + 1) if lent else len(NAMES) << 32
        assert key == want, (t, c)
        seen.add(("pair" if c["paired"] else "single", "own" if own else "lent" if lent else "none"))
    assert at == len(data)
    assert seen == {("single", "own"), ("single", "none"), ("pair", "own"), ("pair", "lent"), ("pair", "none")}
    # the corners of the key: the first sequence at POS 1, the last one at POS 2^32 - 1, and '*'
    assert {1, (len(NAMES) - 1) << 32 | (2**32 - 1), len(NAMES) << 32} <= keys


# ---- the slab cutter ------------------------------------------------------------------------------------------------------------------
def slab_lists(seed=31):
    rng = random.Random(seed)
    lists = [(1024, []), (1024, [1] * 5000), (1, [1] * 50), (1024, [1024]), (1024, [1025]), (1024, [200, 1024, 200]),
             (1024, [500, 524, 1, 5000, 1023, 1, 1]), (1024, [1024] * 7), (16 << 20, [300] * 2000), (1024, [2000, 3000, 4000])]
    for _ in range(60):
        cap = rng.choice([64, 1000, 1024, 4096, 70000])
        n = rng.randrange(0, 400)
        sizes = [rng.choice([1, rng.randrange(1, 60), rng.randrange(200, 700), rng.randrange(700, 1300)]) for _ in range(n)]
        for _ in range(rng.randrange(0, 3)):
            if sizes:
                sizes[rng.randrange(n)] = rng.choice([cap, cap + 1, cap - 1, 3 * cap])  # a line of exactly the cap, and longer ones
        lists.append((cap, sizes))
    return lists


def test_slab_cutter(sort_check, tmp_path):
    lists = slab_lists()
    fin, fout = tmp_path / "lists.bin", tmp_path / "cuts.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(lists)))
        for cap, sizes in lists:
            fh.write(struct.pack("<QQ", cap, len(sizes)) + struct.pack("<%dQ" % len(sizes), *sizes))
    run_clean([sort_check, "slabs", str(fin), str(fout)])
    data = open(fout, "rb").read()
    at = 0
    for t, (cap, sizes) in enumerate(lists):
        (k,) = struct.unpack_from("<Q", data, at)
        cuts = list(struct.unpack_from("<%dQ" % k, data, at + 8))
        at += 8 + 8 * k
        # contiguous, cut at line boundaries only, covering everything: line indices from 0 to n, strictly ascending
        assert cuts[0] == 0 and cuts[-1] == len(sizes), (t, cuts)
        assert all(a < b for a, b in zip(cuts, cuts[1:])), (t, cuts)
        for a, b in zip(cuts, cuts[1:]):
            total = sum(sizes[a:b])
            assert total <= cap or b - a == 1, (t, a, b, total, cap)  # at most max(cap, its single line)
            if b < len(sizes):
                assert total + sizes[b] > cap, (t, a, b)  # and no shorter than it has to be
        if not sizes:
            assert cuts == [0]
    assert at == len(data)


def test_line_copy_at_every_alignment(sort_check):
    r = run_clean([sort_check, "gather"])
    assert r.stdout.startswith("gather ok ")


# ---- rejections -------------------------------------------------------------------------------------------------------------------------
def sorted_rejection_cases(asm, max_device_bytes=0):
    """rejection_cases of tests/test_map_file_host.py through asm_map_file_sorted"""
    lib = asm.load_library()
    MP = asm.MapParams
    dummy = ctypes.create_string_buffer(64)
    names = (ctypes.c_char_p * 1)(b"chr1")
    base = dict(ix=dummy, names=names, fastq=b"reads.fq", sam=b"out.sam", p=MP(2, 1, 0, 3), max_hits=0, strata=0, chunk_bytes=0)
    out = []

    def add(label, **kw):
        a = dict(base, **kw)
        p = None if a["p"] is None else ctypes.byref(a["p"])
        out.append((label, lambda: lib.asm_map_file_sorted(None, a["ix"], a["names"], a["fastq"], a["sam"], None, p, a["max_hits"],
                                                           a["strata"], a["chunk_bytes"], max_device_bytes, None, None)))

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


def test_sorted_call_rejects_what_the_unsorted_call_rejects(asm):
    lib = asm.load_library()
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = [[label, int(thunk()), lib.asm_last_error(None).decode()] for label, thunk in sorted_rejection_cases(asm)]
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert w[2].startswith("asm_map_file: ")
        assert g[1] == w[1] and g[2] == "asm_map_file_sorted: " + w[2][len("asm_map_file: "):], (g, w)
    assert not os.path.exists("out.sam")


def test_negative_max_device_bytes(asm):
    lib = asm.load_library()
    for label, thunk in sorted_rejection_cases(asm, max_device_bytes=-1):
        if label.startswith("no handle"):  # everything else about the call is good
            assert int(thunk()) == -1  # ASM_EINVAL
            assert lib.asm_last_error(None).decode() == "asm_map_file_sorted: max_device_bytes must be >= 0"
    MP, PP = asm.MapParams, asm.PairParams
    p, pp = MP(2, 1, 0, 3), PP(100, 500, -1)
    names = (ctypes.c_char_p * 1)(b"chr1")
    dummy = ctypes.create_string_buffer(64)
    rc = lib.asm_map_pairs_file_sorted(None, dummy, names, b"r1.fq", b"r2.fq", b"out.sam", None, ctypes.byref(p), ctypes.byref(pp), 0, -5, None, None)
    assert int(rc) == -1 and lib.asm_last_error(None).decode() == "asm_map_pairs_file_sorted: max_device_bytes must be >= 0"


def test_sorted_pair_call_rejects_what_the_unsorted_call_rejects(asm):
    """the cases of test_map_pairs_file_rejections (tests/test_map_pairs_file_host.py) through both calls: the same code, and the
    same message under the other name"""
    lib = asm.load_library()
    MP, PP = asm.MapParams, asm.PairParams
    dummy = ctypes.create_string_buffer(64)
    names = (ctypes.c_char_p * 1)(b"chr1")
    base = dict(ix=dummy, names=names, f1=b"r1.fq", f2=b"r2.fq", sam=b"out.sam", p=MP(2, 1, 0, 3), pp=PP(100, 500, -1), chunk_bytes=0)

    def call(sort, **kw):
        a = dict(base, **kw)
        head = (None, a["ix"], a["names"], a["f1"], a["f2"], a["sam"], None, None if a["p"] is None else ctypes.byref(a["p"]),
                None if a["pp"] is None else ctypes.byref(a["pp"]), a["chunk_bytes"])
        rc = lib.asm_map_pairs_file_sorted(*head, 0, None, None) if sort else lib.asm_map_pairs_file(*head, None)
        return int(rc), lib.asm_last_error(None).decode()

    cases = [dict(f1=None), dict(f2=None), dict(sam=None), dict(names=None), dict(p=None), dict(pp=None), dict(ix=None), dict(chunk_bytes=-1),
             dict(p=MP(16, 1, 0, 3)), dict(p=MP(2, 0, 0, 3)), dict(p=MP(2, 1, -1, 3)), dict(p=MP(2, 1, 0, 51)), dict(pp=PP(-1, 500, -1)),
             dict(pp=PP(600, 500, -1)), dict(pp=PP(0, 8193, -1)), dict(pp=PP(100, 500, -2)), dict(pp=PP(100, 500, 16)), dict()]
    for kw in cases:
        code, text = call(False, **kw)
        assert code == -1 and text.startswith("asm_map_pairs_file: "), kw
        assert call(True, **kw) == (code, "asm_map_pairs_file_sorted: " + text[len("asm_map_pairs_file: "):]), kw
    assert not os.path.exists("out.sam")
