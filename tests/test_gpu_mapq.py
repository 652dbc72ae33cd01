"""Mapping quality on the device (docs/design/mapper.md, "Mapping quality"): asm_map_last_mapq and column 5 of the file calls against
the model's Python statement (tests/mapq_cases.py) over brute-force loci, on every record slot of the corpus; the records under
ASM_MAPQ_GAP against model 0's; the default model against an explicit model 0, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import mapq_cases as mq
from tests.test_map_all_host import bf_all, build_bruteforce_all
from tests.test_map_pairs_host import bf_pairs, build_bruteforce_rescue

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
NAMES = ["chrA", "chrB"]
MAX_HITS, MAX_PAIRS = 8, 4
RECORD = ("seq_id", "pos", "end", "dist", "strand", "flags", "greedy_cost", "cigar_nops")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the corpus and, computed once, the brute forces' loci and pair answers of every e"""
    bfa = build_bruteforce_all(tmp_path_factory.mktemp("gmapq_bfa"))
    bfr = build_bruteforce_rescue(tmp_path_factory.mktemp("gmapq_bfr"))
    seqs = mq.reference()
    out = {}
    for e in mq.E_SWEEP:
        rd = [(label, q, bf_all(bfa, seqs, q, e)) for label, q in mq.reads(seqs, e)]
        pr = []
        for label, q1, q2 in mq.pairs(seqs, e):
            loci = [bf_all(bfa, seqs, q1, e), bf_all(bfa, seqs, q2, e)]
            res = bf_pairs(bfa, bfr, seqs, q1, q2, e, *mq.INSERT, rescue=mq.rescue_errors(e), k=8, loci=loci)
            pr.append((label, q1, q2, loci, res, mq.mapq_ref_pair(loci[0], loci[1], len(q1), len(q2), *mq.INSERT, e, res)))
        out[e] = (rd, pr)
    return seqs, out


@pytest.fixture(scope="module")
def engines(asm, world):
    """one engine per model (the third keeps the default) and their indexes per k"""
    seqs, _ = world
    ref, gap, default = asm.Engine(0), asm.Engine(0), asm.Engine(0)
    ref.set_mapq_model("reference")
    gap.set_mapq_model(asm.MAPQ_GAP)
    assert (ref.mapq_model(), gap.mapq_model(), default.mapq_model()) == (0, 1, 0)
    ix = {(name, k): eng.build_index(seqs, k=k) for name, eng in (("ref", ref), ("gap", gap), ("default", default)) for k in mq.K_SWEEP}
    yield {"ref": ref, "gap": gap, "default": default, "ix": ix}
    for x in ix.values():
        x.free()
    for eng in (ref, gap, default):
        eng.close()


def same_records(a, b):
    for name in RECORD:
        assert np.array_equal(a[name], b[name]), name
    assert a["cigar"] == b["cigar"]


def reference_rule(out):
    return np.where((out["flags"] & 1) != 0, np.minimum(254, 60 + out["greedy_cost"].astype(np.int64)), 0).astype(np.uint8)


@pytest.mark.parametrize("k", mq.K_SWEEP)
@pytest.mark.parametrize("e", mq.E_SWEEP)
def test_single_end_calls_equal_the_model_on_every_slot(world, engines, e, k):
    _, out = world
    rd, _ = out[e]
    reads = [q for _, q, _ in rd]
    want = [mq.mapq_ref_read(loci, e) for _, _, loci in rd]
    gap, ref = engines["gap"], engines["ref"]
    g = gap.map_reads(engines["ix"]["gap", k], reads, e)
    slots = gap.last_mapq(len(reads))
    r = ref.map_reads(engines["ix"]["ref", k], reads, e)
    assert np.array_equal(ref.last_mapq(len(reads)), reference_rule(r))
    same_records(g, r)
    assert [int(v) for v in slots] == [w[0] if w else 0 for w in want]
    assert np.array_equal(g["mapping_quality"], slots)
    ga = gap.map_reads_all(engines["ix"]["gap", k], reads, e, max_hits=MAX_HITS)
    slots = gap.last_mapq(len(reads) * MAX_HITS).reshape(len(reads), MAX_HITS)
    ra = ref.map_reads_all(engines["ix"]["ref", k], reads, e, max_hits=MAX_HITS)
    rslots = ref.last_mapq(len(reads) * MAX_HITS).reshape(len(reads), MAX_HITS)
    same_records(ga, ra)
    for i, w in enumerate(want):
        assert [int(v) for v in slots[i]] == (w + [0] * MAX_HITS)[:MAX_HITS], (i, rd[i][0])
    assert np.array_equal(ga["mapping_quality"], slots[ga["read"], ga["rank"]])
    assert np.array_equal(ra["mapping_quality"], np.minimum(254, 60 + ra["greedy_cost"]).astype(np.uint8))
    assert int(rslots.sum()) == int(ra["mapping_quality"].astype(np.int64).sum())  # unused slots: 0
    # rank 0 of the all-hits answer is the best hit under either model
    first = np.cumsum(ga["n_reported"]) - ga["n_reported"]
    hit = ga["n_reported"] > 0
    assert np.array_equal(ga["pos"][first[hit]], g["pos"][hit]) and np.array_equal(ga["mapping_quality"][first[hit]], g["mapping_quality"][hit])


@pytest.mark.parametrize("k", mq.K_SWEEP)
@pytest.mark.parametrize("e", mq.E_SWEEP)
def test_paired_calls_equal_the_model_on_every_slot(world, engines, e, k):
    _, out = world
    _, pr = out[e]
    r1, r2 = [p[1] for p in pr], [p[2] for p in pr]
    gap, ref = engines["gap"], engines["ref"]
    kw = dict(rescue_errors=mq.rescue_errors(e))
    g = gap.map_pairs(engines["ix"]["gap", k], r1, r2, e, *mq.INSERT, **kw)
    slots = gap.last_mapq(2 * len(pr)).reshape(len(pr), 2)
    r = ref.map_pairs(engines["ix"]["ref", k], r1, r2, e, *mq.INSERT, **kw)
    assert np.array_equal(ref.last_mapq(2 * len(pr)).reshape(len(pr), 2), reference_rule(r))
    same_records(g, r)
    for t, p in enumerate(pr):
        assert tuple(int(v) for v in slots[t]) == tuple(p[5]["primary"]), (t, p[0])
        assert bool(g["rescued"][t].any()) == (p[4]["rescued"] is not None)
    assert np.array_equal(g["mapping_quality"], slots)
    ga = gap.map_pairs_all(engines["ix"]["gap", k], r1, r2, e, *mq.INSERT, max_pairs=MAX_PAIRS, **kw)
    slots = gap.last_mapq(2 * len(pr) * MAX_PAIRS).reshape(len(pr), MAX_PAIRS, 2)
    ra = ref.map_pairs_all(engines["ix"]["ref", k], r1, r2, e, *mq.INSERT, max_pairs=MAX_PAIRS, **kw)
    assert np.array_equal(ref.last_mapq(2 * len(pr) * MAX_PAIRS).reshape(len(pr), MAX_PAIRS, 2), reference_rule(ra))
    same_records(ga, ra)
    for t, p in enumerate(pr):
        want = [list(x[2]) for x in p[5]["pairs"]][:MAX_PAIRS] or [list(p[5]["primary"])]
        want += [[0, 0]] * (MAX_PAIRS - len(want))
        assert slots[t].tolist() == want, (t, p[0])
    assert np.array_equal(ga["mapping_quality"], slots)


@pytest.mark.parametrize("strata, max_hits", [(0, MAX_HITS), (1, MAX_HITS), (4, 2), (0, 1)])
def test_the_fold_sees_every_locus_whatever_becomes_an_item(world, engines, strata, max_hits):
    """strata below max_errors, or max_hits below the loci tied at d1, shorten the item list only: d2 and n1 still come from every
    locus within e (the near1 / near2 families need the locus above d1, the five-copy family all five ties)"""
    _, out = world
    e, k = 4, 12
    rd, _ = out[e]
    reads = [q for _, q, _ in rd]
    gap = engines["gap"]
    ga = gap.map_reads_all(engines["ix"]["gap", k], reads, e, max_hits=max_hits, strata=strata)
    slots = gap.last_mapq(len(reads) * max_hits).reshape(len(reads), max_hits)
    shortened = 0
    for i, (_, _, loci) in enumerate(rd):
        full = mq.mapq_ref_read(loci, e)
        d1 = min([l[4] for l in loci], default=0)
        kept = [v for v, l in zip(full, loci) if l[4] <= d1 + strata][:max_hits]
        shortened += len(kept) < len(full)
        assert [int(v) for v in slots[i]] == kept + [0] * (max_hits - len(kept)), (i, rd[i][0])
    assert shortened >= 4
    assert np.array_equal(ga["mapping_quality"], slots[ga["read"], ga["rank"]])


def test_results_do_not_depend_on_the_device_chunk(asm, world, engines, monkeypatch):
    seqs, out = world
    e, k = 2, 12
    rd, pr = out[e]
    reads, r1, r2 = [q for _, q, _ in rd], [p[1] for p in pr], [p[2] for p in pr]
    monkeypatch.setenv("ASM_MAP_CHUNK", "16")
    small = asm.Engine(0)
    monkeypatch.delenv("ASM_MAP_CHUNK")
    try:
        small.set_mapq_model("gap")
        ix = small.build_index(seqs, k=k)
        big, bix = engines["gap"], engines["ix"]["gap", k]
        kw = dict(rescue_errors=mq.rescue_errors(e))
        for a, b in ((small.map_reads(ix, reads, e), big.map_reads(bix, reads, e)),
                     (small.map_reads_all(ix, reads, e, max_hits=MAX_HITS), big.map_reads_all(bix, reads, e, max_hits=MAX_HITS)),
                     (small.map_pairs(ix, r1, r2, e, *mq.INSERT, **kw), big.map_pairs(bix, r1, r2, e, *mq.INSERT, **kw)),
                     (small.map_pairs_all(ix, r1, r2, e, *mq.INSERT, max_pairs=MAX_PAIRS, **kw),
                      big.map_pairs_all(bix, r1, r2, e, *mq.INSERT, max_pairs=MAX_PAIRS, **kw))):
            same_records(a, b)
            assert np.array_equal(a["mapping_quality"], b["mapping_quality"])
        ix.free()
    finally:
        small.close()


def body(path):
    with open(path, "rb") as fh:
        return [l for l in fh.read().split(b"\n") if l and not l.startswith(b"@")]


def write_inputs(tmp, seqs, rd, pr):
    fa, fq, f1, f2 = (tmp / n for n in ("ref.fa", "reads.fq", "r1.fq", "r2.fq"))
    fa.write_text("".join(">%s\n%s\n" % (NAMES[r], s) for r, s in enumerate(seqs)))
    fq.write_text("".join("@r%d_%s\n%s\n+\n%s\n" % (t, label, q, "I" * len(q)) for t, (label, q, _) in enumerate(rd)))
    f1.write_text("".join("@p%d_%s/1\n%s\n+\n%s\n" % (t, p[0], p[1], "I" * len(p[1])) for t, p in enumerate(pr)))
    f2.write_text("".join("@p%d_%s/2\n%s\n+\n%s\n" % (t, p[0], p[2], "I" * len(p[2])) for t, p in enumerate(pr)))
    return fa, fq, f1, f2


def tool(args, out):
    r = subprocess.run([EXE] + [str(a) for a in args] + ["-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return body(out)


def test_file_calls_equal_the_tool_and_the_model(world, engines, tmp_path):
    seqs, out = world
    e, k = 2, 12
    rd, pr = out[e]
    fa, fq, f1, f2 = write_inputs(tmp_path, seqs, rd, pr)
    gap, ix = engines["gap"], engines["ix"]["gap", k]
    ins = "%d,%d" % mq.INSERT
    base = ["-r", fa, "-e", e, "--k", k, "--mapq", "gap"]
    # single end: best hit, all hits, and both sorted
    for extra, kw in (([], {}), (["--all-hits", MAX_HITS], dict(max_hits=MAX_HITS)), (["--sort"], dict(sort=True)),
                      (["--all-hits", MAX_HITS, "--sort"], dict(max_hits=MAX_HITS, sort=True))):
        plain = tool(base + ["-q", fq, "--both-strands"] + extra, tmp_path / "plain.sam")
        gap.map_file(ix, NAMES, str(fq), str(tmp_path / "lib.sam"), e, **kw)
        assert body(tmp_path / "lib.sam") == plain, extra
        assert tool(base + ["-q", fq, "--both-strands", "--stream"] + extra, tmp_path / "stream.sam") == plain, extra
        if "--sort" not in extra:  # column 5 against the model, line by line: a read's lines come in rank order
            got = {}
            for line in plain:
                f = line.split(b"\t")
                if f[2] != b"*":
                    got.setdefault(int(f[0].split(b"_")[0][1:]), []).append(int(f[4]))
            for t, (_, _, loci) in enumerate(rd):
                assert got.get(t, []) == mq.mapq_ref_read(loci, e)[:MAX_HITS if extra else 1], t
    # pairs, plain and sorted
    pbase = base + ["-1", f1, "-2", f2, "--insert", ins, "--rescue", mq.rescue_errors(e)]
    for extra, kw in (([], {}), (["--sort"], dict(sort=True))):
        plain = tool(pbase + extra, tmp_path / "pplain.sam")
        gap.map_pairs_file(ix, NAMES, str(f1), str(f2), str(tmp_path / "plib.sam"), e, *mq.INSERT, rescue_errors=mq.rescue_errors(e), **kw)
        assert body(tmp_path / "plib.sam") == plain, extra
        assert tool(pbase + ["--stream-pairs"] + extra, tmp_path / "pstream.sam") == plain, extra
        if not extra:
            for t, p in enumerate(pr):
                for x in range(2):
                    f = plain[2 * t + x].split(b"\t")
                    assert int(f[4]) == (p[5]["primary"][x] if not int(f[1]) & 4 else 0), (t, x, p[0])


def test_the_default_is_model_0_byte_for_byte(world, engines, tmp_path):
    seqs, out = world
    e, k = 2, 12
    rd, pr = out[e]
    reads, r1, r2 = [q for _, q, _ in rd], [p[1] for p in pr], [p[2] for p in pr]
    fa, fq, f1, f2 = write_inputs(tmp_path, seqs, rd, pr)
    kw = dict(rescue_errors=mq.rescue_errors(e))
    answers = []
    for name in ("default", "ref"):
        eng, ix = engines[name], engines["ix"][name, k]
        a = [eng.map_reads(ix, reads, e), eng.map_reads_all(ix, reads, e, max_hits=MAX_HITS), eng.map_pairs(ix, r1, r2, e, *mq.INSERT, **kw),
             eng.map_pairs_all(ix, r1, r2, e, *mq.INSERT, max_pairs=MAX_PAIRS, **kw)]
        files = []
        for t, fkw in enumerate((dict(), dict(max_hits=MAX_HITS), dict(sort=True))):
            eng.map_file(ix, NAMES, str(fq), str(tmp_path / ("%s%d.sam" % (name, t))), e, header="@HD\tVN:1.6\n", **fkw)
            files.append(open(tmp_path / ("%s%d.sam" % (name, t)), "rb").read())
        for t, fkw in enumerate((dict(), dict(sort=True))):
            eng.map_pairs_file(ix, NAMES, str(f1), str(f2), str(tmp_path / ("%sp%d.sam" % (name, t))), e, *mq.INSERT, header="@HD\tVN:1.6\n",
                               **kw, **fkw)
            files.append(open(tmp_path / ("%sp%d.sam" % (name, t)), "rb").read())
        answers.append((a, files))
    (a0, f0), (a1, f1_) = answers
    for x, y in zip(a0, a1):
        same_records(x, y)
        assert np.array_equal(x["mapping_quality"], y["mapping_quality"]) and np.array_equal(x["mapq"], y["mapq"])
    assert f0 == f1_ and all(len(f) > 1000 for f in f0)
    # and the tool: no option, and --mapq reference
    one = tool(["-r", fa, "-q", fq, "-e", e, "--both-strands"], tmp_path / "t0.sam")
    assert one == tool(["-r", fa, "-q", fq, "-e", e, "--both-strands", "--mapq", "reference"], tmp_path / "t1.sam")
    assert one == body(tmp_path / "default0.sam")
    for line in one:
        f = line.split(b"\t")
        if f[2] != b"*":
            xg = [int(x[5:]) for x in f if x.startswith(b"XG:i:")][0]
            assert int(f[4]) == min(254, 60 + xg)


def test_a_seed_capped_read_claims_no_gap_above_one(asm, world, engines):
    seqs, _ = world
    e, k = 2, 12
    r, a = mq.FAMILIES["five"]["at"][0]
    q = seqs[r][a + 70:a + 170]  # its first two pieces lie in the 5-copy family, the third in unique sequence
    gap, ix = engines["gap"], engines["ix"]["gap", k]
    free = gap.map_reads(ix, [q], e)
    assert free["mapped"][0] and free["mapping_quality"][0] == 60 and not free["flags"][0] & asm.MAP_SEED_CAPPED
    capped = gap.map_reads(ix, [q], e, max_occ=4)  # below the family's bucket size of 5
    assert capped["mapped"][0] and capped["flags"][0] & asm.MAP_SEED_CAPPED
    assert capped["mapping_quality"][0] == 20
    all_capped = gap.map_reads_all(ix, [q], e, max_hits=MAX_HITS, max_occ=4)
    assert all_capped["mapping_quality"].tolist() == [20]


def test_the_new_calls_reject_on_a_handle(asm):
    import ctypes

    eng = asm.Engine(0)
    try:
        with pytest.raises(asm.AsmError, match="model must be"):
            eng.set_mapq_model(2)
        assert eng.mapq_model() == 0
        with pytest.raises(asm.AsmError, match="no in-memory mapping call"):
            eng.last_mapq(1)
        ix = eng.build_index(["ACGT" * 64], k=8)
        eng.map_reads(ix, ["ACGTACGTACGTACGTACGT"], 0)
        assert eng.last_mapq(1).shape == (1,)
        for count in (0, 2):
            with pytest.raises(asm.AsmError, match="count must be"):
                eng.last_mapq(count)
        # a rejected call does not touch the last call's values
        hits = np.zeros(1, asm.MAP_HIT_DTYPE)
        p = asm.MapParams(16, 1, 0, 3)
        ro = np.array([0, 20], np.uint32)
        assert eng.lib.asm_map_reads(eng.h, ix.ptr, 1, b"A" * 20, ro.ctypes.data, ctypes.byref(p), hits.ctypes.data, None, 0, None) == -1
        assert eng.last_mapq(1).shape == (1,)
        ix.free()
    finally:
        eng.close()
