"""CPU checks of the mapping-quality model (docs/design/mapper.md, "Mapping quality"): its Python statement (tests/mapq_cases.py)
against a hand-written table of every branch, what the corpus yields under the brute forces alone, the core's folds
(csrc/asm_map_core.h through host/map_host_check.cpp, built stand-alone under ASan + UBSan) against that statement on the corpus,
and the argument checks of the new calls that need no device."""
import os
import struct
import subprocess

import pytest

from tests import mapq_cases as mq
from tests.test_map_all_host import bf_all, build_bruteforce_all
from tests.test_map_core_host import Reader, case_bytes
from tests.test_map_file_host import PKG, san_flags
from tests.test_map_pairs_host import bf_pairs, build_bruteforce_rescue


def L(*ds):
    """loci with the distances ds, as bf_all lists them: (s, r, i, j, d)"""
    return [(0, 0, 1000 * t, 1000 * t + 100, d) for t, d in enumerate(ds)]


def test_table_by_hand():
    assert [mq.table(1, g) for g in (1, 2, 3, 4, 16)] == [20, 40, 60, 60, 60]
    assert [mq.table(n, 1) for n in (2, 3, 4, 5, 6, 300)] == [3, 1, 1, 0, 0, 0]
    assert mq.table(0, 1) == 0


@pytest.mark.parametrize("ds, e, capped, want", [
    ((0,), 2, False, [60]),            # unique, nothing else within e: d2 = e + 1
    ((0,), 0, False, [20]),            # at e = 0 the search proves a gap of 1 only
    ((2,), 2, False, [20]),            # d1 = e: gap 1
    ((1,), 2, False, [40]),
    ((0, 1), 4, False, [20, 0]),       # the alternative one edit away; it gets 0 itself
    ((0, 2), 4, False, [40, 0]),
    ((0, 3, 4), 4, False, [60, 0, 0]),
    ((1, 1), 2, False, [3, 3]),        # ties share Q_read
    ((0, 0, 0, 2), 2, False, [1, 1, 1, 0]),
    ((0, 0, 0, 0), 2, False, [1] * 4),
    ((0,) * 5, 2, False, [0] * 5),
    ((0,), 4, True, [20]),             # SEED_CAPPED: no gap above 1 is claimed
    ((0, 0), 4, True, [3, 3]),         # the cap only lowers
    ((), 2, False, []),
])
def test_single_end_by_hand(ds, e, capped, want):
    assert mq.mapq_ref_read(L(*ds), e, capped) == want


def _pair(a, b):
    """an FR pair of loci on sequence 0: a forward at j = 100, b reverse with its end at b[0]; each (j, d)"""
    return (0, 0, a[0] - 100, a[0], a[1]), (1, 0, b[0] - 100, b[0], b[1])


def test_pairs_by_hand():
    lo, hi, e = 200, 400, 2
    a, b = _pair((100, 0), (300, 0))
    res = {"rec": [a, b], "rescued": None}
    # one concordant pair, both mates unique: every term agrees
    out = mq.mapq_ref_pair([a], [b], 100, 100, lo, hi, e, res)
    assert out["primary"] == (60, 60) and out["Q_pair"] == 60 and out["fold"] == (0, 1, None)
    # mate 1 in five copies, four of them out of reach: the pair lifts it from 0
    far = [(0, 0, 5000 * t, 5000 * t + 100, 0) for t in range(1, 5)]
    out = mq.mapq_ref_pair([a] + far, [b], 100, 100, lo, hi, e, res)
    assert out["Q_locus"] == (0, 60) and out["Q_pair"] == 60 and out["primary"] == (60, 60)
    # the second term of g: a mate at d = 2 = e leaves room for one more edit only
    a2, b2 = _pair((100, 2), (300, 0))
    out = mq.mapq_ref_pair([a2], [b2], 100, 100, lo, hi, e, {"rec": [a2, b2], "rescued": None})
    assert out["Q_pair"] == 20 and out["primary"] == (20, 60)  # mate 2 keeps its better single-end value
    # the first term: another concordant pair one edit above
    b3 = (1, 0, 250, 350, 1)
    out = mq.mapq_ref_pair([a], [b, b3], 100, 100, lo, hi, e, res)
    assert out["fold"] == (0, 2 - 1, 1) and out["Q_pair"] == 20
    assert [p[2] for p in out["pairs"]] == [(60, 20), (0, 0)]  # mate 1 is unique on its own; the pair above S1 gets 0
    # two pairs tie: 3 on both, on every record with the sum S1
    b4 = (1, 0, 250, 350, 0)
    out = mq.mapq_ref_pair([a], [b, b4], 100, 100, lo, hi, e, res)
    assert out["fold"] == (0, 2, None) and [p[2] for p in out["pairs"]] == [(60, 3), (60, 3)]
    # SEED_CAPPED on either mate caps Q_pair
    out = mq.mapq_ref_pair([a], [b], 100, 100, lo, hi, e, res, capped=(False, True))
    assert out["Q_pair"] == 20 and out["primary"] == (60, 20)
    # rescued: the anchor keeps Q_read, the rescued mate min(Q_anchor, 20)
    y = (1, 0, 200, 300, 5)
    out = mq.mapq_ref_pair([a], [], 100, 100, lo, hi, e, {"rec": [a, y], "rescued": 1})
    assert out["primary"] == (60, 20)
    out = mq.mapq_ref_pair([a, far[0]], [], 100, 100, lo, hi, e, {"rec": [a, y], "rescued": 1})
    assert out["primary"] == (3, 3)
    # no proper pair: each mate its single-end value, 0 when unmapped
    c = (0, 0, 9000, 9100, 1)
    out = mq.mapq_ref_pair([a], [c], 100, 100, lo, hi, e, {"rec": [a, c], "rescued": None})
    assert out["primary"] == (60, 40)
    out = mq.mapq_ref_pair([a], [], 100, 100, lo, hi, e, {"rec": [a, None], "rescued": None})
    assert out["primary"] == (60, 0)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the corpus under the brute forces alone: per e the reads with their loci, the pairs with their loci and bf_pairs' answer"""
    bfa = build_bruteforce_all(tmp_path_factory.mktemp("mapq_bfa"))
    bfr = build_bruteforce_rescue(tmp_path_factory.mktemp("mapq_bfr"))
    seqs = mq.reference()
    out = {}
    for e in mq.E_SWEEP:
        rd = [(label, q, bf_all(bfa, seqs, q, e)) for label, q in mq.reads(seqs, e)]
        pr = []
        for label, q1, q2 in mq.pairs(seqs, e):
            loci = [bf_all(bfa, seqs, q1, e), bf_all(bfa, seqs, q2, e)]
            res = bf_pairs(bfa, bfr, seqs, q1, q2, e, *mq.INSERT, rescue=mq.rescue_errors(e), k=8, loci=loci)
            pr.append((label, q1, q2, loci, res))
        out[e] = (rd, pr)
    return seqs, out


def test_corpus_yields_every_value_single_end(corpus):
    _, out = corpus
    seen = set()
    n = 0
    for e, (rd, _) in out.items():
        for label, q, loci in rd:
            seen.update(mq.mapq_ref_read(loci, e))
            n += 1
    assert seen == {60, 40, 20, 3, 1, 0}
    # "a few hundred reads in all": the single-end reads of the three e and both mates of every pair
    assert 250 <= n + sum(2 * len(pr) for _, pr in out.values()) <= 600


def test_corpus_yields_a_lifted_and_a_rescued_mate(corpus):
    _, out = corpus
    lifted = rescued = tied = 0
    for e, (_, pr) in out.items():
        for label, q1, q2, loci, res in pr:
            ref = mq.mapq_ref_pair(loci[0], loci[1], len(q1), len(q2), *mq.INSERT, e, res)
            if ref["Q_pair"] is not None:
                lifted += any(ref["Q_pair"] > ql for ql in ref["Q_locus"])
                tied += ref["fold"][1] == 2
            rescued += res["rescued"] is not None
    assert lifted >= 1 and rescued >= 1 and tied >= 1


def test_core_folds_equal_the_model_on_the_corpus_under_sanitizers(corpus, tmp_path):
    seqs, out = corpus
    exe, src = str(tmp_path / "map_host_check_asan"), os.path.join(PKG, "host", "map_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = []
    for e, (rd, pr) in out.items():
        for k in mq.K_SWEEP:
            cases.append((e, k, 0, [q for _, q, _ in rd]))
            cases.append((e, k, 1, [p[1] for p in pr] + [p[2] for p in pr]))
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(seqs)) + b"".join(struct.pack("<I", len(s)) + s.encode() for s in seqs))
        fh.write(struct.pack("<I", len(cases)))
        for e, k, paired, reads in cases:
            fh.write(case_bytes(reads, k, e, paired, *(mq.INSERT if paired else (0, 0)), rescue=mq.rescue_errors(e) if paired else -1))
    r = subprocess.run([exe, str(fin), str(fout), "--mapq"], capture_output=True, text=True, timeout=900)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rdr = Reader(open(fout, "rb").read())
    checked = 0
    for e, k, paired, reads in cases:
        rdr.case(len(reads), paired)
        folds = [rdr.take("IIII") for _ in reads]
        rd, pr = out[e]
        loci = [x[2] for x in rd] if not paired else [p[3][0] for p in pr] + [p[3][1] for p in pr]
        for t, (d1, n1, d2, q) in enumerate(folds):
            assert (d1, n1, d2) == mq.read_fold([l[4] for l in loci[t]], e), (e, k, paired, t)
            assert q == mq.read_quality(loci[t], e), (e, k, paired, t)
            checked += 1
        for t in range(len(reads) // 2 if paired else 0):
            S1, N1, S2, qp, qa, qb = rdr.take("iIiIII")
            label, q1, q2, lc, res = pr[t]
            ref = mq.mapq_ref_pair(lc[0], lc[1], len(q1), len(q2), *mq.INSERT, e, res)
            assert (qa, qb) == tuple(ref["primary"]), (e, k, label, t)
            if ref["fold"] is not None:
                assert (S1, N1, -1 if S2 < 0 else S2, qp) == (ref["fold"][0], ref["fold"][1], -1 if ref["fold"][2] is None else ref["fold"][2],
                                                              ref["Q_pair"]), (e, k, label, t)
            else:
                assert N1 == 0 and qp == 0
            checked += 1
    assert rdr.at == len(rdr.data) and checked > 500


def _err(asm):
    return asm.load_library().asm_last_error(None).decode()


def test_new_calls_reject_bad_arguments(asm):
    """What can be rejected without a device: a bad model, and asm_map_last_mapq's count and dst, each checked before the handle is
    looked at.  "Wrong count" and "no prior call" compare against a handle's state, and a handle needs a device, so those two are
    in tests/test_gpu_mapq.py::test_the_new_calls_reject_on_a_handle."""
    lib = asm.load_library()
    for model in (-1, 2, 60):
        assert lib.asm_map_set_mapq_model(None, model) == -1 and "model must be" in _err(asm)
    for model in (asm.MAPQ_REFERENCE, asm.MAPQ_GAP):  # a good model: only the missing handle is left
        assert lib.asm_map_set_mapq_model(None, model) == -1 and "handle" in _err(asm)
    assert lib.asm_map_get_mapq_model(None) == asm.MAPQ_REFERENCE
    import ctypes

    buf = ctypes.create_string_buffer(16)
    assert lib.asm_map_last_mapq(None, buf, -1) == -1 and "count" in _err(asm)
    assert lib.asm_map_last_mapq(None, None, 4) == -1 and "dst" in _err(asm)
    assert lib.asm_map_last_mapq(None, buf, 4) == -1 and "handle" in _err(asm)
    assert (asm.MAPQ_REFERENCE, asm.MAPQ_GAP) == (0, 1)
