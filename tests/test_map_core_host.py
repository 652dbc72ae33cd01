"""The read mapper's per-thread core (csrc/asm_map_core.h) on the CPU (docs/design/mapper.md, "Core and kernels"):
host/map_host_check.cpp, the serial mirror of the pipeline of csrc/asm_map.h, built with plain g++ under ASan + UBSan and run as a
program over reference_small() at every kernel width W in {1, 2, 4, 8}.  Best hits equal tests/cxx/map_bruteforce.cpp, loci
equal tests/cxx/map_bruteforce_all.cpp, CIGARs equal map_cases.ref_cigar op for op, pairs equal an enumeration over the two loci
lists written here, rescued mates equal tests/cxx/map_bruteforce_rescue.cpp.  Any sanitizer report fails the module."""
import os
import random
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import map_cases as mc
from tests.test_map_all_host import bf_all, build_bruteforce_all
from tests.test_map_file_host import PKG, san_flags
from tests.test_map_host import bf_map, build_bruteforce, revcomp
from tests.test_map_pairs_host import bf_pairs, build_bruteforce_rescue, concordant, pair_rank

WIDTHS = (1, 2, 4, 8)
CELLS = [(W, e, mc.K_SWEEP, None) for W in WIDTHS for e in mc.errors_of(W)]
CELLS += [(mc.width_of(m), e, k, (m,)) for k in sorted(mc.EXTRA_CELLS) for m, e in mc.EXTRA_CELLS[k]]
EDGES = {1: (63, 64), 2: (65, 128), 4: (129, 256), 8: (257, 511)}  # one length per side of each word edge
E_ALL, E_PAIR, K = 3, 2, mc.K_SWEEP
CIGAR_CAP, PAIR_CAP = 64, 8
POOL = min(16, os.cpu_count() or 1)


def case_bytes(reads, k, e, paired=0, lo=0, hi=0, rescue=-1):
    out = struct.pack("<4I3i2I", k, e, 1, paired, lo, hi, rescue, CIGAR_CAP, PAIR_CAP) + struct.pack("<I", len(reads))
    return out + b"".join(struct.pack("<I", len(q)) + q.encode() for q in reads)


class Reader:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, fmt):
        v = struct.unpack_from("<" + fmt, self.data, self.at)
        self.at += struct.calcsize("<" + fmt)
        return v

    def case(self, n, paired):
        """-> records (mapped, s, r, i, j, d, flags, ops), loci lists of (s, r, j, d), pairs"""
        recs, loci, pairs = [], [], []
        for _ in range(n):
            seq_id, pos, end, dist, strand, flags, nops = self.take("iIIiIII")
            ops = self.take("%dH" % min(nops, CIGAR_CAP))
            recs.append(((1, strand, seq_id, pos, end, dist) if flags & 1 else (0, -1, -1, -1, -1, -1), flags, nops, ops))
        for _ in range(n):
            (cnt,) = self.take("I")
            loci.append([unkey(k)[:4] for k in self.take("%dQ" % cnt)])
        for _ in range(n // 2 if paired else 0):
            state, n_conc, ka, kb, n_pairs, listed = self.take("IIQQII")
            ks = self.take("%dQ" % (2 * listed))
            pairs.append({"state": state, "n_conc": n_conc, "item": (unkey(ka), unkey(kb)), "n_pairs": n_pairs,
                          "list": [(unkey(ks[2 * t]), unkey(ks[2 * t + 1])) for t in range(listed)]})
        return recs, loci, pairs


def unkey(k):
    """packed locus key -> (s, r, j, d), None for MAP_NO_KEY"""
    return None if k == 2**64 - 1 else ((k >> 58) & 1, (k >> 32) & (2**26 - 1), k & 0xffffffff, k >> 59)


def cigar_string(ops):
    return "".join("%d%s" % (o >> 3, "MID"[o & 7]) for o in ops)


def frag_pairs(seqs, up, m, e, seed):
    """the FR pairs of map_cases.pair_reads at one mate length (fragments of 2 m + 40 .. 2 m + 99 bases; mate 2 with e or e + 2 edits,
    one too short to seed), plus a fragment inside the segment that sequences 3 and 7 share (two concordant combinations) and a
    pair with both mates forward (none)"""
    r1s, r2s = mc.pair_reads(seqs, (m,), e, K, seed)
    f = 2 * m + 70
    for a, same in ((5_100, False), (22_000, True)):
        assert "N" not in up[3][a:a + f]
        q2 = up[3][a + f - m:a + f]
        r1s.append(up[3][a:a + m])
        r2s.append(q2 if same else revcomp(q2))
    return r1s, r2s


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """every case through one run of the sanitized driver: name -> (reads, parsed output)"""
    tmp = tmp_path_factory.mktemp("map_core")
    exe, src = str(tmp / "map_host_check_asan"), os.path.join(PKG, "host", "map_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    seqs = mc.reference_small()
    up = [s.upper() for s in seqs]
    cases = {}
    for c in CELLS:
        W, e, k, lengths = c
        rows = mc.class_reads(seqs, W, e, k, lengths)
        if lengths is None:  # the sweep's cells: a fifth of each cell's reads, drawn with a fixed seed, keeps the module quick
            rows = random.Random(97 * W + e).sample(rows, (len(rows) + 4) // 5)
        cases[("best",) + c] = ([q for _, q in rows], dict(k=k, e=e), [kind for kind, _ in rows])
    for W in WIDTHS:
        rows = mc.class_reads(seqs, W, E_ALL, K, EDGES[W])
        cases[("all", W)] = ([q for _, q in rows], dict(k=K, e=E_ALL), None)
    for m in (100, 129):
        r1s, r2s = frag_pairs(seqs, up, m, E_PAIR, seed=m)
        f = 2 * m + 70
        # windows that admit no fragment, one combination per fragment, and both sequences' copies with a wide margin
        for lo, hi in ((0, m), (f - 30, f + 29), (0, 1400)):
            cases[("pairs", m, lo, hi)] = (r1s + r2s, dict(k=K, e=E_PAIR, paired=1, lo=lo, hi=hi, rescue=-1), None)
        # rescue: the mates with e + 2 edits; 701 ends span five tiles of MAP_RESCUE_TILE = 128, 129 ends cross one tile boundary
        for lo, hi in ((f - 64, f + 64), (f - 100, f + 600)):
            cases[("rescue", m, lo, hi)] = (r1s + r2s, dict(k=K, e=E_PAIR, paired=1, lo=lo, hi=hi, rescue=6), None)
    fin, fout = tmp / "cases.bin", tmp / "out.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(seqs)) + b"".join(struct.pack("<I", len(s)) + s.encode() for s in seqs))
        fh.write(struct.pack("<I", len(cases)))
        for reads, kw, _ in cases.values():
            fh.write(case_bytes(reads, **kw))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=900)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rd = Reader(open(fout, "rb").read())
    out = {name: (reads, kw, kinds, rd.case(len(reads), kw.get("paired", 0))) for name, (reads, kw, kinds) in cases.items()}
    assert rd.at == len(rd.data)
    return seqs, up, out


@pytest.fixture(scope="module")
def bf(tmp_path_factory):
    return build_bruteforce(tmp_path_factory.mktemp("map_bf_core"))


@pytest.fixture(scope="module")
def bfa(tmp_path_factory):
    return build_bruteforce_all(tmp_path_factory.mktemp("map_bf_all_core"))


@pytest.fixture(scope="module")
def bfr(tmp_path_factory):
    return build_bruteforce_rescue(tmp_path_factory.mktemp("map_bf_rescue_core"))


def strand_read(q, s):
    return revcomp(q.upper()) if s else q.upper()


def test_best_hit_and_cigar_equal_brute_force_at_every_width(run, bf):
    seqs, up, out = run

    jobs = [(c, t) for c in CELLS for t in range(len(out[("best",) + c][0]))]
    with ThreadPoolExecutor(POOL) as ex:  # one pool over the reads of all cells
        want = dict(zip(jobs, ex.map(lambda job: bf_map(bf, seqs, out[("best",) + job[0]][0][job[1]], job[0][1]), jobs)))
    for c in CELLS:
        W, e, k, _ = c
        reads, _, kinds, (recs, _, _) = out[("best",) + c]
        assert all(mc.width_of(len(q)) == W for q in reads)
        n_mapped = 0
        for t, q in enumerate(reads):
            got, flags, nops, ops = recs[t]
            rec = want[(c, t)]
            short = len(q) < (e + 1) * k  # the one exclusion of tests/test_gpu_map_widths.py: a read that cannot seed
            assert bool(flags & 2) == short and not flags & (4 | 8), (c, t, flags)
            assert got == ((0, -1, -1, -1, -1, -1) if short else rec), (c, t, kinds[t], q, got, rec)
            cigar = mc.ref_cigar(strand_read(q, got[1]), up[got[2]][got[3]:got[4]]) if got[0] else ""
            assert cigar_string(ops) == cigar and nops == len(ops), (c, t, kinds[t], q)
            n_mapped += got[0]
        assert n_mapped


@pytest.mark.parametrize("W", WIDTHS)
def test_all_loci_equal_brute_force_at_the_word_edges(run, bfa, W):
    seqs, up, out = run
    reads, _, _, (_, loci, _) = out[("all", W)]
    assert {len(q) for q in reads} == set(EDGES[W])
    with ThreadPoolExecutor(POOL) as ex:
        want = list(ex.map(lambda q: bf_all(bfa, seqs, q, E_ALL), reads))
    for t, q in enumerate(reads):
        assert loci[t] == sorted(loci[t], key=lambda x: x[:3])  # walk order
        assert sorted(loci[t]) == sorted((s, r, j, d) for s, r, i, j, d in want[t]), (t, q)
    assert sum(1 for x in loci if x) >= len(reads) // 2


def mate_loci(bfa, seqs, reads, e):
    with ThreadPoolExecutor(POOL) as ex:
        return list(ex.map(lambda q: [] if len(q) < (e + 1) * K else bf_all(bfa, seqs, q, e), reads))


@pytest.mark.parametrize("m", [100, 129])
def test_pairs_equal_an_enumeration_over_the_loci_lists(run, bfa, m):
    seqs, up, out = run
    seen = set()
    for name in [x for x in out if x[:2] == ("pairs", m)]:
        reads, kw, _, (recs, _, pairs) = out[name]
        n = len(reads) // 2
        loci = mate_loci(bfa, seqs, reads, E_PAIR)
        for p in range(n):
            m1, m2 = len(reads[p]), len(reads[n + p])
            conc = sorted((pair_rank(a, b), a, b) for a in loci[p] for b in loci[n + p] if concordant(a, b, m1, m2, kw["lo"], kw["hi"]))
            got = pairs[p]
            flat = lambda x: (x[0], x[1], x[3], x[4])  # noqa: E731  (s, r, i, j, d) -> (s, r, j, d)
            assert got["n_pairs"] == len(conc) and got["list"] == [(flat(a), flat(b)) for _, a, b in conc[:PAIR_CAP]], (name, p)
            assert got["n_conc"] == sum(1 for x in conc if x[0][0] == conc[0][0][0]), (name, p)
            if conc:
                assert got["state"] == 1 and got["item"] == (flat(conc[0][1]), flat(conc[0][2])), (name, p)
                for y, x in ((p, conc[0][1]), (n + p, conc[0][2])):
                    assert recs[y][0] == (1, x[0], x[1], x[2], x[3], x[4]), (name, p)
            else:  # each mate its best hit
                assert got["state"] == 0
                for y in (p, n + p):
                    assert recs[y][0] == ((1,) + loci[y][0] if loci[y] else (0, -1, -1, -1, -1, -1)), (name, p)
            seen.add(min(len(conc), 2))
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("m", [100, 129])
def test_rescue_equals_brute_force_across_tiles(run, bfa, bfr, m):
    seqs, up, out = run
    n_resc = 0
    for name in [x for x in out if x[:2] == ("rescue", m)]:
        reads, kw, _, (recs, _, pairs) = out[name]
        n = len(reads) // 2
        loci = mate_loci(bfa, seqs, reads, E_PAIR)
        for p in range(n):
            want = bf_pairs(bfa, bfr, up, reads[p], reads[n + p], E_PAIR, kw["lo"], kw["hi"], kw["rescue"], K, loci=[loci[p], loci[n + p]])
            for y, x in ((p, want["rec"][0]), (n + p, want["rec"][1])):
                assert recs[y][0] == ((1,) + tuple(x) if x is not None else (0, -1, -1, -1, -1, -1)), (name, p, y)
                if recs[y][0][0]:
                    _, s, r, i, j, d = recs[y][0]
                    assert cigar_string(recs[y][3]) == mc.ref_cigar(strand_read(reads[y], s), up[r][i:j]), (name, p, y)
            assert pairs[p]["state"] == (1 if want["n_concordant"] else 0 if want["rescued"] is None else 3 + want["rescued"]), (name, p)
            assert pairs[p]["n_conc"] == want["n_concordant"]
            n_resc += want["rescued"] is not None
    assert n_resc >= 4
