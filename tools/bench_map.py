"""Read-mapper timings (development tool): PYTHONPATH=. python tools/bench_map.py [--ref-len 5e6] [--reads 1e6] [--len 100]
[--errors 2 4] [--all-hits N [--strata S]] [--repeats] [--out DIR] [--dump DIR] [--profile]
A random reference (one sequence, seeded) and reads sampled from both strands with 0..e substitutions plus 10 % random reads;
reports the index build and the mapping of all reads (both strands), each timed with HIP events on the engine's stream around one
synchronous library call (so host-to-device copies and the host's share of asm_map_reads are inside), plus the wall clock.
--all-hits N also times asm_map_reads_all (up to N loci per read, strata S, default e), alternating with asm_map_reads in the
same process, and prints the hits-per-read distribution.  --repeats pastes 200 copies of a 2 kbp element (0-3 % substitutions,
half reverse-complemented) and 6 kbp of a period-6 tandem repeat into the reference, and draws 30 % of the reads from them.
--paired [--insert 200,500] [--rescue E] simulates --reads / 2 FR pairs (fragments uniform in the insert range, mates of --len
bases with 0..e substitutions; 5 % discordant pairs: out of range, same strand or far apart; 10 % random pairs; 10 % of pairs with
one mate carrying e+1..e+3 substitutions; with --repeats, 30 % of the fragments inside the element copies) and times asm_map_pairs
against asm_map_reads_all (strata = e, max_hits = 1) on the same reads, alternately, and reports the proper and rescued fractions.
--paired --all-hits N [--strata S] times asm_map_pairs_all (up to N pairs per fragment, pair strata S, default 2e) against
asm_map_pairs instead, alternately, and prints the n_pairs distribution.
--dump DIR writes DIR/digests.json: the SHA-256 of every output array of every timed call (per e; CIGAR rows up to their nops), for comparing two builds
of the library (ASM_MI355X_LIB, a fresh process each) for exact equality on a workload of real size.
--mapq reference|gap sets the engine's MAPQ model (docs/design/mapper.md, "Mapping quality") before anything is timed; under gap
asm_map_reads takes the runs path, which is what the option is there to price.  Every row also lists the timed call's
milliseconds of each repeat (map_ms_reps), so that a run shows its own spread.
--profile re-runs the same command under `rocprofv3 --kernel-trace --stats` (a run of its own) and prints the per-kernel totals."""
import argparse
import ctypes
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import approximate_string_matching_amd as m  # noqa: E402

LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = np.arange(256)
for a, b in (b"AT", b"TA", b"CG", b"GC"):
    COMP[a] = b


def make_inputs(ref_len, n, length, e, seed, repeats=False):
    rng = np.random.default_rng(seed)
    ref = LUT[rng.integers(0, 4, ref_len)]
    starts = rng.integers(0, ref_len - length, n)
    if repeats:  # element copies every 20 kbp from 100 kbp on, the tandem repeat at 4.5 Mbp
        elem = LUT[rng.integers(0, 4, 2000)]
        places = 100_000 + 20_000 * np.arange(200)
        for c, a in enumerate(places):
            copy = elem.copy()
            sub = rng.random(2000) < 0.03 * (c % 4) / 3
            copy[sub] = LUT[(np.searchsorted(LUT, copy[sub]) + rng.integers(1, 4, int(sub.sum()))) % 4]
            ref[a:a + 2000] = COMP[copy[::-1]] if c % 2 else copy
        tandem = np.frombuffer(b"AGGTCA" * 1000, np.uint8)
        ref[4_500_000:4_500_000 + tandem.size] = tandem
        rep = rng.random(n) < 0.3
        k = int(rep.sum())
        from_tandem = rng.random(k) < 0.1
        starts[rep] = np.where(from_tandem, 4_500_000 + rng.integers(0, tandem.size - length, k),
                               places[rng.integers(0, 200, k)] + rng.integers(0, 2000 - length, k))
    reads = ref[starts[:, None] + np.arange(length)[None, :]].copy()
    for t in range(e):  # substitutions at random places (some may hit the same base twice: 0..e edits)
        hit = rng.random(n) < 0.7
        col = rng.integers(0, length, n)
        reads[hit, col[hit]] = LUT[(np.searchsorted(LUT, reads[hit, col[hit]]) + rng.integers(1, 4, hit.sum())) % 4]
    rev = rng.random(n) < 0.5
    reads[rev] = COMP[reads[rev][:, ::-1]]
    rnd = rng.random(n) < 0.1
    reads[rnd] = LUT[rng.integers(0, 4, (int(rnd.sum()), length))]
    return ref, reads


def dump_digests(a, e, arrays):
    """adds {call.array: sha256} of one e to DIR/digests.json"""
    os.makedirs(a.dump, exist_ok=True)
    path = os.path.join(a.dump, "digests.json")
    table = json.load(open(path)) if os.path.exists(path) and e != a.errors[0] else {}
    arrays = {name: v for name, v in arrays.items() if v is not None}
    for name in [x for x in arrays if x.endswith(".ops")]:  # a CIGAR row is defined up to its nops; the rest is whatever was there
        nops = arrays[name[:-4] + ".nops"].reshape(-1, 1)
        arrays[name] = np.where(np.arange(16)[None, :] < nops, arrays[name].reshape(-1, 16), 0).astype(np.uint16)
    table["e=%d" % e] = {name: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for name, v in arrays.items()}
    with open(path, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=float, default=5e6)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--errors", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--all-hits", type=int, default=0, help="also time asm_map_reads_all with up to N loci per read")
    ap.add_argument("--strata", type=int, default=None, help="with --all-hits: strata (default e; --paired: 2e)")
    ap.add_argument("--repeats", action="store_true", help="the reference with repeats, 30 %% of the reads from them")
    ap.add_argument("--paired", action="store_true", help="time asm_map_pairs on --reads / 2 simulated pairs")
    ap.add_argument("--insert", default="200,500", help="with --paired: MIN,MAX of the projected span")
    ap.add_argument("--rescue", type=int, default=-1, help="with --paired: mate rescue's error bound (-1: off)")
    ap.add_argument("--out", default=None, help="directory for the JSON result (and the profile with --profile)")
    ap.add_argument("--dump", default=None, help="directory for digests.json, the SHA-256 of every output array")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--mapq", choices=["reference", "gap"], default="reference", help="the engine's MAPQ model")
    a = ap.parse_args()
    extra = ["--mapq", a.mapq]
    extra += (["--all-hits", str(a.all_hits)] if a.all_hits else []) + (["--strata", str(a.strata)] if a.strata is not None else [])
    extra += ["--repeats"] if a.repeats else []
    extra += ["--paired", "--insert", a.insert, "--rescue", str(a.rescue)] if a.paired else []
    n, ref_len = int(a.reads), int(a.ref_len)
    if a.profile:
        out = a.out or "bench_map_profile"
        os.makedirs(out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "map", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--ref-len", str(ref_len), "--reads", str(n), "--len", str(a.len),
               "--k", str(a.k), "--reps", "1", "--errors", *[str(e) for e in a.errors], *extra]
        subprocess.run(cmd, check=True, timeout=1200)
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                rows = list(csv.DictReader(fh))
            print("kernel totals (", path, ")")
            for r in rows:
                print("  %-60s calls %6s total ms %10.3f" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6))
        return
    eng = m.Engine(0)
    eng.set_mapq_model(a.mapq)
    lib, h = eng.lib, eng.h
    tm = eng.timer()
    results = {"ref_len": ref_len, "reads": n, "read_len": a.len, "k": a.k, "mapq": a.mapq, "repeats": a.repeats, "all_hits": a.all_hits, "runs": []}
    if a.paired:
        return run_paired(a, eng, tm, n, ref_len)
    for e in a.errors:
        ref, reads = make_inputs(ref_len, n, a.len, e, seed=1000 + e, repeats=a.repeats)
        off = np.array([0, ref_len], np.uint64)
        ix = ctypes.c_void_p()
        best_ix = 1e30
        for _ in range(a.reps):
            if ix.value:
                lib.asm_index_free(h, ix)
            tm.start()
            eng._chk(lib.asm_index_build(h, ref.ctypes.data, off.ctypes.data, 1, a.k, ctypes.byref(ix)))
            tm.stop()
            best_ix = min(best_ix, tm.elapsed_ms())
        flat = np.ascontiguousarray(reads.reshape(-1))
        ro = (np.arange(n + 1, dtype=np.uint64) * a.len).astype(np.uint32)
        hits = np.zeros(n, m.MAP_HIT_DTYPE)
        ops = np.zeros((n, 16), np.uint16)
        nops = np.zeros(n, np.uint8)
        p = m.MapParams(e, 1, 0, 3)
        H = max(a.all_hits, 1)
        strata = e if a.strata is None else a.strata
        n_hits = np.zeros(n, np.uint32)
        all_hits = np.zeros(n * H, m.MAP_HIT_DTYPE) if a.all_hits else None
        all_ops = np.zeros(n * H * 16, np.uint16) if a.all_hits else None
        all_nops = np.zeros(n * H, np.uint8) if a.all_hits else None
        best_map, best_wall, best_all = 1e30, 1e30, 1e30
        map_reps = []
        for _ in range(a.reps):  # the two calls alternate, so that both see the same machine state
            t0 = time.perf_counter()
            tm.start()
            eng._chk(lib.asm_map_reads(h, ix, n, flat.ctypes.data, ro.ctypes.data, ctypes.byref(p), hits.ctypes.data, ops.ctypes.data,
                                       16, nops.ctypes.data))
            tm.stop()
            best_map = min(best_map, tm.elapsed_ms())
            map_reps.append(round(tm.elapsed_ms(), 3))
            best_wall = min(best_wall, (time.perf_counter() - t0) * 1e3)
            if a.all_hits:
                tm.start()
                eng._chk(lib.asm_map_reads_all(h, ix, n, flat.ctypes.data, ro.ctypes.data, ctypes.byref(p), strata, a.all_hits,
                                               n_hits.ctypes.data, all_hits.ctypes.data, all_ops.ctypes.data, 16, all_nops.ctypes.data))
                tm.stop()
                best_all = min(best_all, tm.elapsed_ms())
        lib.asm_index_free(h, ix)
        if a.dump:
            dump_digests(a, e, {"reads.hits": hits, "reads.ops": ops, "reads.nops": nops, "reads_all.n_hits": n_hits if a.all_hits else None,
                                "reads_all.hits": all_hits, "reads_all.ops": all_ops, "reads_all.nops": all_nops})
        mapped = float(((hits["flags"] & m.MAP_MAPPED) != 0).mean())
        row = {"e": e, "mapq": a.mapq, "index_build_ms": round(best_ix, 3), "map_ms_events": round(best_map, 3), "map_ms_reps": map_reps, "map_ms_wall": round(best_wall, 3),
               "reads_per_s": round(n / best_map * 1e3), "mapped_fraction": round(mapped, 4)}
        if a.all_hits:
            rep_n = np.minimum(n_hits, a.all_hits)
            row.update({"all_hits": a.all_hits, "strata": strata, "all_ms_events": round(best_all, 3),
                        "all_reads_per_s": round(n / best_all * 1e3), "all_over_best": round(best_all / best_map, 3),
                        "hits_per_read_mean": round(float(n_hits.mean()), 3), "reported_per_read_mean": round(float(rep_n.mean()), 3),
                        # distribution of n_hits: 0, 1, 2-3, 4-15, 16-63, >= 64
                        "n_hits_hist": [int(v) for v in np.histogram(n_hits, [0, 1, 2, 4, 16, 64, 2**32])[0]]})
        results["runs"].append(row)
        print(json.dumps(row))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_map.json"), "w") as fh:
            json.dump(results, fh, indent=1)


def make_pairs(ref, npairs, length, e, lo, hi, seed, repeats=False):
    """-> (mates 1, mates 2) as (npairs, length) uint8 arrays; see the module docstring for the mix"""
    rng = np.random.default_rng(seed)
    L = ref.size
    f = rng.integers(max(lo, length), hi + 1, npairs)
    a = rng.integers(0, L - hi - 2100, npairs)
    if repeats:  # the element copies of make_inputs(repeats=True)
        rep = rng.random(npairs) < 0.3
        places = 100_000 + 20_000 * np.arange(200)
        a[rep] = places[rng.integers(0, 200, int(rep.sum()))] + rng.integers(0, 2000 - f[rep] + 1)
    cols = np.arange(length)[None, :]
    m1 = ref[a[:, None] + cols].copy()
    b = a + f - length
    kind = rng.random(npairs)
    disc = kind < 0.05
    far = disc & (kind < 0.05 / 3)
    out_of_range = disc & ~far & (kind < 0.1 / 3)
    b[far] = rng.integers(0, L - length, int(far.sum()))
    b[out_of_range] = a[out_of_range] + rng.integers(hi + 100, hi + 2000, int(out_of_range.sum()))
    m2 = ref[b[:, None] + cols].copy()
    same = disc & ~far & ~out_of_range
    m2[~same] = COMP[m2[~same][:, ::-1]]
    over = (kind >= 0.05) & (kind < 0.15)

    def substitute(x, rows, k):
        for _ in range(k):
            col = rng.integers(0, length, rows.size)
            x[rows, col] = LUT[(np.searchsorted(LUT, x[rows, col]) + rng.integers(1, 4, rows.size)) % 4]

    for x, skip in ((m1, np.zeros(npairs, bool)), (m2, over)):  # 0..e substitutions (not on the mates set below)
        for _ in range(e):
            hit = np.flatnonzero((rng.random(npairs) < 0.7) & ~skip)
            substitute(x, hit, 1)
    heavy = np.flatnonzero(over)
    extra = rng.integers(1, 4, heavy.size)
    for k in range(1, 4):  # e + 1 .. e + 3 substitutions, two columns apart
        rows = heavy[extra == k]
        col = rng.integers(0, length - 8, rows.size)
        for z in range(e + k):
            cc = (col + 2 * z) % length
            m2[rows, cc] = LUT[(np.searchsorted(LUT, m2[rows, cc]) + 1) % 4]
    rnd = (kind >= 0.15) & (kind < 0.25)
    m1[rnd] = LUT[rng.integers(0, 4, (int(rnd.sum()), length))]
    m2[rnd] = LUT[rng.integers(0, 4, (int(rnd.sum()), length))]
    swap = rng.random(npairs) < 0.5
    m1[swap], m2[swap] = m2[swap].copy(), m1[swap].copy()
    return m1, m2


def run_paired(a, eng, tm, n, ref_len):
    lib, h = eng.lib, eng.h
    lo, hi = (int(v) for v in a.insert.split(","))
    npairs = n // 2
    results = {"ref_len": ref_len, "pairs": npairs, "read_len": a.len, "k": a.k, "repeats": a.repeats, "insert": [lo, hi],
               "rescue": a.rescue, "runs": []}
    for e in a.errors:
        ref, _ = make_inputs(ref_len, 1, a.len, 0, seed=1000 + e, repeats=a.repeats)
        m1, m2 = make_pairs(ref, npairs, a.len, e, lo, hi, seed=2000 + e, repeats=a.repeats)
        off = np.array([0, ref_len], np.uint64)
        ix = ctypes.c_void_p()
        eng._chk(lib.asm_index_build(h, ref.ctypes.data, off.ctypes.data, 1, a.k, ctypes.byref(ix)))
        f1, f2 = np.ascontiguousarray(m1.reshape(-1)), np.ascontiguousarray(m2.reshape(-1))
        both = np.concatenate([f1, f2])
        ro = (np.arange(npairs + 1, dtype=np.uint64) * a.len).astype(np.uint32)
        ro2 = (np.arange(2 * npairs + 1, dtype=np.uint64) * a.len).astype(np.uint32)
        p = m.MapParams(e, 1, 0, 3)
        pp = m.PairParams(lo, hi, a.rescue)
        hits = np.zeros(2 * npairs, m.MAP_HIT_DTYPE)
        tlen = np.zeros(npairs, np.int32)
        nconc = np.zeros(npairs, np.uint32)
        ops = np.zeros(2 * npairs * 16, np.uint16)
        nops = np.zeros(2 * npairs, np.uint8)
        n_hits = np.zeros(2 * npairs, np.uint32)
        all_hits = np.zeros(2 * npairs, m.MAP_HIT_DTYPE)
        all_ops = np.zeros(2 * npairs * 16, np.uint16)
        all_nops = np.zeros(2 * npairs, np.uint8)
        P = max(a.all_hits, 1)
        strata = 2 * e if a.strata is None else a.strata
        n_pairs = np.zeros(npairs, np.uint32)
        pa_hits = np.zeros(npairs * P * 2, m.MAP_HIT_DTYPE) if a.all_hits else None
        pa_tlen = np.zeros(npairs * P, np.int32) if a.all_hits else None
        pa_nconc = np.zeros(npairs, np.uint32)
        pa_ops = np.zeros(npairs * P * 2 * 16, np.uint16) if a.all_hits else None
        pa_nops = np.zeros(npairs * P * 2, np.uint8) if a.all_hits else None
        best_pairs, best_all = 1e30, 1e30
        pairs_reps = []
        for _ in range(a.reps):  # alternating, so that both calls see the same machine state
            if a.all_hits:
                tm.start()
                eng._chk(lib.asm_map_pairs_all(h, ix, npairs, f1.ctypes.data, ro.ctypes.data, f2.ctypes.data, ro.ctypes.data,
                                               ctypes.byref(p), ctypes.byref(pp), strata, a.all_hits, n_pairs.ctypes.data,
                                               pa_hits.ctypes.data, pa_tlen.ctypes.data, pa_nconc.ctypes.data, pa_ops.ctypes.data, 16,
                                               pa_nops.ctypes.data))
                tm.stop()
                best_all = min(best_all, tm.elapsed_ms())
            tm.start()
            eng._chk(lib.asm_map_pairs(h, ix, npairs, f1.ctypes.data, ro.ctypes.data, f2.ctypes.data, ro.ctypes.data, ctypes.byref(p),
                                       ctypes.byref(pp), hits.ctypes.data, tlen.ctypes.data, nconc.ctypes.data, ops.ctypes.data, 16,
                                       nops.ctypes.data))
            tm.stop()
            best_pairs = min(best_pairs, tm.elapsed_ms())
            pairs_reps.append(round(tm.elapsed_ms(), 3))
            if a.all_hits:
                continue
            tm.start()
            eng._chk(lib.asm_map_reads_all(h, ix, 2 * npairs, both.ctypes.data, ro2.ctypes.data, ctypes.byref(p), e, 1,
                                           n_hits.ctypes.data, all_hits.ctypes.data, all_ops.ctypes.data, 16, all_nops.ctypes.data))
            tm.stop()
            best_all = min(best_all, tm.elapsed_ms())
        lib.asm_index_free(h, ix)
        if a.dump:
            dump_digests(a, e, {"pairs.hits": hits, "pairs.tlen": tlen, "pairs.n_concordant": nconc, "pairs.ops": ops, "pairs.nops": nops,
                                "pairs_all.n_pairs": n_pairs if a.all_hits else None, "pairs_all.hits": pa_hits, "pairs_all.tlen": pa_tlen,
                                "pairs_all.n_concordant": pa_nconc if a.all_hits else None, "pairs_all.ops": pa_ops,
                                "pairs_all.nops": pa_nops, "reads_all.n_hits": None if a.all_hits else n_hits,
                                "reads_all.hits": None if a.all_hits else all_hits, "reads_all.ops": None if a.all_hits else all_ops,
                                "reads_all.nops": None if a.all_hits else all_nops})
        fl = hits["flags"].reshape(npairs, 2)
        row = {"e": e, "mapq": a.mapq, "pairs_ms_events": round(best_pairs, 3), "pairs_ms_reps": pairs_reps, "pairs_per_s": round(npairs / best_pairs * 1e3),
               "all_hits1_ms_events": round(best_all, 3), "pairs_over_all_hits1": round(best_pairs / best_all, 3),
               "proper_fraction": round(float(((fl[:, 0] & m.MAP_PROPER_PAIR) != 0).mean()), 4),
               "rescued_fraction": round(float(((fl & m.MAP_RESCUED) != 0).any(axis=1).mean()), 4),
               "mates_mapped_fraction": round(float(((fl & m.MAP_MAPPED) != 0).mean()), 4),
               "n_concordant_gt1_fraction": round(float((nconc > 1).mean()), 4)}
        if a.all_hits:
            del row["all_hits1_ms_events"], row["pairs_over_all_hits1"]
            rep_n = np.minimum(n_pairs, a.all_hits)
            row.update({"all_hits": a.all_hits, "strata": strata, "pairs_all_ms_events": round(best_all, 3),
                        "pairs_all_per_s": round(npairs / best_all * 1e3), "pairs_all_over_pairs": round(best_all / best_pairs, 3),
                        "n_pairs_mean": round(float(n_pairs.mean()), 3), "reported_pairs_mean": round(float(rep_n.mean()), 3),
                        "secondary_pairs": int(np.maximum(rep_n.astype(np.int64) - 1, 0).sum()),
                        "rank0_equals_pairs": bool(np.array_equal(pa_nconc, nconc) and np.array_equal(
                            pa_hits.reshape(npairs, P, 2)[:, 0]["pos"], hits.reshape(npairs, 2)["pos"])),
                        # distribution of n_pairs: 0, 1, 2-3, 4-15, 16-63, >= 64
                        "n_pairs_hist": [int(v) for v in np.histogram(n_pairs, [0, 1, 2, 4, 16, 64, 2**32])[0]]})
        results["runs"].append(row)
        print(json.dumps(row))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_map_paired.json"), "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
