"""Compressed-input timings of asm_map_file (development tool; docs/design/mapper.md, "Compressed input"):
PYTHONPATH=. python tools/bench_map_file_gz.py --dir DIR [--ref-len 5e6] [--reads 1e6] [--len 100] [--errors 2] [--reps 9] [--profile]
Writes the workload of tools/bench_map_file.py into DIR (seeded: ref.fa, reads.fq) and reads.fq.gz: the same text in BGZF members
of 65 280 bytes, each deflated by zlib at level 6.  Then, in this one process and on one index:
- one host thread's zlib inflate of reads.fq.gz (member by member, best and all of 3), what a caller pays today in front of the plain call;
- Engine.map_file on reads.fq and on reads.fq.gz alternately, one warm-up each, --reps repeats each: the call's own seconds;
- Engine.bgzf_decompress of the whole file (host memory in and out), for scale.
The two SAM files must be identical.  The files are read once before the first run, so every run finds them in the page cache.
Prints one JSON line.  --profile instead runs `asm-map --stream` on reads.fq.gz once under `rocprofv3 --kernel-trace --stats`, a run
of its own with no counters, and prints the kernel totals.
--paired [--insert 200,500] [--levels 6,6] does the same for asm_map_pairs_file (docs/design/mapper.md, "Compressed input for pairs"):
the paired workload of tools/bench_map_file.py --paired as r1.fq, r2.fq and r1.fq.gz, r2.fq.gz (zlib at --levels, one per file),
Engine.map_pairs_file on the two text files and on the two BGZF files alternately, the outputs identical apart from @PG, one thread's
zlib over both .gz files, and carry_peak of both legs.  --paired --ab BASE.so instead times the plain-text paired call under BASE.so
and under this tree's library alternately, each run in a fresh process (the library's path is read at import), as tools/ab_lib.py
does for the aligners: the text path is meant to cost what it cost."""
import argparse
import csv
import glob
import json
import os
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.bench_map_file import EXE, write_files  # noqa: E402

PAYLOAD = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzip(text, level=6):
    out = []
    for at in range(0, len(text), PAYLOAD):
        part = text[at:at + PAYLOAD]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = z.compress(part) + z.flush()
        out.append(bytes.fromhex("1f8b08040000000000ff0600424302") + b"\0" + struct.pack("<H", len(raw) + 25) + raw +
                   struct.pack("<II", zlib.crc32(part), len(part)))
    return b"".join(out) + EOF_BLOCK


def members(data):
    at = 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        yield data[at + 18:at + size - 8]
        at += size


PLAIN_CHILD = r"""
import json, sys
import approximate_string_matching_amd as asm
fa, f1, f2, out, e, lo, hi, reps = sys.argv[1:9]
eng = asm.Engine(0)
ix, _ = eng.build_index_file(fa, k=12)
times = [eng.map_pairs_file(ix, ix.names, f1, f2, out, int(e), int(lo), int(hi))["seconds"] for _ in range(int(reps) + 1)]
print(json.dumps(times[1:]))
"""


def median(v):
    return sorted(v)[len(v) // 2]


def paired(a):
    a.paired = True
    fa, fqs = write_files(a, a.errors)
    lo, hi = (int(v) for v in a.insert.split(","))
    levels = [int(v) for v in a.levels.split(",")]
    texts = [open(f, "rb").read() for f in fqs]
    gzs = ["%s.l%d.gz" % (f, lv) for f, lv in zip(fqs, levels)]
    for f, text, lv in zip(gzs, texts, levels):
        if not os.path.exists(f):
            with open(f, "wb") as fh:
                fh.write(bgzip(text, lv))
    datas = [open(f, "rb").read() for f in gzs]
    if a.ab:
        libs = {"base": os.path.abspath(a.ab), "new": os.path.join(ROOT, "approximate-string-matching_amd", "libasm_mi355x.so")}
        times = {k: [] for k in libs}
        for _ in range(a.rounds):
            for k, lib in libs.items():
                r = subprocess.run([sys.executable, "-c", PLAIN_CHILD, fa, fqs[0], fqs[1], os.path.join(a.dir, "ab_%s.sam" % k), str(a.errors),
                                    str(lo), str(hi), str(a.reps)], capture_output=True, text=True, timeout=1200,
                                   env=dict(os.environ, ASM_MI355X_LIB=lib, PYTHONPATH=ROOT))
                if r.returncode != 0:
                    raise SystemExit("failed under %s:\n%s" % (lib, r.stderr[-2000:]))
                times[k] += json.loads(r.stdout.strip().split("\n")[-1])
        same = open(os.path.join(a.dir, "ab_base.sam"), "rb").read() == open(os.path.join(a.dir, "ab_new.sam"), "rb").read()
        print(json.dumps({"ab_plain_pairs": True, "pairs": int(a.reads) // 2, "same_sam": same,
                          "base_s": [round(v, 4) for v in times["base"]], "new_s": [round(v, 4) for v in times["new"]],
                          "base_median_s": round(median(times["base"]), 4), "new_median_s": round(median(times["new"]), 4),
                          "new_inside_base_spread": min(times["base"]) <= median(times["new"]) <= max(times["base"])}))
        return
    import approximate_string_matching_amd as asm

    inflate = []
    for _ in range(3):
        t0 = time.perf_counter()
        total = sum(len(zlib.decompress(m, wbits=-15)) for d in datas for m in members(d))
        inflate.append(time.perf_counter() - t0)
    assert total == len(texts[0]) + len(texts[1])
    eng = asm.Engine(0)
    ix, _ = eng.build_index_file(fa, k=12)
    legs = {"plain": (fqs, os.path.join(a.dir, "plain_pairs.sam")), "gz": (gzs, os.path.join(a.dir, "gz_pairs.sam"))}
    times, stats = {"plain": [], "gz": []}, {}
    for rep in range(a.reps + 1):                       # rep 0: the warm-up of each leg
        for leg, (src, dst) in legs.items():
            st = eng.map_pairs_file(ix, ix.names, src[0], src[1], dst, a.errors, lo, hi, chunk_bytes=a.chunk_bytes)
            if rep:
                times[leg].append(st["seconds"])
            stats[leg] = st
    body = [[ln for ln in open(dst, "rb").read().split(b"\n") if not ln.startswith(b"@PG")] for _, dst in legs.values()]
    bound = min(times["plain"]) + min(inflate)
    chunk = a.chunk_bytes or 16 << 20
    print(json.dumps({
        "paired": True, "pairs": int(a.reads) // 2, "levels": levels, "text_bytes": [len(t) for t in texts], "gz_bytes": [len(d) for d in datas],
        "members": [sum(1 for _ in members(d)) for d in datas], "same_sam": body[0] == body[1],
        "zlib_inflate_s": [round(v, 4) for v in inflate], "plain_s": [round(v, 4) for v in times["plain"]],
        "gz_s": [round(v, 4) for v in times["gz"]], "plain_median_s": round(median(times["plain"]), 4), "gz_median_s": round(median(times["gz"]), 4),
        "gz_over_plain_median": round(median(times["gz"]) / median(times["plain"]), 3),
        "gz_over_zlib_plus_plain_median": round(median(times["gz"]) / (median(times["plain"]) + median(inflate)), 3),
        "fastest_plain_plus_inflate_s": round(bound, 4), "every_gz_below_it": max(times["gz"]) < bound,
        "chunks": {k: v["chunks"] for k, v in stats.items()}, "carry_peak": {k: v["carry_peak"] for k, v in stats.items()},
        # the design section's bound: six chunks between reader and cut, each less than chunk + one member a file, and a record a file
        "carry_bound": 6 * (chunk + 2 * 65536) + 2 * (2 * a.len + 64),
        "reader_busy_s": {k: round(v["seconds_read"], 4) for k, v in stats.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--ref-len", type=float, default=5e6)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--errors", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--paired", action="store_true", help="asm_map_pairs_file on two text files against two BGZF files")
    ap.add_argument("--insert", default="200,500", help="with --paired: MIN,MAX of the projected span")
    ap.add_argument("--levels", default="6,6", help="with --paired: zlib's level for r1 and for r2")
    ap.add_argument("--chunk-bytes", type=int, default=0, help="with --paired: chunk_bytes of both legs (0: the library's 16 MiB)")
    ap.add_argument("--ab", default=None, help="with --paired: BASE.so, time the plain-text paired call under it and under this tree's library")
    ap.add_argument("--rounds", type=int, default=3, help="with --ab: fresh processes per library")
    a = ap.parse_args()
    if a.paired:
        return paired(a)
    a.paired = False
    os.makedirs(a.dir, exist_ok=True)
    fa, (fq,) = write_files(a, a.errors)
    gz = fq + ".gz"
    text = open(fq, "rb").read()
    if not os.path.exists(gz):
        with open(gz, "wb") as fh:
            fh.write(bgzip(text))
    data = open(gz, "rb").read()
    nmembers = sum(1 for _ in members(data))
    if a.profile:
        out = os.path.join(a.dir, "profile_gz")
        os.makedirs(out, exist_ok=True)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "map_file_gz", "--output-format", "csv", "--", EXE, "-r", fa, "-q",
                        gz, "-e", str(a.errors), "--both-strands", "--stream", "-o", os.path.join(a.dir, "profile.sam")], check=True, timeout=1200)
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                rows = list(csv.DictReader(fh))
            print("kernel totals (", path, "); %d members, %d text bytes, %d compressed bytes" % (nmembers, len(text), len(data)))
            for r in rows[:40]:
                print("  %-60s calls %6s total %10.3f ms  avg %9.1f us" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6,
                                                                           float(r["AverageNs"]) / 1e3))
        return
    import approximate_string_matching_amd as asm

    inflate = []
    for _ in range(3):
        t0 = time.perf_counter()
        total = sum(len(zlib.decompress(m, wbits=-15)) for m in members(data))
        inflate.append(time.perf_counter() - t0)
    assert total == len(text)
    eng = asm.Engine(0)
    ix, _ = eng.build_index_file(fa, k=12)
    legs = {"plain": (fq, os.path.join(a.dir, "plain.sam")), "gz": (gz, os.path.join(a.dir, "gz.sam"))}
    times = {"plain": [], "gz": []}
    stats = {}
    for rep in range(a.reps + 1):                       # rep 0: the warm-up of each leg
        for leg, (src, dst) in legs.items():
            st = eng.map_file(ix, ix.names, src, dst, a.errors)
            if rep:
                times[leg].append(st["seconds"])
            stats[leg] = st
    same = open(legs["plain"][1], "rb").read() == open(legs["gz"][1], "rb").read()
    dec = []
    for _ in range(4):
        t0 = time.perf_counter()
        got = eng.bgzf_decompress(data)
        dec.append(time.perf_counter() - t0)
    assert got == text
    bound = min(times["plain"]) + min(inflate)
    print(json.dumps({
        "reads": int(a.reads), "text_bytes": len(text), "gz_bytes": len(data), "members": nmembers, "same_sam": same,
        "zlib_inflate_s": [round(v, 4) for v in inflate], "plain_s": [round(v, 4) for v in times["plain"]],
        "gz_s": [round(v, 4) for v in times["gz"]], "gz_over_plain_median": round(sorted(times["gz"])[len(times["gz"]) // 2] /
                                                                                 sorted(times["plain"])[len(times["plain"]) // 2], 3),
        "fastest_plain_plus_inflate_s": round(bound, 4), "every_gz_below_it": max(times["gz"]) < bound,
        "chunks": {k: v["chunks"] for k, v in stats.items()}, "reader_busy_s": {k: round(v["seconds_read"], 4) for k, v in stats.items()},
        "bgzf_decompress_s": [round(v, 4) for v in dec]}))


if __name__ == "__main__":
    main()
