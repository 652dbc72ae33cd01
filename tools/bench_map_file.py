"""File-to-file read mapping timings (development tool):
PYTHONPATH=. python tools/bench_map_file.py --dir DIR [--ref-len 5e6] [--reads 1e6] [--len 100] [--errors 2] [--all-hits N]
[--reps 3] [--chunk-bytes N] [--profile] [--paired [--insert 200,500] [--rescue E]] [--sort] [--exe PATH] [--mapq reference|gap] [--md]
Writes the workload of tools/bench_map.py as files into DIR (seeded: a reference of --ref-len bases as ref.fa and --reads reads of
--len bases with qualities as reads.fq), then runs `asm-map` and `asm-map --stream` on them alternately, --reps times each, in this
one call.  For every run: the wall clock of the whole process (reference parsing and index build included, the same in both) and,
for --stream, the library's own split (whole asm_map_file call, reader busy, writer busy).  The comparison is always against the
same asm-map without --stream on the same files; the two SAM files must be identical apart from @PG.  The files are read once
before the first run, so every run finds them in the page cache; the SAM files go to DIR too.
--paired writes the paired workload of tools/bench_map.py --paired instead (--reads / 2 pairs, as r1.fq and r2.fq) and compares
`asm-map -1 -2` with `asm-map -1 -2 --stream-pairs`; the streamed runs also report the reader's carry_peak (from a library call of
its own on the same files, Engine.map_pairs_file).
--profile runs `asm-map --stream` (or --stream-pairs) once under `rocprofv3 --kernel-trace --stats` (a run of its own) and prints the kernel totals.
--sort times coordinate-sorted output instead (docs/design/mapper.md, "Sorted output"): in one process and on one index, the
unsorted and the sorted library call alternately, --reps times each after one warm-up of each, with the sort's own seconds and the
slabs; the sorted file is checked once against Python's stable sort of the unsorted one; and a device-to-device hipMemcpyAsync of as
many bytes as the gather kernel moves is timed with events, the yardstick for that kernel.  With --profile the traced run is
`asm-map --stream --sort`, whose kernel totals hold the sort's split (radix sort, scan, sam_line_gather_kernel).
--mapq gap runs every leg under ASM_MAPQ_GAP (asm-map --mapq gap, Engine.set_mapq_model): the price of the repeat- and pair-aware
MAPQ, whose best-hit calls take the runs path.  The default passes no option, so that --exe may name an older asm-map.
--md runs every leg with the MD:Z tag (asm-map --md, Engine.set_sam_tags): the price of the tag, which map_md_kernel builds on the
device in the streamed legs and asm_md_format on the host in the others.  The default passes no option, as for --mapq.
--exe PATH runs another build's asm-map in the tool legs (for a comparison of two builds on the same files)."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.bench_map import make_inputs, make_pairs  # noqa: E402

EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")


def write_fastq(path, reads, prefix, seed):
    n, m = reads.shape
    rng = np.random.default_rng(seed)
    names = np.char.add(prefix, np.arange(n).astype(str)).astype(bytes)
    quals = rng.integers(35, 74, (n, m), dtype=np.uint8)
    with open(path, "wb") as fh:
        for lo in range(0, n, 100_000):
            hi = min(n, lo + 100_000)
            fh.write(b"".join(names[t] + b"\n" + reads[t].tobytes() + b"\n+\n" + quals[t].tobytes() + b"\n" for t in range(lo, hi)))


def write_files(a, e):
    """-> the reference and the read files (one, or with --paired the two mates' files)"""
    ref, reads = make_inputs(int(a.ref_len), 1 if a.paired else int(a.reads), a.len, e, seed=1234)
    fa = os.path.join(a.dir, "ref.fa")
    with open(fa, "wb") as fh:
        fh.write(b">ref\n")
        body = np.full((ref.size + 69) // 70 * 71, 10, np.uint8).reshape(-1, 71)
        flat = np.zeros(body.shape[0] * 70, np.uint8)
        flat[:ref.size] = ref
        body[:, :70] = flat.reshape(-1, 70)
        out = body.reshape(-1)
        out = out[out != 0]
        fh.write(out.tobytes())
    if a.paired:
        lo, hi = (int(v) for v in a.insert.split(","))
        m1, m2 = make_pairs(ref, int(a.reads) // 2, a.len, e, lo, hi, seed=4321)
        fqs = [os.path.join(a.dir, "r1.fq"), os.path.join(a.dir, "r2.fq")]
        write_fastq(fqs[0], m1, "@frag", 99)
        write_fastq(fqs[1], m2, "@frag", 100)
        return fa, fqs
    fq = os.path.join(a.dir, "reads.fq")
    write_fastq(fq, reads, "@read", 99)
    return fa, [fq]


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("failed: %s\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    return wall, r.stderr


def body_of(path):
    with open(path, "rb") as fh:
        return [ln for ln in fh.read().split(b"\n") if not ln.startswith(b"@PG")]


def sort_leg(a, fqs, result):
    """the unsorted and the sorted library call, alternately; -> result"""
    import torch

    import approximate_string_matching_amd as m

    eng = m.Engine(0)
    eng.set_mapq_model(a.mapq)
    if a.md:
        eng.set_sam_tags(md=True)
    ref, _ = make_inputs(int(a.ref_len), 1, a.len, a.errors, seed=1234)
    ix = eng.build_index([ref.tobytes().decode()], k=12)
    sams = [os.path.join(a.dir, "lib_unsorted.sam"), os.path.join(a.dir, "lib_sorted.sam")]

    def call(sort):
        kw = dict(chunk_bytes=a.chunk_bytes, sort=sort)
        if a.paired:
            lo, hi = (int(v) for v in a.insert.split(","))
            return eng.map_pairs_file(ix, ["ref"], fqs[0], fqs[1], sams[sort], a.errors, lo, hi, rescue_errors=a.rescue, **kw)
        return eng.map_file(ix, ["ref"], fqs[0], sams[sort], a.errors, max_hits=a.all_hits, **kw)

    call(False), call(True)  # warm-up: code objects, the pool, pinned buffers
    with open(sams[0], "rb") as fh:
        lines = fh.read().split(b"\n")[:-1]

    def key(ln):
        c = ln.split(b"\t", 4)
        return (1 if c[2] == b"*" else 0, int(c[3]))

    with open(sams[1], "rb") as fh:
        result["sorted_is_python_sort"] = fh.read() == b"".join(ln + b"\n" for ln in sorted(lines, key=key))
    print("sorted file equals Python's stable sort of the unsorted file:", result["sorted_is_python_sort"], flush=True)
    result["pairs"] = []
    for rep in range(a.reps):
        st0, st1 = call(False), call(True)
        pair = {"unsorted_s": round(st0["seconds"], 4), "sorted_s": round(st1["seconds"], 4), "ratio": round(st1["seconds"] / st0["seconds"], 3),
                "sort_s": round(st1["sort"]["seconds_sort"], 4), "slabs": st1["sort"]["slabs"], "lines": st1["sort"]["lines"],
                "bytes_held": st1["sort"]["bytes_held"], "write_s": [round(st0["seconds_write"], 4), round(st1["seconds_write"], 4)]}
        result["pairs"].append(pair)
        print("pair %d: unsorted call %.4f s, sorted call %.4f s (x%.3f), of it sort to last slab %.4f s; %d lines, %d bytes held, %d slabs" %
              (rep, pair["unsorted_s"], pair["sorted_s"], pair["ratio"], pair["sort_s"], pair["lines"], pair["bytes_held"], pair["slabs"]), flush=True)
    # the yardstick of sam_line_gather_kernel: the same number of bytes, device to device, as one hipMemcpyAsync
    n = int(result["pairs"][-1]["bytes_held"])
    src, dst = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    times = []
    for _ in range(12):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        dst.copy_(src)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e-3)
    best = sorted(times[2:])
    result["d2d_memcpy"] = {"bytes": n, "median_s": best[len(best) // 2], "min_s": best[0], "gb_per_s": round(n / best[len(best) // 2] / 1e9, 1)}
    print("device-to-device copy of %d bytes: median %.6f s (%.1f GB/s)" % (n, result["d2d_memcpy"]["median_s"], result["d2d_memcpy"]["gb_per_s"]),
          flush=True)
    ix.free()
    eng.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="directory for the input and output files")
    ap.add_argument("--ref-len", type=float, default=5e6)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--errors", type=int, default=2)
    ap.add_argument("--all-hits", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--paired", action="store_true", help="asm-map -1 -2 against --stream-pairs on --reads / 2 simulated pairs")
    ap.add_argument("--insert", default="200,500", help="with --paired: MIN,MAX of the projected span")
    ap.add_argument("--rescue", type=int, default=-1, help="with --paired: mate rescue's error bound (-1: off)")
    ap.add_argument("--sort", action="store_true", help="the sorted library call against the unsorted one; with --profile: asm-map --stream --sort")
    ap.add_argument("--exe", default=EXE, help="the asm-map to run in the tool legs")
    ap.add_argument("--mapq", choices=["reference", "gap"], default="reference", help="the MAPQ model of every leg")
    ap.add_argument("--md", action="store_true", help="MD:Z on every leg")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    fa, fqs = write_files(a, a.errors)
    for path in [fa] + fqs:  # into the page cache
        with open(path, "rb") as fh:
            while fh.read(1 << 24):
                pass
    if a.paired:
        flags = ["-e", str(a.errors), "--insert", a.insert] + (["--rescue", str(a.rescue)] if a.rescue >= 0 else [])
        base = [a.exe, "-r", fa, "-1", fqs[0], "-2", fqs[1]] + flags
    else:
        flags = ["-e", str(a.errors), "--both-strands"] + (["--all-hits", str(a.all_hits)] if a.all_hits else [])
        base = [a.exe, "-r", fa, "-q", fqs[0]] + flags
    if a.mapq != "reference":
        base += ["--mapq", a.mapq]
    if a.md:
        base += ["--md"]
    stream = ["--stream-pairs" if a.paired else "--stream"] + (["--chunk-bytes", str(a.chunk_bytes)] if a.chunk_bytes else [])
    if a.sort and a.profile:
        stream.append("--sort")
    sam0, sam1 = os.path.join(a.dir, "plain.sam"), os.path.join(a.dir, "stream.sam")
    if a.profile:
        out = os.path.join(a.dir, "profile")
        os.makedirs(out, exist_ok=True)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "map_file", "--output-format", "csv", "--"] + base +
                       ["-o", sam1] + stream, check=True, timeout=1200)
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                rows = list(csv.DictReader(fh))
            print("kernel totals (", path, ")")
            for r in (rows if a.sort else rows[:40]):  # --sort: the sort's kernels are short and stand far down the list
                print("  %-60s calls %6s total %10.3f ms  avg %9.1f us" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6,
                                                                           float(r["AverageNs"]) / 1e3))
        return
    result = {"mapq": a.mapq, "md": a.md, "reads": int(a.reads), "len": a.len, "ref_len": int(a.ref_len), "errors": a.errors, "all_hits": a.all_hits,
              "paired": a.paired, "insert": a.insert if a.paired else None, "rescue": a.rescue if a.paired else None,
              "fastq_bytes": sum(os.path.getsize(fq) for fq in fqs), "page_cache": True, "pairs": []}
    if a.sort:
        print(json.dumps(sort_leg(a, fqs, result)))
        return
    for rep in range(a.reps):
        w0, err0 = run(base + ["-o", sam0])
        w1, err1 = run(base + ["-o", sam1] + stream)
        mt = re.search(r"([\d.]+) s \(reader busy ([\d.]+) s, writer busy ([\d.]+) s\)", err1)
        pair = {"plain_s": round(w0, 3), "stream_s": round(w1, 3), "ratio": round(w0 / w1, 2), "call_s": float(mt.group(1)),
                "read_s": float(mt.group(2)), "write_s": float(mt.group(3)), "faster": w1 < w0}
        result["pairs"].append(pair)
        print("pair %d: asm-map %.3f s, asm-map %s %.3f s (x%.2f); library call %.3f s, reader busy %.3f s, writer busy %.3f s" %
              (rep, w0, stream[0], w1, w0 / w1, pair["call_s"], pair["read_s"], pair["write_s"]), flush=True)
        if rep == 0:
            result["sam_bytes"] = os.path.getsize(sam1)
            result["identical"] = body_of(sam0) == body_of(sam1)
            result["summary"] = err1.splitlines()[0]
            print("SAM files identical apart from @PG:", result["identical"], flush=True)
    result["all_faster"] = all(p["faster"] for p in result["pairs"])
    if a.paired:  # the reader's carry, which the tool does not print: one library call on the same files
        import approximate_string_matching_amd as m

        eng = m.Engine(0)
        eng.set_mapq_model(a.mapq)
        if a.md:
            eng.set_sam_tags(md=True)
        ref, _ = make_inputs(int(a.ref_len), 1, a.len, a.errors, seed=1234)
        ix = eng.build_index([ref.tobytes().decode()], k=12)
        lo, hi = (int(v) for v in a.insert.split(","))
        st = eng.map_pairs_file(ix, ["ref"], fqs[0], fqs[1], sam1, a.errors, lo, hi, rescue_errors=a.rescue, chunk_bytes=a.chunk_bytes)
        result["library"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}
        ix.free()
        eng.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
