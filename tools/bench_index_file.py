#!/usr/bin/env python3
"""From a FASTA file to the mapper's index: the host parse asm-map does plus asm_index_build, against asm_index_build_file
(docs/design/mapper.md, "Reference: FASTA in, index out").  Writes a seeded reference of --mbp Mbp in --seqs sequences twice, with
60-column lines and unwrapped, and for each file runs `asm-map --bench-ref`, which builds the index both ways alternately in one
process; the file is in the page cache (it has just been written, and one untimed read comes first).  Prints the best of --reps per
path and file as a table and as one JSON line.

    python tools/bench_index_file.py [--mbp 200] [--seqs 24] [--reps 3] [--k 12] [--dir DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")


def write_reference(path, seqs, width):
    """seqs: uint8 arrays; width 0: one line per sequence"""
    with open(path, "wb") as fh:
        for r, s in enumerate(seqs):
            fh.write(b">chr%d synthetic sequence %d\n" % (r + 1, r + 1))
            if width:
                whole = s.size // width * width
                lines = np.empty((whole // width, width + 1), np.uint8)
                lines[:, :width] = s[:whole].reshape(-1, width)
                lines[:, width] = 10
                fh.write(lines.tobytes())
                if whole < s.size:
                    fh.write(s[whole:].tobytes() + b"\n")
            else:
                fh.write(s.tobytes() + b"\n")


def run(path, reps, k):
    with open(path, "rb") as fh:  # into the page cache
        while fh.read(1 << 24):
            pass
    r = subprocess.run([EXE, "-r", path, "--bench-ref", str(reps), "--k", str(k)], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit("asm-map --bench-ref failed: " + r.stderr[-2000:])
    rows = {"host": [], "file": []}
    for line in r.stdout.splitlines():
        f = line.split()
        rows[f[0]].append({f[i]: float(f[i + 1]) for i in range(1, len(f), 2)})
    return {kind: min(v, key=lambda x: x["seconds"]) for kind, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=200.0)
    ap.add_argument("--seqs", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    total = int(a.mbp * 1e6)
    cuts = np.sort(rng.choice(np.arange(1, total), a.seqs - 1, replace=False)) if a.seqs > 1 else np.array([], np.int64)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total, dtype=np.uint8)]
    seqs = np.split(bases, cuts)
    out = {"mbp": a.mbp, "seqs": a.seqs, "k": a.k, "reps": a.reps, "files": {}}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for label, width in (("60 columns", 60), ("unwrapped", 0)):
            path = os.path.join(tmp, "ref.fa")
            write_reference(path, seqs, width)
            best = run(path, a.reps, a.k)
            best["file_bytes"] = os.path.getsize(path)
            out["files"][label] = best
            os.remove(path)
    print("%-12s %28s %44s %8s" % ("lines", "(a) host parse + index_build", "(b) asm_index_build_file", "(a)/(b)"))
    for label, b in out["files"].items():
        h, f = b["host"], b["file"]
        print("%-12s %8.3f s (parse %6.3f, build %5.3f) %8.3f s (reader busy %5.3f, index stage %5.3f, %3d chunks) %7.2fx" % (
            label, h["seconds"], h["parse"], h["index_build"], f["seconds"], f["reader_busy"], f["index_stage"], int(f["chunks"]),
            h["seconds"] / f["seconds"]))
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
