"""Same-box A/B of the two streamed-file calls across builds of the library (development tool, GPU box):
    PYTHONPATH=. python tools/ab_stream.py --dir DIR --out FILE NAME=BUILD_DIR [NAME=BUILD_DIR ...]
BUILD_DIR holds libasm_mi355x.so and asm-map of one build (asm-map finds the library next to itself); the LAST one named is the
result, the others are copies of the parent.  Workloads: the FASTQ of tools/bench_map_file.py through `asm-map --stream` (best hit
and --all-hits 16) and the pair file of tools/bench_host_path.py through Engine.stream_seq_file (clean and sequential).
First the outputs: SAM bodies (apart from @PG) and, for stream_seq_file, SHA-256 of the penalty arrays, the counters, pairs,
max_length and chunks, at the default chunk size and at 1 MiB, first parent against result.  Then the timings: a fresh process per
(build, workload, round), builds alternating, --rounds rounds; margin per metric = max - min of all parent values (all copies
pooled); verdict: result median <= parent median + margin."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEQ_CHILD = r"""
import hashlib, json, sys
import approximate_string_matching_amd as m
path, mode, chunk, reps, n = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
eng = m.Engine(0)
_, _, p = m.workload("C2")
best = None
for it in range(reps):
    res, st = eng.stream_seq_file(path, p, m.GREEDY_CLEAN if mode == "clean" else m.GREEDY_SEQUENTIAL, chunk_bytes=chunk, capacity=n)
    if reps == 1 or (it and (best is None or st.seconds < best.seconds)):
        best = st
out = {"seconds": best.seconds, "seconds_read": best.seconds_read, "pairs": best.pairs, "chunks": best.chunks,
       "max_length": best.max_length, "counters": list(best.counters)}
for a, v in sorted(res.items()):
    out["sha_%d" % a] = hashlib.sha256(v[:best.pairs].tobytes()).hexdigest()
print(json.dumps(out))
"""


def seq_run(build, path, mode, chunk, reps, n):
    env = dict(os.environ, ASM_MI355X_LIB=os.path.join(build, "libasm_mi355x.so"), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", SEQ_CHILD, path, mode, str(chunk), str(reps), str(n)], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise SystemExit("stream_seq_file child failed (%s): %s" % (build, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def map_run(build, fa, fq, sam, all_hits, chunk):
    cmd = [os.path.join(build, "asm-map"), "-r", fa, "-q", fq, "-e", "2", "--both-strands", "-o", sam, "--stream"]
    cmd += (["--all-hits", str(all_hits)] if all_hits else []) + (["--chunk-bytes", str(chunk)] if chunk else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("failed: %s\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    mt = re.search(r"([\d.]+) s \(reader busy ([\d.]+) s, writer busy ([\d.]+) s\)", r.stderr)
    return {"call_s": float(mt.group(1)), "read_s": float(mt.group(2))}


def sam_body(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(b"\n".join(ln for ln in fh.read().split(b"\n") if not ln.startswith(b"@PG"))).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=float, default=4e6)
    ap.add_argument("builds", nargs="+")
    a = ap.parse_args()
    builds = [(b.split("=", 1)[0], os.path.abspath(b.split("=", 1)[1])) for b in a.builds]
    parents, result = builds[:-1], builds[-1]
    os.makedirs(a.dir, exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the two files
    from tools.bench_map_file import write_files
    fa, (fq,) = write_files(types.SimpleNamespace(dir=a.dir, ref_len=5e6, reads=1e6, len=100, paired=False), 2)
    import approximate_string_matching_amd as m
    n = int(a.pairs)
    seq = os.path.join(a.dir, "pairs_C2_%d.seq" % n)
    cfg, _, _ = m.workload("C2")
    with open(seq, "wb") as fh:
        for lo in range(0, n, 500_000):
            part = m.generate_pairs(cfg, lo, min(500_000, n - lo))
            fh.write(b"".join((">%s\n<%s\n" % part.pair(i)).encode() for i in range(part.n)))
    for path in (fa, fq, seq):  # into the page cache
        with open(path, "rb") as fh:
            while fh.read(1 << 24):
                pass

    # ---- outputs, first parent against result
    say("# outputs: %s against %s" % (parents[0][0], result[0]))
    same = True
    for all_hits in (0, 16):
        for chunk in (0, 1 << 20):
            sha = []
            for name, build in (parents[0], result):
                sam = os.path.join(a.dir, "%s.sam" % name)
                map_run(build, fa, fq, sam, all_hits, chunk)
                sha.append(sam_body(sam))
            same &= sha[0] == sha[1]
            say("outputs asm-map --stream all_hits=%-2d chunk=%-8s SAM apart from @PG: %s" % (all_hits, chunk or "default",
                                                                                           "identical" if sha[0] == sha[1] else "DIFFERENT"))
    for mode in ("clean", "sequential"):
        for chunk in (0, 1 << 20):
            got = [seq_run(build, seq, mode, chunk, 1, n) for _, build in (parents[0], result)]
            keys = [k for k in got[0] if k not in ("seconds", "seconds_read")]
            diff = [k for k in keys if got[0][k] != got[1][k]]
            same &= not diff
            say("outputs stream_seq_file %-10s chunk=%-8s pairs %d chunks %d max_length %d, 3 penalty arrays + counters: %s" % (
                mode, chunk or "default", got[1]["pairs"], got[1]["chunks"], got[1]["max_length"], "identical" if not diff else "DIFFERENT " + ",".join(diff)))

    # ---- timings
    vals = {}
    for rnd in range(a.rounds):
        for name, build in builds:
            for all_hits in (0, 16):
                r = map_run(build, fa, fq, os.path.join(a.dir, "ab.sam"), all_hits, 0)
                for k, v in r.items():
                    vals.setdefault(("asm-map --stream all_hits=%d" % all_hits, k), {}).setdefault(name, []).append(v)
            for mode in ("clean", "sequential"):
                r = seq_run(build, seq, mode, 0, 3, n)
                for k in ("seconds", "seconds_read"):
                    vals.setdefault(("stream_seq_file %s" % mode, k), {}).setdefault(name, []).append(r[k])
    say("")
    say("# timings, s; median [min .. max]; %d rounds" % a.rounds)
    ok_all = True
    for (work, metric), by in sorted(vals.items()):
        pooled = [v for name, _ in parents for v in by[name]]
        margin = max(pooled) - min(pooled)
        pmed, rmed = statistics.median(by[parents[0][0]]), statistics.median(by[result[0]])
        ok = rmed <= pmed + margin
        ok_all &= ok
        cols = "  ".join("%-8s %8.4f [%8.4f .. %8.4f]" % (name, statistics.median(by[name]), min(by[name]), max(by[name])) for name, _ in builds)
        say("%-32s %-13s %s  margin %7.4f  result-parent %+8.4f  %s" % (work, metric, cols, margin, rmed - pmed, "ok" if ok else "OVER"))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if same and ok_all else 1)


if __name__ == "__main__":
    main()
