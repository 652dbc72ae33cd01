"""The pair aligners' fixed-width CIGAR rows: what a row must hold for a given oracle CIGAR and cap, and inputs whose rows fill.

A producer (CigarSink of the six Greedy families, nw_trace_cover_kernel<.., 32|64>, nw_trace_affine_kernel) stores the first
min(R, cap) entries of a pair's R runs as count << 3 | op and reports nops = min(R, 255): the count is a byte that saturates, so
nops > cap says "truncated" and nops == 255 says "255 or more".  expect_row states exactly that for an oracle CIGAR string; every
expectation of tests/test_gpu_cigar_rows.py and of the truncating runs in tests/test_greedy_lane_host.py is this function's.

Inputs are small: N_PAIRS = 1061 pairs, two full workgroups of 512 plus a ragged tail of 37.

Greedy saturation.  Greedy reads at most 128 characters of either string, so a Greedy CIGAR cannot have many runs: every 'M' run
takes a column and every switch sits between two of them.  tests/test_cigar_rows_host.py searches indel_comb (every edit applied) at
periods 1..8, lengths 100, 128, 200 and 511 and k in (1, 2, 3, 5, 10, 17, 32, 40) with the oracle: the largest R it finds is GREEDY_MAX_R_FOUND
below (asserted there), far from 255.  No Greedy input of at most 511 characters that reaches R >= 256 is known, so saturation is
tested on NW rows only (subst_comb(511): R = 511), and on the readers (cover_verdict, asm_cigar_format, decode_cigars) with
hand-made counts."""
import re

import numpy as np

OPS = "MID=X"
NOPS_MAX = 255
N_PAIRS = 1061
N_PAIRS_511 = 165  # the 511-character comb goes through the full matrix, 64 pairs a workgroup: two full ones and a tail of 37
GREEDY_MAX_R_FOUND = 98  # indel_comb(128, 2, ragged=False) at k = 1: the search of test_cigar_rows_host.py

_ACGT = "ACGT"


def encode(cigar):
    """The oracle's CIGAR string -> entries count << 3 | op (M I D = X -> 0 1 2 3 4) as Python ints in uint16 range"""
    runs = re.findall(r"(\d+)([MID=X])", cigar)
    if "".join(c + o for c, o in runs) != cigar:
        raise ValueError(f"not a CIGAR of M, I, D, = and X runs: {cigar!r}")
    out = [int(c) << 3 | OPS.index(o) for c, o in runs]
    if any(not 8 <= v <= 0xFFFF for v in out):
        raise ValueError(f"a run of {cigar!r} is empty or does not fit 13 bits")
    return out


def run_count(cigar):
    return len(encode(cigar))


def expect_row(cigar, cap, reverse=False):
    """-> (the first min(R, cap) entries a producer must store, the count it must report = min(R, 255)).  reverse: the entries in
    traceback order (last run first), as the NW kernels emit them."""
    row = encode(cigar)
    if reverse:
        row = row[::-1]
    return row[:min(len(row), cap)], min(len(row), NOPS_MAX)


def expect_matrix(cigars, reverse=False):
    """All rows at once for array comparisons: (uint16[n][max R] padded with 0, R int64[n])"""
    rows = [encode(c)[::-1] if reverse else encode(c) for c in cigars]
    R = np.array([len(r) for r in rows], np.int64)
    full = np.zeros((len(rows), max(int(R.max(initial=0)), 1)), np.uint16)
    for i, r in enumerate(rows):
        full[i, :len(r)] = r
    return full, R


def nw_cigar_wide(oracle, hb, x=1, o=1, e=1, stride=4096):
    """oracle.nw_cigar with room for a 511-run CIGAR (the binding's own stride holds 767 characters): (penalties, strings)"""
    from tests import oracle_binding as ob

    keep, args = ob._batch_args(hb)
    pen = np.zeros(hb.n, np.int32)
    cg = np.zeros(hb.n * stride + 1, np.uint8)
    assert oracle.lib.orc_nw_cigar_batch(*args, x, o, e, pen.ctypes.data, cg.ctypes.data, stride) == 0
    out = ob._cigars(cg, hb.n, stride)
    assert max(len(c) for c in out) < stride - 8  # nothing was cut
    return pen, out


def cap_ladder(R):
    """The caps every case runs at: 1, 2, median(R), max(R) - 1, max(R), max(R) + 1 (at least 1, each once, ascending)"""
    R = np.asarray(R)
    top = int(R.max())
    return sorted({max(1, c) for c in (1, 2, int(np.median(R)), top - 1, top, top + 1)})


def split_at(R, cap):
    """(share of rows truncated at cap, share not)"""
    R = np.asarray(R)
    return float((R > cap).mean()), float((R <= cap).mean())


def _random_text(rng, length):
    return "".join(_ACGT[i] for i in rng.integers(0, 4, length))


def _other(rng, c, avoid=""):
    """a base that is neither c nor in avoid"""
    pool = [b for b in _ACGT if b != c and b not in avoid]
    return pool[int(rng.integers(0, len(pool)))]


def noisy_c2(asm, n=N_PAIRS, err=0.30, first=17):
    """The C2 configuration (100 bp, generated the reference's way) at a high error rate: Greedy rows with a spread of run counts,
    NW distances on both sides of either window's margin"""
    cfg, _, _ = asm.workload("C2")
    cfg.err = err
    return asm.generate_pairs(cfg, first, n)


def indel_comb_pairs(length, period, n=N_PAIRS, seed=1, ragged=True):
    """The reference is the read with a one-base deletion and a one-base insertion alternating every `period` bases, so the lengths
    differ by at most one and the alignment stays inside the smallest band while the Greedy row collects I / D / M runs.  ragged:
    pair i stops editing at a point drawn uniformly from the string, which spreads the run counts from 1 to the full comb's."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        read = _random_text(rng, length)
        stop = int(rng.integers(0, length + 1)) if ragged else length
        ref, delete = [], True
        for p, c in enumerate(read):
            if p and p % period == 0 and p < stop:
                if delete:
                    delete = False
                    continue  # the reference lacks this base
                ref.append(_other(rng, c, avoid=ref[-1] if ref else ""))  # an extra base that matches neither neighbour
                delete = True
            ref.append(c)
        pairs.append((read, "".join(ref)))
    return pairs


def indel_comb(asm, length, period, n=N_PAIRS, seed=1, ragged=True):
    return asm.HostBatch.from_strings(indel_comb_pairs(length, period, n, seed, ragged))


def subst_comb_pairs(length, n=N_PAIRS, seed=2):
    """Every second base substituted: the NW row is 1=1X1=1X... with R = length.  The read is drawn from A and C and the substitutes
    from G and T, so none of the length // 2 substitutes matches any base of the read: each costs at least one, the diagonal costs
    exactly that, and a path with a gap pays for the gap on top (the lengths are equal, so a gap needs a second one).  The diagonal
    is the only optimal alignment under any penalties with x <= 2 * (o + e), whatever the tie-break."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        read = ["AC"[i] for i in rng.integers(0, 2, length)]
        ref = list(read)
        for p in range(1, length, 2):
            ref[p] = "GT"[int(rng.integers(0, 2))]
        pairs.append(("".join(read), "".join(ref)))
    return pairs


def subst_comb(asm, length, n=N_PAIRS, seed=2):
    return asm.HostBatch.from_strings(subst_comb_pairs(length, n, seed))


def sparse_subst_pairs(length, d, n=N_PAIRS, seed=3):
    """d substitutions spread evenly over the string (place (2j + 1) * length / (2d)): NW distance at most d, so d <= 13 stays within
    the window=32 pass's margin C - 3 = 13 and d <= 29 within the window=64 pass's (C = window / 2)."""
    rng = np.random.default_rng(seed)
    places = sorted({(2 * j + 1) * length // (2 * d) for j in range(d)})
    assert len(places) == d
    pairs = []
    for _ in range(n):
        read = _random_text(rng, length)
        ref = list(read)
        for p in places:
            ref[p] = _other(rng, read[p])
        pairs.append((read, "".join(ref)))
    return pairs


def sparse_subst(asm, length, d, n=N_PAIRS, seed=3):
    return asm.HostBatch.from_strings(sparse_subst_pairs(length, d, n, seed))


def ragged_129_256(asm, n=N_PAIRS, seed=53):
    """Reads of 129 to 256 characters with 12 % random edits: the second width class (two plane granules per string)"""
    from tests.util import random_ragged_batch

    return random_ragged_batch(asm, seed, n, 129, 256)


# ---- the cases of the GPU tests, stated once so that the CPU test can check the inputs they rely on ----
INPUTS = {"noisy_c2": noisy_c2, "ragged_129_256": ragged_129_256, "sparse12": lambda asm: sparse_subst(asm, 100, 12),
          "sparse28": lambda asm: sparse_subst(asm, 100, 28), "comb100": lambda asm: subst_comb(asm, 100),
          "comb511": lambda asm: subst_comb(asm, 511, n=N_PAIRS_511), "indel_comb": lambda asm: indel_comb(asm, 100, 9)}
GREEDY_INPUTS = ("noisy_c2", "ragged_129_256")
# (id, k, (x, o, e), greedy mode (1 clean / 0 sequential), engine switch turned off or None)
GREEDY_CASES = [("k3", 3, (1, 1, 1), 1, None), ("k3_sequential", 3, (1, 1, 1), 0, None), ("k10", 10, (1, 1, 1), 1, None),
                ("k17", 17, (1, 1, 1), 1, None), ("k32", 32, (1, 1, 1), 1, None), ("k40", 40, (1, 1, 1), 1, None),
                ("k20_wide", 20, (1, 1, 1), 1, "ASM_WAVE"), ("k16_231", 16, (2, 3, 1), 1, None), ("k17_231", 17, (2, 3, 1), 1, None)]
# (id, input, penalties, window): both tracebacks and both windows
NW_CASES = [("sparse12_w32", "sparse12", (1, 1, 1), 32), ("sparse28_w64", "sparse28", (1, 1, 1), 64),
            ("sparse28_w32_handed_over", "sparse28", (1, 1, 1), 32), ("comb100_w32", "comb100", (1, 1, 1), 32),
            ("comb100_w64", "comb100", (1, 1, 1), 64), ("comb511_w64", "comb511", (1, 1, 1), 64),
            ("ragged_129_256_w32", "ragged_129_256", (1, 1, 1), 32), ("ragged_129_256_w64", "ragged_129_256", (1, 1, 1), 64),
            ("noisy_c2_231", "noisy_c2", (2, 3, 1), 64)]
# coverage on truncated Greedy rows: (id, input, penalties, window) — banded and full-matrix verdicts, one and two granules
COVER_CASES = [("noisy_c2_banded_w64", "noisy_c2", (1, 1, 1), 64), ("noisy_c2_w32", "noisy_c2", (1, 1, 1), 32),
               ("noisy_c2_full_matrix_231", "noisy_c2", (2, 3, 1), 64), ("indel_comb_banded", "indel_comb", (1, 1, 1), 64),
               ("ragged_129_256_banded_w64", "ragged_129_256", (1, 1, 1), 64),
               ("ragged_129_256_full_matrix_231", "ragged_129_256", (2, 3, 1), 64)]
COVER_K = 3
