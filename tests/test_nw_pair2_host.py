"""Host logic of the banded unit-cost NW sweeps (csrc/asm_nwband.h): nw_band<4, 32>, nw_band<4, 64> and the two-pairs-per-dword
nw_band2x16<4>, compiled for the CPU (host/nw_host_check.cpp, the packed 16-bit operations in plain C++) and diffed against
the oracle's NW.  What is checked: a window reports a value only when it is the distance and within 2(C-1) - |n-m|; one
half of the dword never sees the other; and the 16-row pass really settles the benchmark's pairs.  No GPU needed; the
kernel around it is in test_gpu_nw_pair2.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
SO = os.path.join(PKG, "libnw_hostcheck.so")
_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def nwh():
    subprocess.check_call(["make", "-s", "-C", PKG, "nwcheck"])
    lib = ctypes.CDLL(SO)
    lib.nw_host_band.argtypes = [ctypes.c_long, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]
    lib.nw_host_pair2.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp]
    lib.nw_host_full.argtypes = [ctypes.c_long, _vp, _vp, _vp, _vp, _vp]
    return lib


def _strings(hb):
    keep = tuple(np.ascontiguousarray(a, t) for a, t in ((hb.reads, np.uint8), (hb.read_off, np.uint32), (hb.refs, np.uint8),
                                                         (hb.ref_off, np.uint32)))
    return keep, [a.ctypes.data for a in keep]


def band(nwh, hb, W):
    keep, s = _strings(hb)
    out = np.zeros(hb.n, np.int32)
    assert nwh.nw_host_band(hb.n, *s, W, out.ctypes.data) == 0
    return out


def full(nwh, hb):
    keep, s = _strings(hb)
    out = np.zeros(hb.n, np.int32)
    assert nwh.nw_host_full(hb.n, *s, out.ctypes.data) == 0
    return out


def pair2(nwh, hb, ip, iq):
    """The two halves' raw results for the couples (ip[j], iq[j])."""
    keep, s = _strings(hb)
    ip, iq = np.ascontiguousarray(ip, np.int64), np.ascontiguousarray(iq, np.int64)
    rp, rq = np.zeros(len(ip), np.int32), np.zeros(len(ip), np.int32)
    assert nwh.nw_host_pair2(*s, len(ip), ip.ctypes.data, iq.ctypes.data, rp.ctypes.data, rq.ctypes.data) == 0
    return rp, rq


def half16(nwh, hb):
    """Every pair's 16-row result with the kernel's packing in small: pair 2j low, pair 2j+1 high (an odd last pair with itself)."""
    idx = np.arange(hb.n)
    ip, iq = idx[0::2], idx[1::2]
    if len(iq) < len(ip):
        iq = np.append(iq, ip[-1])
    rp, rq = pair2(nwh, hb, ip, iq)
    out = np.zeros(hb.n, np.int32)
    out[0::2] = rp
    out[1::2] = rq[:hb.n // 2]
    return out


def edited_pairs(rng, count, lo, hi, edits_lo, edits_hi, sub_share):
    """(read, reference) strings over ACGT: the reference is the read after `edits` random edits, a share of them substitutions
    and the rest insertions and deletions in equal parts; both stay within 1..128 bases."""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for _ in range(count):
        a = acgt[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))]
        b = list(a)
        for _ in range(int(rng.integers(edits_lo, edits_hi + 1))):
            u = rng.random()
            if u < sub_share:
                p = int(rng.integers(0, len(b)))
                b[p] = acgt[(int(np.searchsorted(acgt, b[p])) + int(rng.integers(1, 4))) % 4]  # A < C < G < T: always another base
            elif (u < sub_share + (1 - sub_share) / 2 and len(b) > 1) or len(b) >= 128:
                del b[int(rng.integers(0, len(b)))]
            else:
                b.insert(int(rng.integers(0, len(b) + 1)), acgt[rng.integers(0, 4)])
        pairs.append((bytes(a).decode(), bytes(bytearray(int(c) for c in b)).decode()))
    return pairs


def check_halves(hb, h16, want):
    m, n = hb.lengths()
    told = h16 >= 0
    assert np.array_equal(h16[told], want[told])
    assert (h16[told] <= 14 - np.abs(n - m)[told]).all()
    return told


def cascade(nwh, hb, h16):
    """What the kernel stores: 16 rows, else 32, else 64, else the full height."""
    out = h16.copy()
    for stage in (band(nwh, hb, 32), band(nwh, hb, 64), full(nwh, hb)):
        out = np.where(out >= 0, out, stage)
    return out


@pytest.mark.parametrize("sub_share", [0.0, 0.5, 0.96, 1.0])
def test_seeded_batches_match_the_oracle(nwh, asm, oracle, sub_share):
    """Lengths 1-128, 0-20 edits, couples of every mix of lengths: whatever a half reports is the distance and within its
    bound, and the cascade's penalty is the oracle's for every pair."""
    rng = np.random.default_rng(int(sub_share * 100) + 7)
    pairs = edited_pairs(rng, 1500, 1, 128, 0, 20, sub_share)
    # partners of very different and of equal length, side by side
    pairs += edited_pairs(rng, 1, 1, 1, 0, 1, sub_share) + edited_pairs(rng, 1, 128, 128, 0, 20, sub_share)
    pairs += edited_pairs(rng, 1, 100, 100, 0, 10, sub_share) + edited_pairs(rng, 1, 37, 37, 0, 10, sub_share)
    pairs += edited_pairs(rng, 2, 64, 64, 3, 3, 1.0) + edited_pairs(rng, 2, 128, 128, 0, 0, 1.0)
    for la, lb in ((1, 128), (128, 1), (8, 9), (7, 120), (16, 17), (15, 96), (96, 95), (112, 113), (2, 2)):
        pairs += edited_pairs(rng, 1, la, la, 0, 4, sub_share) + edited_pairs(rng, 1, lb, lb, 0, 4, sub_share)
    hb = asm.HostBatch.from_strings(pairs)
    want = oracle.nw(hb)
    h16 = half16(nwh, hb)
    told = check_halves(hb, h16, want)
    assert told.mean() > 0.3  # the batch does exercise the 16-row pass (most pairs here have few edits for their length)
    assert np.array_equal(cascade(nwh, hb, h16), want)


def test_a_half_never_sees_its_partner(nwh, asm, oracle):
    """Carry isolation: a fixed pair gives the same 16-row result whichever partner shares its dword, in either half.  All-'A'
    against all-'A' makes Eq and VP all ones (the longest carry chains of the add), all-'A' against all-'C' has no match at all."""
    rng = np.random.default_rng(11)
    fixed = [("A" * 100, "A" * 100), ("A" * 128, "A" * 128), ("A" * 100, "C" * 100), ("A" * 12, "C" * 12), ("A" * 128, "A" * 120),
             ("A" * 16, "A" * 16), ("A" * 1, "A" * 1)] + edited_pairs(rng, 5, 90, 128, 2, 10, 0.9)
    partners = (edited_pairs(rng, 300, 1, 128, 0, 20, 0.7) + [("A" * L, "A" * L) for L in (1, 15, 16, 17, 100, 127, 128)] +
                [("T" * L, "T" * L) for L in (16, 100, 128)] + [("A" * L, "C" * L) for L in (5, 16, 100)])
    hb = asm.HostBatch.from_strings(fixed + partners)
    want = oracle.nw(hb)
    nf = len(fixed)
    alone = half16(nwh, asm.HostBatch.from_strings([p for p in fixed for _ in (0, 1)]))[0::2]  # each with itself
    assert (alone[:4] == [0, 0, -1, 12]).all()  # 100 mismatches are beyond 14; 12 are not
    for f in range(nf):
        others = np.arange(nf, hb.n)
        me = np.full(len(others), f)
        low, q_of_low = pair2(nwh, hb, me, others)
        p_of_high, high = pair2(nwh, hb, others, me)
        assert (low == alone[f]).all() and (high == alone[f]).all(), fixed[f]
        # and the partners are what they are next to anybody
        for got in (q_of_low, p_of_high):
            told = got >= 0
            assert np.array_equal(got[told], want[others][told])
        assert np.array_equal(q_of_low, p_of_high)


@pytest.mark.parametrize("W", [32, 64])
def test_the_bound_of_the_wide_windows(nwh, asm, oracle, W):
    """16-30 edits at 100-128 bases: every result a window accepts is the distance and within 2(C-1) - |n-m|, and the 32-row
    window now accepts results above the old limit of 15."""
    rng = np.random.default_rng(W)
    pairs = edited_pairs(rng, 1500, 100, 128, 16, 30, 0.5) + edited_pairs(rng, 1500, 100, 128, 16, 30, 0.96)
    hb = asm.HostBatch.from_strings(pairs)
    want = oracle.nw(hb)
    m, n = hb.lengths()
    got = band(nwh, hb, W)
    told = got >= 0
    assert np.array_equal(got[told], want[told])
    assert (got[told] <= W - 2 - np.abs(n - m)[told]).all()
    if W == 32:
        assert (got[told] > 15).sum() > 100
    # nothing within the bound is turned away when its end cell is in the window
    assert told[(want <= W - 2 - np.abs(n - m)) & (np.abs(n - m) < W // 2)].all()


def test_the_16_row_pass_settles_the_benchmark_pairs(nwh, asm, oracle):
    """C2-shaped pairs (100 bases, 10 edits, 96 % substitutions): at least 99 % are settled by the 16-row pass itself — a fast
    path that stopped accepting would otherwise still pass every comparison through the cascade."""
    rng = np.random.default_rng(2)
    hb = asm.HostBatch.from_strings(edited_pairs(rng, 3000, 100, 100, 10, 10, 0.96))
    h16 = half16(nwh, hb)
    told = check_halves(hb, h16, oracle.nw(hb))
    assert told.mean() >= 0.99, told.mean()


def test_the_generator_s_c2_pairs(nwh, asm, oracle):
    """The same on the product generator's own C2 stream (what bench.py times)."""
    cfg, _, _ = asm.workload("C2")
    hb = asm.generate_pairs(cfg, 0, 4000)
    h16 = half16(nwh, hb)
    told = check_halves(hb, h16, oracle.nw(hb))
    assert told.mean() >= 0.99, told.mean()
