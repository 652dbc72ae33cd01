"""Host logic of the unit-penalty LEAP core (csrc/asm_leapunit.h): what a thread of leap_unit_kernel / leap_unit_hint_kernel
runs for its pair, compiled for the CPU (host/leap_host_check.cpp) and diffed against the oracle's LEAP.  Three forms per
pair: leap_unit_generic (every width's code before the one-granule form), leap_unit_core (what the kernels call) and the
one-granule form with its clamp check switched on, which evaluates the clamped lane step beside the unclamped one and counts
where they part.  What is checked: all three give the oracle's result, and no lane step differs.  No GPU needed; the kernels
around it are in test_gpu_leap_unit.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
SO = os.path.join(PKG, "libleap_hostcheck.so")
_vp = ctypes.c_void_p

EDGE_LENGTHS = (1, 2, 3, 4, 62, 63, 64, 65, 66, 99, 100, 101, 126, 127, 128)
GENERIC, CORE, CHECKED = 0, 1, 2


@pytest.fixture(scope="module")
def leaph():
    subprocess.check_call(["make", "-s", "-C", PKG, "leapcheck"])
    lib = ctypes.CDLL(SO)
    lib.leap_host_unit.argtypes = [ctypes.c_long, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]
    return lib


def run(leaph, hb, k, form, w64=2):
    """(results, lane steps in which clamped and unclamped differ) of one form over the batch."""
    keep = tuple(np.ascontiguousarray(a, t) for a, t in ((hb.reads, np.uint8), (hb.read_off, np.uint32), (hb.refs, np.uint8),
                                                         (hb.ref_off, np.uint32)))
    out = np.zeros(hb.n, np.int32)
    differ = ctypes.c_int64(-1)
    rc = leaph.leap_host_unit(hb.n, *[a.ctypes.data for a in keep], k, w64, form, out.ctypes.data, ctypes.addressof(differ))
    assert rc == 0, rc
    return out, differ.value


def edge_pairs(seed):
    """Every (m, n) of EDGE_LENGTHS, |n-m| > k included, each with identical content, all-different content, and 10 % and 30 %
    substitutions (seeded) on a common random text."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for m in EDGE_LENGTHS:
        for n in EDGE_LENGTHS:
            code = rng.integers(0, 4, 128)
            text = bytes(acgt[code]).decode()
            pairs.append((text[:m], text[:n]))
            pairs.append((text[:m], bytes(acgt[(code + 1 + rng.integers(0, 3, 128)) % 4]).decode()[:n]))
            for rate in (0.10, 0.30):
                hit = rng.random(128) < rate
                other = np.where(hit, (code + 1 + rng.integers(0, 3, 128)) % 4, code)
                pairs.append((text[:m], bytes(acgt[other]).decode()[:n]))
    return pairs


def indel_pairs(seed, count):
    """Reads of every length 1..128 against themselves after 0-12 random edits, a third of them insertions and deletions."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for i in range(count):
        a = list(acgt[rng.integers(0, 4, 1 + i % 128)])
        b = list(a)
        for _ in range(int(rng.integers(0, 13))):
            u = rng.random()
            if u < 2 / 3 or (len(b) <= 1 and u < 5 / 6):
                b[int(rng.integers(0, len(b)))] = acgt[rng.integers(0, 4)]
            elif u < 5 / 6 or len(b) >= 128:
                del b[int(rng.integers(0, len(b)))]
            else:
                b.insert(int(rng.integers(0, len(b) + 1)), acgt[rng.integers(0, 4)])
        pairs.append((bytes(bytearray(int(c) for c in a)).decode(), bytes(bytearray(int(c) for c in b)).decode()))
    return pairs


def check_all_forms(leaph, oracle, hb, k, seen_as=None):
    want = oracle.leap(hb if seen_as is None else seen_as, k=k)
    generic, _ = run(leaph, hb, k, GENERIC)
    core, _ = run(leaph, hb, k, CORE)
    checked, differ = run(leaph, hb, k, CHECKED)
    m, n = hb.lengths()
    for name, got in (("generic", generic), ("core", core), ("checked", checked)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, k, bad.size, hb.pair(int(bad[0])), int(got[bad[0]]), int(want[bad[0]]), int(m[bad[0]]), int(n[bad[0]]))
    # the two clamp statements, on every lane step of every pair: a scan from `from` <= len returns at most len, and the scan
    # from st gives the end that the scan from min(st, len), capped at len, gives
    assert differ == 0, (k, differ)
    return want


@pytest.mark.parametrize("k", [1, 2, 3])
def test_word_edge_lengths(leaph, asm, oracle, k):
    hb = asm.HostBatch.from_strings(edge_pairs(100 + k))
    want = check_all_forms(leaph, oracle, hb, k)
    m, n = hb.lengths()
    assert (np.abs(n - m) > k).sum() > 100 and (want >= 0).sum() > 50  # pairs outside the band, and pairs that align


@pytest.mark.parametrize("k", [1, 2, 3])
def test_every_length_with_indels(leaph, asm, oracle, k):
    hb = asm.HostBatch.from_strings(indel_pairs(200 + k, 2560))
    want = check_all_forms(leaph, oracle, hb, k)
    assert (want > k).sum() > 100  # generations beyond the first K run as well


@pytest.mark.parametrize("k", [1, 2, 3])
def test_c2_shaped_sample(leaph, asm, oracle, k):
    """The product generator's own C2 stream (what bench.py times): 100 bp, 10 edits."""
    cfg, _, _ = asm.workload("C2")
    hb = asm.generate_pairs(cfg, 7, 4000)
    check_all_forms(leaph, oracle, hb, k)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_non_acgt_bytes(leaph, asm, oracle, k):
    """Anything but C, G, T is code 00, the same as A (bit_convert.cpp:340-355): the planes of such a pair are the planes of
    the pair with every other byte written as A, and that is the pair the oracle, which compares characters, is given."""
    rng = np.random.default_rng(300 + k)
    alphabet = np.frombuffer(b"ACGTNacgtnRY-*x", np.uint8)
    pairs = []
    for i in range(600):
        a = alphabet[rng.integers(0, len(alphabet), int(rng.choice(EDGE_LENGTHS)))]
        b = a.copy()
        hit = rng.random(len(b)) < 0.08
        b[hit] = alphabet[rng.integers(0, len(alphabet), int(hit.sum()))]
        cut = int(rng.integers(0, min(k + 1, len(b))))
        b = b[cut:] if i % 3 == 0 and len(b) > cut else b
        pairs.append((bytes(a).decode(), bytes(b).decode()))
    pairs += [("N" * 100, "A" * 100), ("N" * 128, "n" * 128), ("ACGTN" * 20, "ACGTA" * 20), ("N", "C")]
    hb = asm.HostBatch.from_strings(pairs)
    as_a = np.full(256, ord("A"), np.uint8)
    as_a[[ord("C"), ord("G"), ord("T")]] = [ord("C"), ord("G"), ord("T")]
    seen = asm.HostBatch(as_a[hb.reads], hb.read_off, as_a[hb.refs], hb.ref_off)
    assert (seen.reads != hb.reads).mean() > 0.3
    check_all_forms(leaph, oracle, hb, k, seen_as=seen)


def test_three_word_width_is_the_generic_form(leaph, asm, oracle):
    """129-192 bases: leap_unit_core<K, 3> is leap_unit_generic<K, 3>, and both are the oracle's."""
    rng = np.random.default_rng(9)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for i in range(400):
        a = acgt[rng.integers(0, 4, int(rng.integers(129, 193)))]
        b = a.copy()
        hit = rng.random(len(b)) < 0.05
        b[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        b = b[:len(b) - int(rng.integers(0, 3))]
        pairs.append((bytes(a).decode(), bytes(b).decode()))
    hb = asm.HostBatch.from_strings(pairs)
    want = oracle.leap(hb, k=3)
    assert np.array_equal(run(leaph, hb, 3, GENERIC, w64=3)[0], want)
    assert np.array_equal(run(leaph, hb, 3, CORE, w64=3)[0], want)
