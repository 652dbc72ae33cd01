"""Host logic of what the general-penalty kernels share (csrc/asm_affine.h), compiled for the CPU (host/affine_host_check.cpp)
and diffed against the oracle: gotoh_sweep with the empty sink (nw_affine_kernel's thread) against `nw`, gotoh_sweep with the trace
sink and gotoh_traceback (nw_trace_affine_kernel's thread) against `nw_cigar`, CIGAR for CIGAR, and a single-thread LV loop made
of lv_affine_step, LvRingView and LvRings (the shape of leap_general_kernel) against `leap`.  Lengths on both sides of a plane
word (64) and of a column block of the sweep (32), and the empty and the one-base string; the pair kinds of
tests/structured_cases.py.  The same source built as a stand-alone program under ASan + UBSan runs the same batches with the same
penalties, and must print what the library gave.  No GPU needed; the kernels around these functions are in test_gpu_structured.py and
test_gpu_parity.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import structured_cases as sc
from tests.oracle_binding import CIGAR_STRIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
SO = os.path.join(PKG, "libaffine_hostcheck.so")
_vp, _i = ctypes.c_void_p, ctypes.c_int

LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128)
PENALTIES = [(2, 3, 1), (4, 6, 2), (3, 1, 1)]  # the triples of the GPU tests; the last has x > o


@pytest.fixture(scope="module")
def affh():
    subprocess.check_call(["make", "-s", "-C", PKG, "affinecheck"])
    lib = ctypes.CDLL(SO)
    lib.affine_host_nw.argtypes = [ctypes.c_long, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]
    lib.affine_host_nw_cigar.argtypes = [ctypes.c_long, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i]
    lib.affine_host_leap.argtypes = [ctypes.c_long, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]
    return lib


def san_flags():
    """SAN_FLAGS of oracle/Makefile"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        for line in fh:
            if line.startswith("SAN_FLAGS :="):
                return line.split(":=", 1)[1].split()
    raise AssertionError("oracle/Makefile has no SAN_FLAGS")


@pytest.fixture(scope="module")
def affine_check_asan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("affine_check") / "affine_host_check_asan")
    src = os.path.join(PKG, "host", "affine_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-DAFFINE_HOST_CHECK_MAIN"] + san_flags() + ["-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _args(hb):
    keep = tuple(np.ascontiguousarray(a, t) for a, t in ((hb.reads, np.uint8), (hb.read_off, np.uint32), (hb.refs, np.uint8),
                                                         (hb.ref_off, np.uint32)))
    return keep, [hb.n] + [a.ctypes.data for a in keep]


def edge_pairs(seed):
    """Every (m, n) of LENGTHS with identical content, with 10 % substitutions, and with unrelated content."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for m in LENGTHS:
        for n in LENGTHS:
            code = rng.integers(0, 4, 128)
            text = bytes(acgt[code]).decode()
            hit = rng.random(128) < 0.10
            pairs.append((text[:m], text[:n]))
            pairs.append((text[:m], bytes(acgt[np.where(hit, (code + 1 + rng.integers(0, 3, 128)) % 4, code)]).decode()[:n]))
            pairs.append((text[:m], bytes(acgt[rng.integers(0, 4, 128)]).decode()[:n]))
    return pairs


@pytest.fixture(scope="module")
def corpus(asm):
    """name -> (batch, batch as packed): the length grid, and every structured kind with its longer string at each length from 31 up
    (32 pairs per length: four of each kind), 556 pairs in all."""
    grid = asm.HostBatch.from_strings(edge_pairs(5))
    out = {"grid": (grid, grid)}
    for L in LENGTHS[2:]:
        hb = sc.all_kinds_batch(asm, L, L, 3, n=32, seed=L)
        out[f"kinds at {L}"] = (hb, sc.as_packed(asm, hb))
    return out


def _first_bad(hb, got, want):
    bad = [i for i in range(hb.n) if got[i] != want[i]]
    return (len(bad), bad[0], hb.pair(bad[0]), got[bad[0]], want[bad[0]]) if bad else None


@pytest.mark.parametrize("pen", PENALTIES)
def test_gotoh_sweep_and_traceback(affh, oracle, corpus, pen):
    x, o, e = pen
    pairs = 0
    for name, (hb, seen) in corpus.items():
        want, want_cig = oracle.nw_cigar(seen, x, o, e)
        assert np.array_equal(want, oracle.nw(seen, x, o, e))
        keep, args = _args(hb)
        score, traced = np.zeros(hb.n, np.int32), np.zeros(hb.n, np.int32)
        cig = np.zeros(hb.n * CIGAR_STRIDE + 1, np.uint8)
        assert affh.affine_host_nw(*args, x, o, e, score.ctypes.data) == 0
        assert affh.affine_host_nw_cigar(*args, x, o, e, traced.ctypes.data, cig.ctypes.data, CIGAR_STRIDE) == 0
        raw = cig.tobytes()
        got_cig = [raw[i * CIGAR_STRIDE:(i + 1) * CIGAR_STRIDE].split(b"\0", 1)[0].decode() for i in range(hb.n)]
        assert _first_bad(hb, score, want) is None, (name, pen, "empty sink", _first_bad(hb, score, want))
        assert _first_bad(hb, traced, want) is None, (name, pen, "trace sink", _first_bad(hb, traced, want))
        assert _first_bad(hb, got_cig, want_cig) is None, (name, pen, "traceback", _first_bad(hb, got_cig, want_cig))
        pairs += hb.n
    assert pairs >= 500


@pytest.mark.parametrize("k", [3, 10])
@pytest.mark.parametrize("pen", PENALTIES)
def test_lv_lane_step_rings_and_geometry(affh, oracle, corpus, pen, k):
    x, o, e = pen
    aligned = 0
    for name, (hb, seen) in corpus.items():
        want = oracle.leap(seen, k, x, o, e)
        keep, args = _args(hb)
        got = np.zeros(hb.n, np.int32)
        assert affh.affine_host_leap(*args, k, x, o, e, got.ctypes.data) == 0
        assert _first_bad(hb, got, want) is None, (name, pen, k, _first_bad(hb, got, want))
        aligned += int((want > 0).sum())
    assert aligned > 100  # generations beyond the first ran


@pytest.mark.parametrize("pen", PENALTIES)
def test_the_same_batches_under_sanitizers(affh, affine_check_asan, oracle, corpus, pen, tmp_path):
    """The stand-alone program reads each batch into arrays of exactly its size and prints sweep score, traced score, LEAP (k = 3)
    and CIGAR per pair: the oracle's, with no sanitizer report."""
    x, o, e = pen
    for name, (hb, seen) in corpus.items():
        keep, _ = _args(hb)
        path = tmp_path / "batch.bin"
        path.write_bytes(np.int32(hb.n).tobytes() + keep[1].tobytes() + keep[3].tobytes() + keep[0].tobytes() + keep[2].tobytes())
        r = subprocess.run([affine_check_asan, str(path), "3", str(x), str(o), str(e)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, pen, r.returncode, r.stderr[-3000:])  # a report ends the run with another status
        rows = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
        want, want_cig = oracle.nw_cigar(seen, x, o, e)
        leap = oracle.leap(seen, 3, x, o, e)
        assert len(rows) == hb.n
        got = [(int(a), int(b), int(c), d) for a, b, c, d in rows]
        assert got == [(int(want[i]), int(want[i]), int(leap[i]), want_cig[i]) for i in range(hb.n)], (name, pen)
