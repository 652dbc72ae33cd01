"""Host logic of the filters (csrc/asm_simd_ed.h: what a thread of the kernels of csrc/asm_filter.h decides for its pair), compiled
for the CPU (host/filter_host_check.cpp) and driven serially in the kernels' shapes: SIMD_ED's Levenshtein events with the register
column and with the column in memory, the clean, final and sequential verdicts, the affine mode thread per pair and as a mirror of
the four-threads-per-pair kernel, with and without its SHD, and the stand-alone SHD — against the reference's recorded results
(tests/golden/filter_*.npz) and against the oracle on ragged, dirty and word-edge input.  The same source built as a stand-alone
program under ASan + UBSan runs the whole core on reduced batches and must give the library's digest.  No GPU needed; the kernels
around these functions are in test_gpu_parity.py and test_gpu_filter_edges.py."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests.test_affine_host import san_flags
from tests.test_oracle_golden import GOLD, _inputs_sha
from tests.oracle_binding import SIMD_WARM_STATE
from tests.util import check, random_ragged_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
SO = os.path.join(PKG, "libfilter_hostcheck.so")
_vp, _i = ctypes.c_void_p, ctypes.c_int
SEQUENTIAL, CLEAN = 0, 1  # asm.FILTER_*
REG_MAX_T = 8

with open(os.path.join(GOLD, "filter_index.json")) as fh:
    FILTER_INDEX = json.load(fh)

EDGE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)


def _args(hb):
    keep = tuple(np.ascontiguousarray(a, t) for a, t in ((hb.reads, np.uint8), (hb.read_off, np.uint32), (hb.refs, np.uint8),
                                                         (hb.ref_off, np.uint32)))
    return keep, [hb.n] + [a.ctypes.data for a in keep]


class Core:
    def __init__(self, lib):
        b5 = [ctypes.c_long, _vp, _vp, _vp, _vp]
        lib.filter_host_events.argtypes = b5 + [_i, _i, _i, _i, _vp]
        lib.filter_host_verdicts.argtypes = [ctypes.c_long, _vp, _i, _i, _vp]
        lib.filter_host_affine.argtypes = b5 + [_i] * 8 + [_vp]
        lib.filter_host_shd.argtypes = b5 + [_i, _vp]
        lib.filter_host_quad_extend.argtypes = b5 + [_vp]
        lib.filter_host_selfcheck.argtypes = b5 + [_vp]
        lib.filter_host_selfcheck.restype = ctypes.c_long
        self.lib = lib

    def events(self, hb, t, shd, ed_mode=0, form=1):
        keep, args = _args(hb)
        ev = np.zeros(hb.n, np.int32)
        assert self.lib.filter_host_events(*args, t, 1 if shd else 0, ed_mode, form, ev.ctypes.data) == 0
        return ev

    def simd_ed(self, hb, t, shd, mode, state, ed_mode=0, form=1):
        """asm_simd_ed_mode_batch_async: events, then one of final / clean / sequential -> (ed, state after)"""
        ed = self.events(hb, t, shd, ed_mode, form)
        st = np.array(state, np.int32)
        how = 1 if ed_mode in (1, 3) else 0 if mode == CLEAN else 2
        assert self.lib.filter_host_verdicts(hb.n, ed.ctypes.data, t, how, st.ctypes.data) == 0
        return ed, tuple(int(v) for v in st)

    def simd_ed_affine(self, hb, g, af, x, o, e, shd_t=None, mode=0, form=0):
        keep, args = _args(hb)
        out = np.zeros(hb.n, np.int32)
        assert self.lib.filter_host_affine(*args, g, af, x, o, e, mode, -1 if shd_t is None else shd_t, form, out.ctypes.data) == 0
        return out

    def shd(self, hb, max_error):
        keep, args = _args(hb)
        out = np.zeros(hb.n, np.int32)
        assert self.lib.filter_host_shd(*args, max_error, out.ctypes.data) == 0
        return out

    def quad_extend_differ(self, hb):
        keep, args = _args(hb)
        bad = np.zeros(1, np.int64)
        assert self.lib.filter_host_quad_extend(*args, bad.ctypes.data) == 0
        return int(bad[0])

    def selfcheck(self, hb):
        keep, args = _args(hb)
        digest = np.zeros(1, np.uint64)
        return int(self.lib.filter_host_selfcheck(*args, digest.ctypes.data)), int(digest[0])


@pytest.fixture(scope="module")
def core():
    subprocess.check_call(["make", "-s", "-C", PKG, "filtercheck"])
    return Core(ctypes.CDLL(SO))


@pytest.fixture(scope="module")
def filter_check_asan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_check") / "filter_host_check_asan")
    src = os.path.join(PKG, "host", "filter_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-DFILTER_HOST_CHECK_MAIN"] + san_flags() + ["-o", exe, src],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def short_pairs(asm, hb):
    """the pairs whose strings both fit one granule: a batch the four-threads-per-pair kernel takes"""
    m, n = hb.lengths()
    return asm.HostBatch.from_strings([hb.pair(int(i)) for i in np.nonzero(np.maximum(m, n) <= 128)[0]])


def edge_batch(asm, seed=11):
    """Every (read, reference) length of EDGE_LENGTHS: identical up to the shorter one, with 10 % substitutions, and unrelated."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for m in EDGE_LENGTHS:
        for n in EDGE_LENGTHS:
            code = rng.integers(0, 4, 300)
            text = bytes(acgt[code]).decode()
            hit = rng.random(300) < 0.10
            pairs.append((text[:m], text[:n]))
            pairs.append((text[:m], bytes(acgt[np.where(hit, (code + 1 + rng.integers(0, 3, 300)) % 4, code)]).decode()[:n]))
            pairs.append((text[:m], bytes(acgt[rng.integers(0, 4, 300)]).decode()[:n]))
    return asm.HostBatch.from_strings(pairs)


def dirty_ragged_batch(asm):
    """the input of test_gpu_parity.test_filters_on_ragged_and_dirty_input"""
    hb = random_ragged_batch(asm, 47, 4000, 0, 300)
    rng = np.random.default_rng(5)
    reads = hb.reads.copy()
    hits = rng.random(reads.size) < 0.01
    reads[hits] = rng.choice(np.frombuffer(b"NnacgtRY-*", np.uint8), int(hits.sum()))
    return asm.HostBatch(reads, hb.read_off, hb.refs, hb.ref_off)


@pytest.fixture(scope="module")
def corpus(asm):
    """name -> batch: ragged and dirty, the length grid, and of each the pairs of at most 128 characters (the quad kernel's batches)"""
    out = {"ragged": dirty_ragged_batch(asm), "edges": edge_batch(asm)}
    for name in ("ragged", "edges"):
        out[name + " <= 128"] = short_pairs(asm, out[name])
    return out


@pytest.mark.parametrize("name", sorted(FILTER_INDEX["cases"]))
def test_core_matches_reference_goldens(asm, core, name):
    """The arrays and the rules of test_oracle_golden.test_filter_oracle_matches_reference_goldens, the core in the oracle's place."""
    meta = FILTER_INDEX["cases"][name]
    cfg, _, _ = asm.workload(meta["workload"])
    hb = asm.generate_pairs(cfg, meta["first"], meta["n"])
    assert _inputs_sha(hb) == meta["inputs_sha256"], "generator output changed: regenerate the goldens deliberately"
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    state = tuple(FILTER_INDEX["warm_state"])
    for t, shd in FILTER_INDEX["simd_settings"]:
        forms = (0, 1) if t <= REG_MAX_T else (1,)
        for form in forms:
            ed, _ = core.simd_ed(hb, t, bool(shd), SEQUENTIAL, state, form=form)
            ps = gold[f"pass_t{t}_shd{shd}"]
            assert np.array_equal((ed >= 0).astype(np.uint8), ps), (name, t, shd, form, "check_pass")
            assert np.array_equal(ed, np.where(ps == 1, gold[f"ed_t{t}_shd{shd}"], -1)), (name, t, shd, form, "get_ED")
    for me in FILTER_INDEX["shd_errors"]:
        assert np.array_equal(core.shd(hb, me), gold[f"shd_e{me}"]), (name, me)
    quad = int(np.maximum(*hb.lengths()).max()) <= 128
    for form in (0, 1) if quad else (0,):
        for g, af, x, o, e in FILTER_INDEX["affine_settings"]:
            ed = core.simd_ed_affine(hb, g, af, x, o, e, form=form)
            key = f"g{g}_a{af}_x{x}o{o}e{e}"
            ps = gold["af_pass_" + key]
            assert np.array_equal((ed >= 0).astype(np.uint8), ps), (name, key, form, "check_pass")
            assert np.array_equal(ed, np.where(ps == 1, gold["af_ed_" + key], -1)), (name, key, form, "get_ED")
        for g, af, x, o, e, st in FILTER_INDEX["affine_shd_settings"]:
            ed = core.simd_ed_affine(hb, g, af, x, o, e, shd_t=st, form=form)
            key = f"g{g}_a{af}_x{x}o{o}e{e}_s{st}"
            ps = gold["afs_pass_" + key]
            assert np.array_equal((ed >= 0).astype(np.uint8), ps), (name, key, form, "check_pass")
            assert np.array_equal(ed, np.where(ps == 1, gold["afs_ed_" + key], -1)), (name, key, form, "get_ED")


@pytest.mark.parametrize("ed_mode", [0, 1, 2, 3])
def test_levenshtein_matches_oracle(core, oracle, corpus, ed_mode):
    """Every ED_mode, sequential from the warm state (with the state that comes back chained into a second half) and clean,
    thresholds on both sides of the register forms' limit and of SHD's, both column forms where both exist."""
    for name, hb in corpus.items():
        for t, shd in ((1, True), (3, True), (7, False), (8, True), (9, False), (12, True), (16, True), (32, False)):
            forms = (0, 1) if t <= REG_MAX_T and ed_mode in (0, 3) else (1,)
            for mode in (SEQUENTIAL, CLEAN):
                want, _, _ = oracle.simd_ed(hb, t, shd, mode, SIMD_WARM_STATE, ed_mode=ed_mode)
                for form in forms:
                    got, _ = core.simd_ed(hb, t, shd, mode, SIMD_WARM_STATE, ed_mode, form)
                    check(f"{name} T={t} shd={shd} mode={mode} ed_mode={ed_mode} form={form}", got, want, hb)
            half = hb.n // 2
            first, state = core.simd_ed(hb.slice(0, half), t, shd, SEQUENTIAL, SIMD_WARM_STATE, ed_mode)
            second, _ = core.simd_ed(hb.slice(half, hb.n), t, shd, SEQUENTIAL, state, ed_mode)
            want, _, _ = oracle.simd_ed(hb, t, shd, SEQUENTIAL, SIMD_WARM_STATE, ed_mode=ed_mode)
            check(f"{name} T={t} in two chunks", np.concatenate([first, second]), want, hb)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_affine_matches_oracle(core, oracle, corpus, mode):
    """Every ED_mode, narrow and wide bands, deep rings, with and without the SHD in front; thread per pair on every batch, the mirror
    of the four-threads-per-pair kernel on the batches it takes."""
    for name, hb in corpus.items():
        for g, af, x, o, e in ((3, 60, 2, 3, 1), (8, 100, 4, 6, 2), (32, 200, 15, 15, 15), (6, 30, 1, 1, 1)):
            for st in (None, 0, min(g, 16)):
                want, _ = oracle.simd_ed_affine(hb, g, af, x, o, e, shd_t=st, mode=mode)
                for form in (0, 1) if name.endswith("<= 128") else (0,):
                    got = core.simd_ed_affine(hb, g, af, x, o, e, st, mode, form)
                    check(f"{name} {(g, af, x, o, e)} shd={st} mode={mode} form={form}", got, want, hb)


@pytest.mark.parametrize("max_error", [0, 1, 2, 6, 16])
def test_shd_matches_oracle(core, oracle, corpus, max_error):
    for name, hb in corpus.items():
        check(f"{name} e={max_error}", core.shd(hb, max_error), oracle.shd(hb, max_error), hb)


@pytest.mark.parametrize("t", range(1, REG_MAX_T + 1))
def test_register_and_memory_columns_give_the_same_events(core, corpus, t):
    reached = 0
    for name, hb in corpus.items():
        for shd in (True, False):
            for ed_mode in (0, 3):
                reg, col = core.events(hb, t, shd, ed_mode, 0), core.events(hb, t, shd, ed_mode, 1)
                check(f"{name} T={t} shd={shd} ed_mode={ed_mode}", reg, col, hb)
                reached += int((col >= 0).sum())
    assert reached > 100  # generations beyond the first ran


QUAD_LENGTHS = (0, 1, 31, 32, 33, 64, 96, 127, 128)


def quad_batch(asm, seed=23, per_length=40):
    """Reads of every length of QUAD_LENGTHS; references a near copy, a shifted copy or unrelated text, shorter, equal and longer."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for m in QUAD_LENGTHS:
        for k in range(per_length):
            code = rng.integers(0, 4, 128)
            n = int((m, 128, rng.integers(0, 129), max(m - int(rng.integers(0, 9)), 0))[k % 4])
            kind = k % 3
            other = np.where(rng.random(128) < 0.05, rng.integers(0, 4, 128), code) if kind == 0 else \
                np.roll(code, int(rng.integers(-8, 9))) if kind == 1 else rng.integers(0, 4, 128)
            pairs.append((bytes(acgt[code[:m]]).decode(), bytes(acgt[other[:n]]).decode()))
    return asm.HostBatch.from_strings(pairs)


def test_quad_extension_equals_the_vector_extension(asm, core):
    """simd_quad_extend on the staged dword planes against simd_extend(simd_lane_mask(d), st, len) on VW<2>: every d in [-32, 32] and
    every st in [0, len] of 360 seeded pairs, len over QUAD_LENGTHS."""
    hb = quad_batch(asm)
    assert hb.n >= 300 and set(int(v) for v in hb.lengths()[0]) == set(QUAD_LENGTHS)
    assert core.quad_extend_differ(hb) == 0


def test_the_core_under_sanitizers(asm, core, filter_check_asan, corpus, tmp_path):
    """The stand-alone program reads a batch into arrays of exactly its size and runs the whole core on it — both columns, the three
    resolvers, both affine forms with and without SHD in every ED_mode, SHD, the quad extension: no form parts from its twin, no
    sanitizer report, and the digest of every result is the library's."""
    batches = {"edges": corpus["edges"], "edges <= 128": corpus["edges <= 128"], "ragged": corpus["ragged"].slice(0, 120),
               "ragged <= 128": corpus["ragged <= 128"].slice(0, 120), "quad": quad_batch(asm, per_length=4)}
    for name, hb in batches.items():
        keep, _ = _args(hb)
        path = tmp_path / "batch.bin"
        path.write_bytes(np.int32(hb.n).tobytes() + keep[1].tobytes() + keep[3].tobytes() + keep[0].tobytes() + keep[2].tobytes())
        r = subprocess.run([filter_check_asan, str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-3000:])  # a report ends the run with another status
        bad, digest = core.selfcheck(hb)
        assert bad == 0 and r.stdout.split() == ["%016x" % digest, "0"], (name, bad, r.stdout)
