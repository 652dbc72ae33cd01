"""MI355X-native batched pair aligner — Python host side over the C ABI (include/asm_mi355x.h).

This package is plumbing: it binds libasm_mi355x.so (HIP kernels + C ABI, built in-tree by
`make -C approximate-string-matching_amd lib`) with ctypes and mirrors the reference's per-pair interface
for the ONE path this repo accelerates — `benchmark::_run_benchmark`
(/root/reference/GASMA/benchmark/benchmark_utils.h:231-259: NW, LEAP, Greedy per read pair) — as whole-batch
calls.  There is no CPU fallback: every compute call needs the library and a HIP device and raises otherwise.

Import name: the directory is `approximate-string-matching_amd`; `import approximate_string_matching_amd`
works through the loader module of that name at the repo root.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ASM_MI355X_LIB") or os.path.join(_HERE, "libasm_mi355x.so")  # override: A/B builds of the same ABI
HEADER_PATH = os.path.join(_HERE, "..", "include", "asm_mi355x.h")

NW, LEAP, GREEDY = 0, 1, 2
ALIGNER_NAMES = {NW: "nw", LEAP: "leap", GREEDY: "greedy"}
GREEDY_SEQUENTIAL, GREEDY_CLEAN = 0, 1
FILTER_SEQUENTIAL, FILTER_CLEAN = 0, 1
ALIGN_GLOBAL, ALIGN_SEMI_GLOBAL = 0, 1
LEAP_GLOBAL, LEAP_LOCAL, LEAP_SEMI_FREE_BEGIN, LEAP_SEMI_FREE_END = 0, 1, 2, 3  # asm_params.leap_mode: LV::init's ED_modes
GEN_EXACT_ERRORS, GEN_PER_BASE, GEN_UP_TO_ERRORS = 0, 1, 2
GREEDY_MAX_LENGTH = 128
LEAP_MAX_LENGTH = 256
MAX_LENGTH = 512


class AsmError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"asm_mi355x error {code}: {message}")
        self.code = code


class Params(ctypes.Structure):
    """asm_params: constructor arguments of `benchmark` (benchmark_utils.h:263-289) and of hurdle_matrix
    (hurdle_matrix.h:552-559)."""

    _fields_ = [("k", ctypes.c_int32), ("x", ctypes.c_int32), ("o", ctypes.c_int32), ("e", ctypes.c_int32),
                ("p_match", ctypes.c_double), ("p_mismatch", ctypes.c_double), ("p_indel", ctypes.c_double),
                ("alignment_type", ctypes.c_int32), ("leap_mode", ctypes.c_int32)]

    @classmethod
    def default(cls, k: int = 3, x: int = 1, o: int = 1, e: int = 1, p_match: float = 0.80,
                p_mismatch: float = 0.20 / 3, p_indel: float = 0.40 / 3, alignment_type: int = 0, leap_mode: int = 0) -> "Params":
        """alignment_type: ALIGN_GLOBAL (0) or ALIGN_SEMI_GLOBAL (1) — hurdle_matrix's alignment_type_t; Greedy only.
        leap_mode: LEAP_GLOBAL (0, the harness) / LEAP_LOCAL / LEAP_SEMI_FREE_BEGIN / LEAP_SEMI_FREE_END — LV::init's ED_modes."""
        return cls(k, x, o, e, p_match, p_mismatch, p_indel, alignment_type, leap_mode)


class StreamStats(ctypes.Structure):
    """asm_stream_stats: what asm_stream_seq_file did."""

    _fields_ = [("pairs", ctypes.c_int64), ("chunks", ctypes.c_int64), ("bytes", ctypes.c_int64),
                ("counters", ctypes.c_ulonglong * 4), ("seconds", ctypes.c_double), ("seconds_read", ctypes.c_double),
                ("max_length", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class GenConfig(ctypes.Structure):
    """asm_gen_config: seeded restatement of `Dataset` (benchmark_dataset.h:61-253)."""

    _fields_ = [("seed", ctypes.c_uint64), ("kind", ctypes.c_int32), ("len_lo", ctypes.c_int32),
                ("len_hi", ctypes.c_int32), ("err", ctypes.c_float), ("mismatch_rate", ctypes.c_float),
                ("p_sub", ctypes.c_float), ("p_ins", ctypes.c_float), ("p_del", ctypes.c_float)]

    @classmethod
    def exact(cls, seed: int, length: int, err: float, mismatch_rate: float = 0.96, length_hi: Optional[int] = None):
        """Dataset(num_reads, length, err, 0.96, exact=true) — benchmark.cpp:19."""
        return cls(seed, GEN_EXACT_ERRORS, length, length_hi if length_hi is not None else length, err,
                   mismatch_rate, 0.0, 0.0, 0.0)

    @classmethod
    def up_to(cls, seed: int, length: int, err: float, mismatch_rate: float = 0.96, length_hi: Optional[int] = None):
        """Dataset(..., exact=false), the "lt_eq" files of GASMA/benchmark/README.md: 0 .. ceil(L*err) - 1 edit operations,
        uniformly (benchmark_dataset.h:153-156)."""
        return cls(seed, GEN_UP_TO_ERRORS, length, length_hi if length_hi is not None else length, err,
                   mismatch_rate, 0.0, 0.0, 0.0)

    @classmethod
    def per_base(cls, seed: int, length: int, p_sub: float, p_ins: float, p_del: float,
                 length_hi: Optional[int] = None):
        """Independent per-base events; SRR611076-shaped rates are README.md:73-76 of the reference."""
        return cls(seed, GEN_PER_BASE, length, length_hi if length_hi is not None else length, 0.0, 0.0, p_sub,
                   p_ins, p_del)


class MapParams(ctypes.Structure):
    """asm_map_params: max errors e (0..15), both strands, k-mer bucket cap (0 = none), Greedy's k."""

    _fields_ = [("max_errors", ctypes.c_int32), ("both_strands", ctypes.c_int32), ("max_occ", ctypes.c_int32),
                ("greedy_k", ctypes.c_int32)]


class MapFileStats(ctypes.Structure):
    """asm_map_file_stats"""
    _fields_ = [("reads", ctypes.c_int64), ("mapped", ctypes.c_int64), ("too_long", ctypes.c_int64), ("records", ctypes.c_int64),
                ("chunks", ctypes.c_int64), ("bytes_in", ctypes.c_int64), ("bytes_out", ctypes.c_int64),
                ("seconds", ctypes.c_double), ("seconds_read", ctypes.c_double), ("seconds_write", ctypes.c_double)]


class MapPairsFileStats(ctypes.Structure):
    """asm_map_pairs_file_stats"""
    _fields_ = [("pairs", ctypes.c_int64), ("proper", ctypes.c_int64), ("rescued", ctypes.c_int64), ("unsent", ctypes.c_int64),
                ("records", ctypes.c_int64), ("chunks", ctypes.c_int64), ("bytes_in", ctypes.c_int64), ("bytes_out", ctypes.c_int64),
                ("carry_peak", ctypes.c_int64), ("seconds", ctypes.c_double), ("seconds_read", ctypes.c_double),
                ("seconds_write", ctypes.c_double)]


class SamSortStats(ctypes.Structure):
    """asm_sam_sort_stats"""
    _fields_ = [("lines", ctypes.c_int64), ("bytes_held", ctypes.c_int64), ("slabs", ctypes.c_int64), ("seconds_sort", ctypes.c_double)]


class BamIndexStats(ctypes.Structure):
    """asm_bam_index_stats"""
    _fields_ = [("refs", ctypes.c_int64), ("bins", ctypes.c_int64), ("chunks", ctypes.c_int64), ("intervals", ctypes.c_int64),
                ("no_coor", ctypes.c_int64), ("bytes", ctypes.c_int64), ("seconds_index", ctypes.c_double)]


class IndexFileStats(ctypes.Structure):
    """asm_index_file_stats"""
    _fields_ = [("n_seqs", ctypes.c_int64), ("bases", ctypes.c_int64), ("bytes_in", ctypes.c_int64), ("chunks", ctypes.c_int64),
                ("seconds", ctypes.c_double), ("seconds_read", ctypes.c_double), ("seconds_index", ctypes.c_double)]


class PairParams(ctypes.Structure):
    """asm_pair_params: projected span in [min_insert, max_insert] (0 <= min <= max <= 8192), mate rescue's error bound (-1 = off)."""

    _fields_ = [("min_insert", ctypes.c_int32), ("max_insert", ctypes.c_int32), ("rescue_errors", ctypes.c_int32)]


# asm_map_hit, one per read
MAP_HIT_DTYPE = np.dtype([("seq_id", np.int32), ("pos", np.uint32), ("end", np.uint32), ("dist", np.int16), ("strand", np.uint8),
                          ("flags", np.uint8), ("greedy_cost", np.int32)])
MAP_MAPPED, MAP_TOO_SHORT, MAP_SEED_CAPPED, MAP_CIGAR_TRUNCATED = 1, 2, 4, 8
MAPQ_REFERENCE, MAPQ_GAP = 0, 1  # asm_map_set_mapq_model
SAM_TAG_MD, MAP_MD_CAP = 1, 80  # asm_map_set_sam_tags; ASM_MAP_MD_CAP: an MD tag and its NUL always fit
OUT_SAM, OUT_BAM, BGZF_PAYLOAD = 0, 1, 65280  # asm_map_set_output_format; ASM_BGZF_PAYLOAD: uncompressed bytes per BGZF block
BGZF_STORED, BGZF_DEFLATE = 0, 1  # asm_map_set_bgzf_level: the BAM container's blocks
BAM_INDEX_NONE, BAM_INDEX_BAI = 0, 1  # asm_map_set_bam_index: what the sorted BAM calls write beside the file
MAP_SECONDARY, MAP_HITS_TRUNCATED, MAP_MAX_HITS = 16, 32, 256
MAP_PROPER_PAIR, MAP_RESCUED, MAP_MAX_INSERT = 64, 128, 8192
MAP_MIN_K, MAP_MAX_K, MAP_MAX_READ, MAP_MAX_ERRORS = 8, 14, 511, 15
FASTA_TILE = 4096  # ASM_FASTA_TILE: the bytes one workgroup of build_index_file's parser takes, 16 per thread


def _as_bytes(s) -> bytes:
    return s.encode("ascii") if isinstance(s, str) else bytes(s)


def pack_sequences(seqs) -> Tuple[np.ndarray, np.ndarray]:
    """Sequences (str / bytes) -> (concatenated uint8, n+1 uint64 offsets)."""
    parts = [_as_bytes(s) for s in seqs]
    off = np.zeros(len(parts) + 1, np.uint64)
    if parts:
        off[1:] = np.cumsum([len(b) for b in parts])
    return np.frombuffer(b"".join(parts), np.uint8).copy(), off


def read_fasta(path: str):
    """-> [(name, sequence)]; the name is the first word of the header."""
    out, name, chunks = [], None, []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(chunks)))
                name, chunks = (line[1:].split() or [""])[0], []
            elif name is not None:
                chunks.append(line.strip())
    if name is not None:
        out.append((name, "".join(chunks)))
    return out


def read_fastq(path: str):
    """-> [(name, sequence, quality)]; FASTA input gives quality '*'."""
    with open(path) as fh:
        first = fh.read(1)
    if first == ">":
        return [(n, s, "*") for n, s in read_fasta(path)]
    out = []
    with open(path) as fh:
        while True:
            h = fh.readline()
            if not h:
                break
            if not h.strip():
                continue
            seq = fh.readline().rstrip("\r\n")
            fh.readline()
            qual = fh.readline().rstrip("\r\n")
            out.append(((h[1:].split() or [""])[0], seq, qual))
    return out


# The named workloads of BASELINE.json `configs`.
def workload(name: str) -> Tuple[GenConfig, int, Params]:
    """-> (generator config, number of pairs, aligner params) for C1..C5."""
    if name == "C1":
        return GenConfig.exact(1, 100, 0.05), 10_000, Params.default(k=3)
    if name == "C2":
        return GenConfig.exact(2, 100, 0.10), 1_000_000, Params.default(k=3)
    if name == "C3":
        return GenConfig.exact(3, 150, 0.20), 10_000_000, Params.default(k=30)
    if name == "C4":
        return GenConfig.per_base(4, 100, 0.02452, 0.000468, 0.000553), 10_000_000, Params.default(k=3)
    if name == "C5":
        return GenConfig.exact(5, 64, 0.10, length_hi=300), 10_000_000, Params.default(k=3)
    raise KeyError(name)


_lib = None


def load_library() -> ctypes.CDLL:
    """Loads the in-tree C-ABI library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AsmError(-2, f"{LIB_PATH} is missing — build it with `make -C {_HERE} lib` "
                           "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    c = ctypes
    vp, i32, i64, u64p = c.c_void_p, c.c_int, c.c_int64, c.POINTER(c.c_ulonglong)
    sigs = {
        "asm_version": (c.c_char_p, []),
        "asm_default_params": (None, [c.POINTER(Params)]),
        "asm_device_count": (i32, []),
        "asm_create": (i32, [c.POINTER(vp), i32]),
        "asm_destroy": (i32, [vp]),
        "asm_last_error": (c.c_char_p, [vp]),
        "asm_set_stream": (i32, [vp, vp]),
        "asm_reset_stream": (i32, [vp]),
        "asm_synchronize": (i32, [vp]),
        "asm_generate_pairs": (i32, [c.POINTER(GenConfig), i64, i64, vp, vp, vp, c.c_size_t, vp, c.c_size_t]),
        "asm_batch_upload": (i32, [vp, i64, vp, vp, vp, vp, i32, c.POINTER(vp)]),
        "asm_batch_generate": (i32, [vp, c.POINTER(GenConfig), i64, i64, i32, c.POINTER(vp)]),
        "asm_reference_upload": (i32, [vp, vp, c.c_size_t, c.POINTER(vp)]),
        "asm_reference_free": (i32, [vp, vp]),
        "asm_batch_from_hits": (i32, [vp, vp, i64, vp, vp, vp, i32, c.POINTER(vp)]),
        "asm_batch_free": (i32, [vp, vp]),
        "asm_batch_from_text": (i32, [vp, vp, c.c_size_t, i32, c.POINTER(vp)]),
        "asm_stream_seq_file": (i32, [vp, c.c_char_p, c.POINTER(Params), i32, i32, i64, i64, vp, vp, vp, i64, vp, i64,
                                      c.POINTER(StreamStats)]),
        "asm_batch_tail_summary": (i32, [vp, vp, vp]),
        "asm_tail_state_advance": (i32, [vp, vp, i64]),
        "asm_batch_resolve_tails": (i32, [vp, vp, vp]),
        "asm_batch_size": (i64, [vp]),
        "asm_batch_max_length": (i32, [vp]),
        "asm_batch_text_bytes": (i64, [vp]),
        "asm_batch_download": (i32, [vp, vp, vp, vp, vp, c.c_size_t, vp, c.c_size_t]),
        "asm_batch_planes_size": (i64, [vp]),
        "asm_batch_download_planes": (i32, [vp, vp, vp, c.c_size_t, vp, vp]),
        "asm_batch_pack_async": (i32, [vp, vp]),
        "asm_align_batch_async": (i32, [vp, vp, i32, c.POINTER(Params), vp]),
        "asm_align_batch_hinted_async": (i32, [vp, vp, i32, c.POINTER(Params), vp, vp]),
        "asm_align_batch": (i32, [vp, i32, i64, vp, vp, vp, vp, c.POINTER(Params), i32, vp]),
        "asm_greedy_cigar_batch_async": (i32, [vp, vp, c.POINTER(Params), vp, vp, i32, vp]),
        "asm_cigar_format": (i32, [vp, i32, i32, vp, c.c_size_t]),
        "asm_coverage": (i32, [vp, vp, c.POINTER(Params), vp, i32, vp, i32, vp, vp, i32, vp, vp]),
        "asm_simd_ed_batch_async": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "asm_simd_ed_mode_batch_async": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
        "asm_simd_ed_affine_batch_async": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
        "asm_simd_ed_affine_shd_batch_async": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        "asm_simd_ed_affine_mode_batch_async": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "asm_shd_filter_batch_async": (i32, [vp, vp, i32, vp]),
        "asm_pipeline_join_async": (i32, [vp]),
        "asm_profile_enable": (i32, [vp, i32, c.c_uint32]),
        "asm_profile_read": (i32, [vp, vp, i32, vp]),
        "asm_count_equal_async": (i32, [vp, vp, vp, i64, vp]),
        "asm_accuracy_async": (i32, [vp, vp, vp, vp, vp, i64, vp]),
        "asm_run_benchmark_async": (i32, [vp, vp, c.POINTER(Params), i32, vp, vp, vp, vp, vp]),
        "asm_index_build": (i32, [vp, vp, vp, c.c_int32, i32, c.POINTER(vp)]),
        "asm_index_free": (i32, [vp, vp]),
        "asm_map_reads": (i32, [vp, vp, i64, vp, vp, c.POINTER(MapParams), vp, vp, i32, vp]),
        "asm_map_reads_all": (i32, [vp, vp, i64, vp, vp, c.POINTER(MapParams), i32, i32, vp, vp, vp, i32, vp]),
        "asm_map_pairs": (i32, [vp, vp, i64, vp, vp, vp, vp, c.POINTER(MapParams), c.POINTER(PairParams), vp, vp, vp, vp, i32, vp]),
        "asm_map_pairs_all": (i32, [vp, vp, i64, vp, vp, vp, vp, c.POINTER(MapParams), c.POINTER(PairParams), i32, i32, vp, vp, vp, vp,
                                    vp, i32, vp]),
        "asm_map_set_mapq_model": (i32, [vp, i32]),
        "asm_map_get_mapq_model": (i32, [vp]),
        "asm_map_last_mapq": (i32, [vp, vp, i64]),
        "asm_map_set_sam_tags": (i32, [vp, c.c_uint]),
        "asm_map_get_sam_tags": (c.c_uint, [vp]),
        "asm_map_set_output_format": (i32, [vp, i32]),
        "asm_map_get_output_format": (i32, [vp]),
        "asm_bgzf_bound": (c.c_size_t, [c.c_size_t, i32]),
        "asm_bgzf_frame": (i32, [vp, vp, c.c_size_t, i32, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "asm_map_set_bgzf_level": (i32, [vp, i32]),
        "asm_map_get_bgzf_level": (i32, [vp]),
        "asm_bgzf_compress": (i32, [vp, vp, c.c_size_t, i32, i32, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "asm_bgzf_compress_host": (i32, [vp, c.c_size_t, i32, i32, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "asm_map_set_bam_index": (i32, [vp, i32]),
        "asm_map_get_bam_index": (i32, [vp]),
        "asm_map_last_bam_index": (i32, [vp, c.POINTER(BamIndexStats)]),
        "asm_bam_index_host": (i32, [vp, c.c_size_t, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "asm_bgzf_decompressed_size": (i32, [vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "asm_bgzf_decompress": (i32, [vp, vp, c.c_size_t, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "asm_bgzf_decompress_host": (i32, [vp, c.c_size_t, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "asm_md_format": (i32, [vp, i32, c.c_char_p, i32, c.c_char_p, i32, vp, c.c_size_t]),
        "asm_map_file": (i32, [vp, vp, c.POINTER(c.c_char_p), c.c_char_p, c.c_char_p, c.c_char_p, c.POINTER(MapParams), i32, i32, i64,
                               c.POINTER(MapFileStats)]),
        "asm_fastq_cut": (c.c_size_t, [vp, c.c_size_t, c.POINTER(i64)]),
        "asm_map_pairs_file": (i32, [vp, vp, c.POINTER(c.c_char_p), c.c_char_p, c.c_char_p, c.c_char_p, c.c_char_p, c.POINTER(MapParams),
                                     c.POINTER(PairParams), i64, c.POINTER(MapPairsFileStats)]),
        "asm_fastq_cut_n": (c.c_size_t, [vp, c.c_size_t, i64, c.POINTER(i64)]),
        "asm_map_file_sorted": (i32, [vp, vp, c.POINTER(c.c_char_p), c.c_char_p, c.c_char_p, c.c_char_p, c.POINTER(MapParams), i32, i32, i64,
                                      i64, c.POINTER(MapFileStats), c.POINTER(SamSortStats)]),
        "asm_map_pairs_file_sorted": (i32, [vp, vp, c.POINTER(c.c_char_p), c.c_char_p, c.c_char_p, c.c_char_p, c.c_char_p,
                                            c.POINTER(MapParams), c.POINTER(PairParams), i64, i64, c.POINTER(MapPairsFileStats),
                                            c.POINTER(SamSortStats)]),
        "asm_index_build_file": (i32, [vp, c.c_char_p, i32, i64, c.POINTER(vp), c.POINTER(IndexFileStats)]),
        "asm_index_n_seqs": (c.c_int32, [vp]),
        "asm_index_seq_len": (c.c_uint64, [vp, c.c_int32]),
        "asm_index_seq_name": (c.c_char_p, [vp, c.c_int32]),
        "asm_index_get_text": (i32, [vp, vp, c.c_uint64, c.c_uint64, vp]),
        "asm_fasta_cut": (c.c_size_t, [vp, c.c_size_t, i32, c.POINTER(i32)]),
        "asm_device_malloc": (i32, [vp, c.c_size_t, c.POINTER(vp)]),
        "asm_device_free": (i32, [vp, vp]),
        "asm_memcpy_d2h": (i32, [vp, vp, vp, c.c_size_t]),
        "asm_memcpy_h2d": (i32, [vp, vp, vp, c.c_size_t]),
        "asm_memset_async": (i32, [vp, vp, i32, c.c_size_t]),
        "asm_timer_create": (i32, [vp, c.POINTER(vp)]),
        "asm_timer_start": (i32, [vp, vp]),
        "asm_timer_stop": (i32, [vp, vp]),
        "asm_timer_elapsed_ms": (i32, [vp, vp, c.POINTER(c.c_float)]),
        "asm_timer_destroy": (i32, [vp, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError here = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    lib._asm_symbols = tuple(sigs)
    _lib = lib
    return lib


def device_count() -> int:
    return int(load_library().asm_device_count())


@dataclass
class HostBatch:
    """A batch of read pairs in the C ABI's layout: concatenated ASCII + n+1 prefix offsets."""

    reads: np.ndarray     # uint8
    read_off: np.ndarray  # uint32, n+1
    refs: np.ndarray      # uint8
    ref_off: np.ndarray   # uint32, n+1

    @property
    def n(self) -> int:
        return int(self.read_off.shape[0] - 1)

    @classmethod
    def from_strings(cls, pairs: Iterable[Tuple[str, str]]) -> "HostBatch":
        pairs = list(pairs)
        ro = np.zeros(len(pairs) + 1, np.uint32)
        fo = np.zeros(len(pairs) + 1, np.uint32)
        if pairs:
            ro[1:] = np.cumsum([len(p[0]) for p in pairs])
            fo[1:] = np.cumsum([len(p[1]) for p in pairs])
        reads = np.frombuffer("".join(p[0] for p in pairs).encode("ascii"), np.uint8).copy()
        refs = np.frombuffer("".join(p[1] for p in pairs).encode("ascii"), np.uint8).copy()
        return cls(reads, ro, refs, fo)

    def pair(self, i: int) -> Tuple[str, str]:
        a = self.reads[self.read_off[i]:self.read_off[i + 1]].tobytes().decode("ascii")
        b = self.refs[self.ref_off[i]:self.ref_off[i + 1]].tobytes().decode("ascii")
        return a, b

    def slice(self, lo: int, hi: int) -> "HostBatch":
        ro = self.read_off[lo:hi + 1].astype(np.int64)
        fo = self.ref_off[lo:hi + 1].astype(np.int64)
        return HostBatch(self.reads[ro[0]:ro[-1]].copy(), (ro - ro[0]).astype(np.uint32),
                         self.refs[fo[0]:fo[-1]].copy(), (fo - fo[0]).astype(np.uint32))

    def lengths(self) -> Tuple[np.ndarray, np.ndarray]:
        return np.diff(self.read_off.astype(np.int64)), np.diff(self.ref_off.astype(np.int64))

    @classmethod
    def read_seq_file(cls, path: str, max_pairs: Optional[int] = None) -> "HostBatch":
        """The harness's input format (benchmark_utils.h:325-352): line 2i = '>'+read, 2i+1 = '<'+ref; the
        first character of every line is skipped blindly."""
        pairs = []
        with open(path, "r") as fh:
            while max_pairs is None or len(pairs) < max_pairs:
                a = fh.readline()
                if not a:
                    break
                b = fh.readline()
                pairs.append((a.rstrip("\n")[1:], b.rstrip("\n")[1:]))
        return cls.from_strings(pairs)

    def write_seq_file(self, path: str) -> None:
        """benchmark_dataset.h:229,234 — '>%s\\n<%s\\n'."""
        with open(path, "w") as fh:
            for i in range(self.n):
                a, b = self.pair(i)
                fh.write(f">{a}\n<{b}\n")


def generate_pairs(cfg: GenConfig, first: int, n: int) -> HostBatch:
    """Host generator (asm_generate_pairs): pairs [first, first+n) of the seeded stream.  Needs no GPU."""
    lib = load_library()
    ro = np.zeros(n + 1, np.uint32)
    fo = np.zeros(n + 1, np.uint32)
    rc = lib.asm_generate_pairs(ctypes.byref(cfg), first, n, ro.ctypes.data, fo.ctypes.data, None, 0, None, 0)
    if rc:
        raise AsmError(rc, lib.asm_last_error(None).decode())
    reads = np.zeros(max(int(ro[-1]), 1), np.uint8)
    refs = np.zeros(max(int(fo[-1]), 1), np.uint8)
    rc = lib.asm_generate_pairs(ctypes.byref(cfg), first, n, ro.ctypes.data, fo.ctypes.data, reads.ctypes.data,
                                reads.size, refs.ctypes.data, refs.size)
    if rc:
        raise AsmError(rc, lib.asm_last_error(None).decode())
    return HostBatch(reads[:int(ro[-1])], ro, refs[:int(fo[-1])], fo)


class DeviceBatch:
    """asm_batch: a device-resident batch (ASCII + packed bit planes)."""

    def __init__(self, engine: "Engine", ptr: int):
        self.engine, self.ptr = engine, ptr
        self.n = int(engine.lib.asm_batch_size(ptr))
        self.max_length = int(engine.lib.asm_batch_max_length(ptr))
        self.ascii_bytes = int(engine.lib.asm_batch_text_bytes(ptr))

    def free(self) -> None:
        if self.ptr:
            self.engine.lib.asm_batch_free(self.engine.h, self.ptr)
            self.ptr = None

    def download(self) -> HostBatch:
        lib, h = self.engine.lib, self.engine.h
        ro = np.zeros(self.n + 1, np.uint32)
        fo = np.zeros(self.n + 1, np.uint32)
        self.engine._chk(lib.asm_batch_download(h, self.ptr, ro.ctypes.data, fo.ctypes.data, None, 0, None, 0))
        reads = np.zeros(max(int(ro[-1]), 1), np.uint8)
        refs = np.zeros(max(int(fo[-1]), 1), np.uint8)
        self.engine._chk(lib.asm_batch_download(h, self.ptr, None, None, reads.ctypes.data, reads.size,
                                                refs.ctypes.data, refs.size))
        return HostBatch(reads[:int(ro[-1])], ro, refs[:int(fo[-1])], fo)

    def download_planes(self):
        """The packed form: (planes uint32[4 * entries, 4], lens uint32[n], order uint32[n]), lens and order in bucketed order
        (order = bucket slot -> pair index).  Bucket b's planes are a uint4[4][w4][size] block, buckets back to back."""
        lib, h = self.engine.lib, self.engine.h
        planes = np.zeros((int(lib.asm_batch_planes_size(self.ptr)), 4), np.uint32)
        lens = np.zeros(max(self.n, 1), np.uint32)
        order = np.zeros(max(self.n, 1), np.uint32)
        self.engine._chk(lib.asm_batch_download_planes(h, self.ptr, planes.ctypes.data, planes.size, lens.ctypes.data,
                                                       order.ctypes.data))
        return planes, lens[:self.n], order[:self.n]

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Reference:
    """asm_reference: a reference text resident in HBM."""

    def __init__(self, engine: "Engine", ptr, length: int):
        self.engine, self.ptr, self.length = engine, ptr, length

    def free(self) -> None:
        if self.ptr:
            self.engine.lib.asm_reference_free(self.engine.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Index:
    """asm_index: a k-mer index of reference sequences, resident in HBM."""

    def __init__(self, engine: "Engine", ptr, k: int, lengths: Sequence[int], names: Optional[Sequence[str]] = None):
        self.engine, self.ptr, self.k, self.lengths = engine, ptr, k, list(lengths)
        self.names = [""] * len(self.lengths) if names is None else list(names)

    def text(self, start: int, n: int) -> bytes:
        """asm_index_get_text: bytes [start, start + n) of the upper-cased text, by global offsets."""
        buf = ctypes.create_string_buffer(max(int(n), 1))
        self.engine._chk(self.engine.lib.asm_index_get_text(self.engine.h, self.ptr, int(start), int(n), buf))
        return buf.raw[:int(n)]

    def free(self) -> None:
        if self.ptr:
            self.engine.lib.asm_index_free(self.engine.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """asm_handle: one per GPU.  All device work of the hot path goes through here."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.asm_create(ctypes.byref(h), device)
        if rc:
            raise AsmError(rc, self.lib.asm_last_error(None).decode())
        self.h = h
        self.device = device

    def _chk(self, rc: int) -> None:
        if rc:
            raise AsmError(rc, self.lib.asm_last_error(self.h).decode())

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.asm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: Optional[int]) -> None:
        """Launch on a caller-owned hipStream_t.  0/None is HIP's legacy default stream (torch's `current_stream().cuda_stream`
        outside a stream context), not "the engine's own stream" — that is `reset_stream()`."""
        self._chk(self.lib.asm_set_stream(self.h, hip_stream or None))

    def reset_stream(self) -> None:
        self._chk(self.lib.asm_reset_stream(self.h))

    def synchronize(self) -> None:
        self._chk(self.lib.asm_synchronize(self.h))

    # ---- batches ----
    def upload(self, hb: HostBatch, greedy_mode: int = GREEDY_CLEAN) -> DeviceBatch:
        ptr = ctypes.c_void_p()
        reads = np.ascontiguousarray(hb.reads, np.uint8)
        refs = np.ascontiguousarray(hb.refs, np.uint8)
        ro = np.ascontiguousarray(hb.read_off, np.uint32)
        fo = np.ascontiguousarray(hb.ref_off, np.uint32)
        self._chk(self.lib.asm_batch_upload(self.h, hb.n, reads.ctypes.data, ro.ctypes.data, refs.ctypes.data,
                                            fo.ctypes.data, greedy_mode, ctypes.byref(ptr)))
        return DeviceBatch(self, ptr)

    def generate(self, cfg: GenConfig, first: int, n: int, greedy_mode: int = GREEDY_CLEAN) -> DeviceBatch:
        ptr = ctypes.c_void_p()
        self._chk(self.lib.asm_batch_generate(self.h, ctypes.byref(cfg), first, n, greedy_mode, ctypes.byref(ptr)))
        return DeviceBatch(self, ptr)

    def batch_from_text(self, text, greedy_mode: int = GREEDY_CLEAN) -> DeviceBatch:
        """asm_batch_from_text: a batch out of the harness's file format held in memory (bytes / uint8 array); the raw text
        goes to the GPU as it is and is parsed there."""
        buf = np.frombuffer(text.encode("ascii") if isinstance(text, str) else bytes(text), np.uint8) \
            if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        ptr = ctypes.c_void_p()
        self._chk(self.lib.asm_batch_from_text(self.h, buf.ctypes.data if buf.size else None, buf.size, greedy_mode,
                                               ctypes.byref(ptr)))
        return DeviceBatch(self, ptr)

    def stream_seq_file(self, path: str, params: Params, greedy_mode: int = GREEDY_SEQUENTIAL,
                        aligners: Sequence[int] = (NW, LEAP, GREEDY), chunk_bytes: int = 0, max_pairs: int = 0,
                        capacity: Optional[int] = None, answers: Optional[np.ndarray] = None):
        """asm_stream_seq_file: `benchmark::read_string_file` + `run` (benchmark_utils.h:325-385) for a file of any size, streamed
        through pinned buffers with the parse, the pack and the aligners of one chunk overlapping the transfer of the next.
        -> (dict aligner -> int32[pairs], StreamStats).  capacity: entries of the result arrays (default: max_pairs, or an upper
        bound from the file size: a pair takes at least two bytes, the newlines of two lines of zero bytes, which the parser
        reads as two empty strings, so a file of B bytes holds at most B // 2 + 1 pairs)."""
        if capacity is None:
            try:
                capacity = max_pairs if max_pairs > 0 else os.path.getsize(path) // 2 + 16
            except OSError:
                capacity = 16  # the library reports the unreadable file (benchmark_utils.h:350 only prints)
        mask = sum(1 << a for a in aligners)
        out = {a: np.zeros(capacity, np.int32) for a in aligners}
        st = StreamStats()
        ans = None if answers is None else np.ascontiguousarray(answers, np.int32)
        ptr = lambda a: out[a].ctypes.data if a in out else None  # noqa: E731
        self._chk(self.lib.asm_stream_seq_file(self.h, path.encode(), ctypes.byref(params), greedy_mode, mask, chunk_bytes, max_pairs,
                                               ptr(NW), ptr(LEAP), ptr(GREEDY), capacity, None if ans is None else ans.ctypes.data,
                                               0 if ans is None else ans.size, ctypes.byref(st)))
        return {a: v[:st.pairs] for a, v in out.items()}, st

    def upload_reference(self, text) -> "Reference":
        """Reference text (bytes / str / uint8 array) resident in HBM for seed-hit batches."""
        buf = np.frombuffer(text.encode("ascii") if isinstance(text, str) else bytes(text), np.uint8)
        ptr = ctypes.c_void_p()
        self._chk(self.lib.asm_reference_upload(self.h, buf.ctypes.data, buf.size, ctypes.byref(ptr)))
        return Reference(self, ptr, buf.size)

    def batch_from_hits(self, ref: "Reference", reads: np.ndarray, read_off: np.ndarray, hit_pos: np.ndarray,
                        greedy_mode: int = GREEDY_CLEAN) -> DeviceBatch:
        """The mapper's call shape (GASMA/mapper/main.cpp:77-86): pair i = (read i, reference window at hit_pos[i])."""
        reads = np.ascontiguousarray(reads, np.uint8)
        ro = np.ascontiguousarray(read_off, np.uint32)
        pos = np.ascontiguousarray(hit_pos, np.uint64)
        ptr = ctypes.c_void_p()
        self._chk(self.lib.asm_batch_from_hits(self.h, ref.ptr, ro.size - 1, reads.ctypes.data, ro.ctypes.data,
                                               pos.ctypes.data, greedy_mode, ctypes.byref(ptr)))
        return DeviceBatch(self, ptr)

    # ---- read mapping (docs/design/mapper.md) ----
    def build_index(self, seqs, k: int = 12) -> Index:
        """asm_index_build over reference sequences (str / bytes, upper-cased on the device)."""
        text, off = pack_sequences(seqs)
        ptr = ctypes.c_void_p()
        self._chk(self.lib.asm_index_build(self.h, text.ctypes.data if text.size else None, off.ctypes.data, len(off) - 1, int(k),
                                           ctypes.byref(ptr)))
        return Index(self, ptr, int(k), np.diff(off).astype(np.int64))

    def build_index_file(self, path: str, k: int = 12, chunk_bytes: int = 0):
        """asm_index_build_file: the index of a FASTA file, read, parsed and indexed without a host copy of the text
        (docs/design/mapper.md, "Reference: FASTA in, index out").  -> (Index with .names and .lengths from the file, the stats as a
        dict: n_seqs, bases, bytes_in, chunks, seconds, seconds_read, seconds_index)."""
        ptr, st = ctypes.c_void_p(), IndexFileStats()
        self._chk(self.lib.asm_index_build_file(self.h, os.fsencode(path), int(k), int(chunk_bytes), ctypes.byref(ptr), ctypes.byref(st)))
        n = self.lib.asm_index_n_seqs(ptr)
        index = Index(self, ptr, int(k), [int(self.lib.asm_index_seq_len(ptr, r)) for r in range(n)],
                      [self.lib.asm_index_seq_name(ptr, r).decode("latin-1") for r in range(n)])
        return index, {name: getattr(st, name) for name, _ in IndexFileStats._fields_}

    def set_mapq_model(self, model) -> None:
        """asm_map_set_mapq_model: MAPQ_REFERENCE / "reference" (the default, min(254, 60 + greedy_cost)) or MAPQ_GAP / "gap" (the
        repeat- and pair-aware model of docs/design/mapper.md, "Mapping quality") for every later map_* call of this engine."""
        self._chk(self.lib.asm_map_set_mapq_model(self.h, {"reference": MAPQ_REFERENCE, "gap": MAPQ_GAP}.get(model, model)))

    def mapq_model(self) -> int:
        return int(self.lib.asm_map_get_mapq_model(self.h))

    def set_sam_tags(self, md: bool = False) -> None:
        """asm_map_set_sam_tags: the optional tags of the lines map_file and map_pairs_file write (sorted or not).  md=True: every
        line that shows a CIGAR carries MD:Z behind XG (docs/design/mapper.md, "MD tag"), built on the device.  The default, nothing
        set, leaves every byte as it is.  The in-memory map_* calls carry no MD; md_format gives it from their records."""
        self._chk(self.lib.asm_map_set_sam_tags(self.h, SAM_TAG_MD if md else 0))

    @property
    def sam_tags(self) -> int:
        """asm_map_get_sam_tags: the mask in force (SAM_TAG_MD)"""
        return int(self.lib.asm_map_get_sam_tags(self.h))

    def set_output_format(self, fmt) -> None:
        """asm_map_set_output_format: OUT_SAM / "sam" (the default) or OUT_BAM / "bam": what map_file and map_pairs_file (sorted or
        not) write to sam_path.  BAM: the records encoded and BGZF-framed (stored blocks) on the device, and what they say is what
        the SAM lines say (docs/design/mapper.md, "BAM output")."""
        self._chk(self.lib.asm_map_set_output_format(self.h, {"sam": OUT_SAM, "bam": OUT_BAM}.get(fmt, fmt)))

    @property
    def output_format(self) -> int:
        """asm_map_get_output_format: the format in force (OUT_SAM, OUT_BAM)"""
        return int(self.lib.asm_map_get_output_format(self.h))

    def bgzf_frame(self, data: bytes, eof: bool = True) -> bytes:
        """asm_bgzf_frame: data in BGZF blocks of BGZF_PAYLOAD bytes (stored deflate, the last one shorter, none for b""), framed
        by the device kernel of the BAM file calls; eof: the 28-byte EOF block behind them.  gzip.decompress gives data back."""
        data = bytes(data)
        cap = int(self.lib.asm_bgzf_bound(len(data), int(eof)))
        out = ctypes.create_string_buffer(max(cap, 1))
        got = ctypes.c_size_t(0)
        self._chk(self.lib.asm_bgzf_frame(self.h, data if data else None, len(data), int(eof), out, cap, ctypes.byref(got)))
        return out.raw[: got.value]

    def set_bgzf_level(self, level) -> None:
        """asm_map_set_bgzf_level: BGZF_STORED / "stored" (the default) or BGZF_DEFLATE / "deflate": the blocks of the BAM file the
        file calls write.  Deflate: every block encoded on the device as the smallest of a stored, a fixed-Huffman and a
        dynamic-Huffman deflate block (docs/design/mapper.md, "Deflate"); the uncompressed stream and its cut stay the same.  No
        effect under OUT_SAM."""
        self._chk(self.lib.asm_map_set_bgzf_level(self.h, {"stored": BGZF_STORED, "deflate": BGZF_DEFLATE}.get(level, level)))

    def get_bgzf_level(self) -> int:
        """asm_map_get_bgzf_level: the level in force (BGZF_STORED, BGZF_DEFLATE)"""
        return int(self.lib.asm_map_get_bgzf_level(self.h))

    def set_bam_index(self, kind) -> None:
        """asm_map_set_bam_index: BAM_INDEX_NONE / "none" (the default) or BAM_INDEX_BAI / "bai": under OUT_BAM the sorted file calls
        then write `<sam_path>.bai` beside the BAM file, a BAI index built on the device (docs/design/mapper.md, "BAM index").  No
        effect under OUT_SAM or in the unsorted calls."""
        self._chk(self.lib.asm_map_set_bam_index(self.h, {"none": BAM_INDEX_NONE, "bai": BAM_INDEX_BAI}.get(kind, kind)))

    @property
    def bam_index(self) -> int:
        """asm_map_get_bam_index: the kind in force (BAM_INDEX_NONE, BAM_INDEX_BAI)"""
        return int(self.lib.asm_map_get_bam_index(self.h))

    def last_bam_index(self) -> dict:
        """asm_map_last_bam_index: refs, bins, chunks, intervals, no_coor, bytes and seconds_index of the last sorted BAM call of
        this engine that wrote an index; all zero before one"""
        st = BamIndexStats()
        self._chk(self.lib.asm_map_last_bam_index(self.h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in BamIndexStats._fields_}

    def bgzf_compress(self, data: bytes, eof: bool = True, level: int = BGZF_DEFLATE) -> bytes:
        """asm_bgzf_compress: bgzf_frame with a level, by the device kernels of the BAM file calls.  Level BGZF_STORED gives
        bgzf_frame's bytes; BGZF_DEFLATE the bytes of bgzf_compress_host.  gzip.decompress gives data back."""
        data = bytes(data)
        cap = int(self.lib.asm_bgzf_bound(len(data), int(eof)))
        out = ctypes.create_string_buffer(max(cap, 1))
        got = ctypes.c_size_t(0)
        self._chk(self.lib.asm_bgzf_compress(self.h, data if data else None, len(data), int(eof), int(level), out, cap, ctypes.byref(got)))
        return out.raw[: got.value]

    def bgzf_decompress(self, data: bytes) -> bytes:
        """asm_bgzf_decompress: a BGZF container (what bgzip, bgzf_compress and the BAM file calls write) decoded by the device's
        deflate decoder, one wavefront per member; the bytes of bgzf_decompress_host.  Corrupt input raises AsmError naming the
        member; plain gzip is refused (docs/design/mapper.md, "Compressed input")."""
        data = bytes(data)
        cap = bgzf_decompressed_size(data)
        out = ctypes.create_string_buffer(max(cap, 1))
        got = ctypes.c_size_t(0)
        self._chk(self.lib.asm_bgzf_decompress(self.h, data if data else None, len(data), out, cap, ctypes.byref(got)))
        return out.raw[: got.value]

    def last_mapq(self, count: int) -> np.ndarray:
        """asm_map_last_mapq: uint8[count], the MAPQ of every record slot of the last in-memory library call, in its `out` layout"""
        out = np.zeros(int(count), np.uint8)
        self._chk(self.lib.asm_map_last_mapq(self.h, out.ctypes.data if count else None, int(count)))
        return out

    def _map_chunks(self, parts, chunk: Optional[int], call, slots: int = 1) -> np.ndarray:
        """The chunk loop of the map_* methods.  parts: one list of byte strings per mate; call(lo, hi, seqs) maps reads [lo, hi)
        and returns the library's code; seqs: per list the address of the packed bytes (None when empty) and of their uint32
        offsets.  -> uint8 (n, slots): the MAPQ of every record slot by the engine's model (asm_map_last_mapq after every call)."""
        n = len(parts[0])
        step = chunk if chunk else max(n, 1)
        mq = np.zeros((n, slots), np.uint8)
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            packed = [(buf, off.astype(np.uint32)) for buf, off in (pack_sequences(p[lo:hi]) for p in parts)]
            seqs = [x for buf, ro in packed for x in (buf.ctypes.data if buf.size else None, ro.ctypes.data)]
            self._chk(call(lo, hi, seqs))
            mq[lo:hi] = self.last_mapq((hi - lo) * slots).reshape(hi - lo, slots)
        return mq

    @staticmethod
    def _mates(reads1, reads2):
        p1, p2 = [_as_bytes(r) for r in reads1], [_as_bytes(r) for r in reads2]
        if len(p1) != len(p2):
            raise ValueError("reads1 and reads2 must hold the same number of mates")
        return p1, p2

    @staticmethod
    def _cigar_args(ops: np.ndarray, nops: np.ndarray, cigar_cap: int, lo: int, hi: int):
        """cigar_ops, cigar_cap, cigar_nops of a library call that writes records [lo, hi) of the full arrays"""
        return (ops[lo:hi].ctypes.data if cigar_cap else None, int(cigar_cap), nops[lo:hi].ctypes.data if cigar_cap else None)

    @staticmethod
    def _hit_fields(hits: np.ndarray, rescued: bool = False) -> dict:
        """the record fields as arrays of hits' shape, plus mapped, mapq (255 when unmapped) and, for the paired calls, rescued"""
        out = {name: hits[name].copy() for name in MAP_HIT_DTYPE.names}
        out["mapped"] = (hits["flags"] & MAP_MAPPED) != 0
        if rescued:
            out["rescued"] = (hits["flags"] & MAP_RESCUED) != 0
        # kept for compatibility: always the reference rule, 255 when unmapped.  The value to use is `mapping_quality`, which the
        # map_* methods add: the library's MAPQ by the engine's model (set_mapq_model), 0 when unmapped, as the SAM files carry it.
        out["mapq"] = np.where(out["mapped"], np.minimum(254, 60 + hits["greedy_cost"].astype(np.int64)), 255).astype(np.int32)
        return out

    @staticmethod
    def _cigars(ops: np.ndarray, nops: np.ndarray, cigar_cap: int):
        """one CIGAR string per record of nops, flat ('' for all when cigar_cap is 0)"""
        if not (cigar_cap and nops.size):
            return [""] * nops.size
        # a record whose row did not fit carries MAP_CIGAR_TRUNCATED and cigar_nops > cigar_cap: its string is the stored prefix
        return decode_cigars(ops.reshape(nops.size, -1), nops.reshape(-1), cigar_cap, truncated="prefix")

    def map_reads(self, index: Index, reads, max_errors: int, both_strands: bool = True, max_occ: int = 0, greedy_k: int = 3,
                  cigar_cap: int = 64, chunk: Optional[int] = None):
        """asm_map_reads: the best hit of every read (str / bytes).  -> dict of numpy arrays, one entry per read: seq_id, pos, end,
        dist, strand, flags, greedy_cost, mapped (bool), mapq (min(254, 60 + greedy_cost), 255 when unmapped), and `cigar`, a
        list of CIGAR strings ('' when unmapped), and mapping_quality.  mapping_quality (uint8) is the MAPQ to use: the library's
        value by the engine's model (set_mapq_model), 0 when unmapped, the number the SAM files carry in column 5; every map_*
        sibling has it in the shape of its records.  The older `mapq` is kept for compatibility and is always the reference rule.  chunk: reads per library call (None: all in one)."""
        parts = [_as_bytes(r) for r in reads]
        n = len(parts)
        p = MapParams(int(max_errors), 1 if both_strands else 0, int(max_occ), int(greedy_k))
        hits = np.zeros(n, MAP_HIT_DTYPE)
        ops = np.zeros((n, max(cigar_cap, 1)), np.uint16)
        nops = np.zeros(n, np.uint8)
        mq = self._map_chunks([parts], chunk, lambda lo, hi, seqs: self.lib.asm_map_reads(
            self.h, index.ptr, hi - lo, *seqs, ctypes.byref(p), hits[lo:hi].ctypes.data, *self._cigar_args(ops, nops, cigar_cap, lo, hi)))
        out = self._hit_fields(hits)
        out["mapping_quality"] = mq.reshape(n)
        out["cigar"] = self._cigars(ops, nops, cigar_cap)
        out["cigar_nops"] = nops
        return out

    def map_reads_all(self, index: Index, reads, max_errors: int, max_hits: int = 16, strata: Optional[int] = None,
                      both_strands: bool = True, max_occ: int = 0, greedy_k: int = 3, cigar_cap: int = 64, chunk: Optional[int] = None):
        """asm_map_reads_all: every locus within max_errors (docs/design/mapper.md, "All hits").  strata=None means max_errors
        (all loci).  -> dict: per read `n_hits` (uncapped), `n_reported` and `read_flags` (the rank-0 record's flags, also for an
        unmapped read: TOO_SHORT, SEED_CAPPED); flat per-hit arrays in read-then-rank order: read,
        rank, seq_id, pos, end, dist, strand, flags, greedy_cost, mapq (min(254, 60 + greedy_cost)), `cigar`, a list of CIGAR
        strings, and cigar_nops (the uncapped number of operations).  chunk: reads per library call (None: all in one)."""
        parts = [_as_bytes(r) for r in reads]
        n = len(parts)
        strata = int(max_errors) if strata is None else int(strata)
        p = MapParams(int(max_errors), 1 if both_strands else 0, int(max_occ), int(greedy_k))
        n_hits = np.zeros(n, np.uint32)
        hits = np.zeros((n, max_hits), MAP_HIT_DTYPE)
        ops = np.zeros((n, max_hits, max(cigar_cap, 1)), np.uint16)
        nops = np.zeros((n, max_hits), np.uint8)
        mq = self._map_chunks([parts], chunk, lambda lo, hi, seqs: self.lib.asm_map_reads_all(
            self.h, index.ptr, hi - lo, *seqs, ctypes.byref(p), strata, int(max_hits), n_hits[lo:hi].ctypes.data,
            hits[lo:hi].ctypes.data, *self._cigar_args(ops, nops, cigar_cap, lo, hi)), slots=int(max_hits))
        n_rep = np.minimum(n_hits, max_hits).astype(np.int64)
        read = np.repeat(np.arange(n, dtype=np.int64), n_rep)
        rank = (np.arange(read.size, dtype=np.int64) - np.repeat(np.cumsum(n_rep) - n_rep, n_rep)) if read.size else read.copy()
        flat = hits[read, rank]
        out = {"n_hits": n_hits, "n_reported": n_rep, "read_flags": hits["flags"][:, 0].copy(), "read": read, "rank": rank}
        out.update({name: flat[name].copy() for name in MAP_HIT_DTYPE.names})
        # kept for compatibility: always the reference rule; `mapping_quality` below is the value to use
        out["mapq"] = np.minimum(254, 60 + flat["greedy_cost"].astype(np.int64)).astype(np.int32)
        out["mapping_quality"] = mq[read, rank]
        out["cigar"] = self._cigars(ops[read, rank], nops[read, rank], cigar_cap)
        out["cigar_nops"] = nops[read, rank]
        return out

    @staticmethod
    def _rnames(index: Index, names):
        """seq_names of the two file calls: one RNAME per sequence of the index, as a C array"""
        names = [_as_bytes(nm) for nm in names]
        if len(names) != len(index.lengths):
            raise ValueError("names must hold one name per sequence of the index")
        return (ctypes.c_char_p * max(len(names), 1))(*names)

    def map_file(self, index: Index, names, fastq_path: str, sam_path: str, max_errors: int, both_strands: bool = True,
                 max_occ: int = 0, greedy_k: int = 3, max_hits: int = 0, strata: Optional[int] = None, chunk_bytes: int = 0,
                 header: Optional[str] = None, sort: bool = False, max_device_bytes: int = 0) -> dict:
        """asm_map_file: a four-line FASTQ file in, a SAM file out, parsed, mapped and formatted on the device (docs/design/mapper.md,
        "Files: FASTQ in, SAM out").  names: one RNAME per sequence of the index.  max_hits=0: the best hit per read (map_reads);
        1..256: the loci of map_reads_all with strata (None: max_errors).  header is written first, as it is.  -> the stats as a dict:
        reads, mapped, too_long, records (SAM lines), chunks, bytes_in, bytes_out, seconds, seconds_read, seconds_write.
        sort=True: asm_map_file_sorted, the same lines in coordinate order ("Sorted output"; max_device_bytes caps what is held on
        the device, 0: no cap); the dict then holds the sort's stats too, under "sort": lines, bytes_held, slabs, seconds_sort."""
        arr = self._rnames(index, names)
        p = MapParams(int(max_errors), 1 if both_strands else 0, int(max_occ), int(greedy_k))
        st = MapFileStats()
        strata = int(max_errors) if strata is None else int(strata)
        args = (self.h, index.ptr, arr, os.fsencode(fastq_path), os.fsencode(sam_path), None if header is None else _as_bytes(header),
                ctypes.byref(p), int(max_hits), strata, int(chunk_bytes))
        if not sort:
            self._chk(self.lib.asm_map_file(*args, ctypes.byref(st)))
            return {name: getattr(st, name) for name, _ in MapFileStats._fields_}
        sst = SamSortStats()
        self._chk(self.lib.asm_map_file_sorted(*args, int(max_device_bytes), ctypes.byref(st), ctypes.byref(sst)))
        return dict({name: getattr(st, name) for name, _ in MapFileStats._fields_},
                    sort={name: getattr(sst, name) for name, _ in SamSortStats._fields_})

    def map_pairs_file(self, index: Index, names, fastq1_path: str, fastq2_path: str, sam_path: str, max_errors: int, min_insert: int,
                       max_insert: int, rescue_errors: int = -1, max_occ: int = 0, greedy_k: int = 3, chunk_bytes: int = 0,
                       header: Optional[str] = None, sort: bool = False, max_device_bytes: int = 0) -> dict:
        """asm_map_pairs_file: two four-line FASTQ files in (record i of each: the mates of pair i), a paired SAM file out, parsed,
        paired, mapped and formatted on the device (docs/design/mapper.md, "Files: two FASTQ files in, paired SAM out"); the answer
        is map_pairs'.  names: one RNAME per sequence of the index.  header is written first, as it is.  -> the stats as a dict:
        pairs, proper, rescued, unsent, records (SAM lines), chunks, bytes_in, bytes_out, carry_peak, seconds, seconds_read,
        seconds_write.  sort=True: asm_map_pairs_file_sorted, the same lines in coordinate order; max_device_bytes and the "sort" entry
        of the dict as for map_file.  Two bgzip-compressed (BGZF) files are taken as they are and inflated on the device; the bytes
        written are those of the call on the inflated texts, and carry_peak then counts text bytes held on the device
        (docs/design/mapper.md, "Compressed input for pairs").  One compressed and one text file, or plain gzip: AsmError."""
        arr = self._rnames(index, names)
        p = MapParams(int(max_errors), 1, int(max_occ), int(greedy_k))
        pp = PairParams(int(min_insert), int(max_insert), int(rescue_errors))
        st = MapPairsFileStats()
        args = (self.h, index.ptr, arr, os.fsencode(fastq1_path), os.fsencode(fastq2_path), os.fsencode(sam_path),
                None if header is None else _as_bytes(header), ctypes.byref(p), ctypes.byref(pp), int(chunk_bytes))
        if not sort:
            self._chk(self.lib.asm_map_pairs_file(*args, ctypes.byref(st)))
            return {name: getattr(st, name) for name, _ in MapPairsFileStats._fields_}
        sst = SamSortStats()
        self._chk(self.lib.asm_map_pairs_file_sorted(*args, int(max_device_bytes), ctypes.byref(st), ctypes.byref(sst)))
        return dict({name: getattr(st, name) for name, _ in MapPairsFileStats._fields_},
                    sort={name: getattr(sst, name) for name, _ in SamSortStats._fields_})

    def map_pairs(self, index: Index, reads1, reads2, max_errors: int, min_insert: int, max_insert: int, rescue_errors: int = -1,
                  max_occ: int = 0, greedy_k: int = 3, cigar_cap: int = 64, chunk: Optional[int] = None):
        """asm_map_pairs: paired-end reads, FR orientation (docs/design/mapper.md, "Paired-end reads"); reads1[i] and reads2[i]
        are the two mates of pair i, both strands are searched.  -> dict of (n, 2) arrays, column 0 mate 1 and column 1 mate 2:
        seq_id, pos, end, dist, strand, flags, greedy_cost, mapq (min(254, 60 + greedy_cost), 255 when unmapped), mapped and
        rescued (bool), `cigar` (n lists of 2 CIGAR strings); per pair: proper (bool), tlen and n_concordant.  chunk: pairs per
        library call (None: all in one)."""
        mates = self._mates(reads1, reads2)
        n = len(mates[0])
        p = MapParams(int(max_errors), 1, int(max_occ), int(greedy_k))
        pp = PairParams(int(min_insert), int(max_insert), int(rescue_errors))
        hits = np.zeros((n, 2), MAP_HIT_DTYPE)
        tlen = np.zeros(n, np.int32)
        n_conc = np.zeros(n, np.uint32)
        ops = np.zeros((n, 2, max(cigar_cap, 1)), np.uint16)
        nops = np.zeros((n, 2), np.uint8)
        mq = self._map_chunks(mates, chunk, lambda lo, hi, seqs: self.lib.asm_map_pairs(
            self.h, index.ptr, hi - lo, *seqs, ctypes.byref(p), ctypes.byref(pp), hits[lo:hi].ctypes.data, tlen[lo:hi].ctypes.data,
            n_conc[lo:hi].ctypes.data, *self._cigar_args(ops, nops, cigar_cap, lo, hi)), slots=2)
        out = self._hit_fields(hits, rescued=True)
        out["mapping_quality"] = mq
        out["proper"] = (hits["flags"][:, 0] & MAP_PROPER_PAIR) != 0
        out["tlen"], out["n_concordant"] = tlen, n_conc
        flat = self._cigars(ops, nops, cigar_cap)
        out["cigar"] = [[flat[2 * t], flat[2 * t + 1]] for t in range(n)]
        out["cigar_nops"] = nops
        return out

    def map_pairs_all(self, index: Index, reads1, reads2, max_errors: int, min_insert: int, max_insert: int, max_pairs: int = 16,
                      strata: Optional[int] = None, rescue_errors: int = -1, max_occ: int = 0, greedy_k: int = 3, cigar_cap: int = 64,
                      chunk: Optional[int] = None):
        """asm_map_pairs_all: every concordant pair whose d sum is within strata of the best (docs/design/mapper.md, "Secondary
        pairs"); strata=None means 2 * max_errors (all concordant pairs).  -> dict: the fields of map_pairs shaped (n, max_pairs, 2)
        (rank, then mate 1 / mate 2): seq_id, pos, end, dist, strand, flags, greedy_cost, mapq, mapped, rescued, cigar_nops; per
        pair and rank (n, max_pairs): proper, tlen; per pair: n_pairs (uncapped), n_reported (min(n_pairs, max_pairs)) and
        n_concordant; `cigar`: n lists of max_pairs pairs of CIGAR strings.  Rank 0 is map_pairs' answer.  chunk: pairs per
        library call (None: all in one)."""
        mates = self._mates(reads1, reads2)
        n, P = len(mates[0]), int(max_pairs)
        strata = 2 * int(max_errors) if strata is None else int(strata)
        p = MapParams(int(max_errors), 1, int(max_occ), int(greedy_k))
        pp = PairParams(int(min_insert), int(max_insert), int(rescue_errors))
        hits = np.zeros((n, P, 2), MAP_HIT_DTYPE)
        tlen = np.zeros((n, P), np.int32)
        n_pairs = np.zeros(n, np.uint32)
        n_conc = np.zeros(n, np.uint32)
        ops = np.zeros((n, P, 2, max(cigar_cap, 1)), np.uint16)
        nops = np.zeros((n, P, 2), np.uint8)
        mq = self._map_chunks(mates, chunk, lambda lo, hi, seqs: self.lib.asm_map_pairs_all(
            self.h, index.ptr, hi - lo, *seqs, ctypes.byref(p), ctypes.byref(pp), strata, P, n_pairs[lo:hi].ctypes.data,
            hits[lo:hi].ctypes.data, tlen[lo:hi].ctypes.data, n_conc[lo:hi].ctypes.data, *self._cigar_args(ops, nops, cigar_cap, lo, hi)),
            slots=2 * P)
        out = self._hit_fields(hits, rescued=True)
        out["mapping_quality"] = mq.reshape(n, P, 2)
        out["proper"] = (hits["flags"][:, :, 0] & MAP_PROPER_PAIR) != 0
        out["tlen"], out["n_pairs"], out["n_concordant"] = tlen, n_pairs, n_conc
        out["n_reported"] = np.minimum(n_pairs, P).astype(np.int64)
        flat = self._cigars(ops, nops, cigar_cap)
        out["cigar"] = [[[flat[2 * (t * P + k)], flat[2 * (t * P + k) + 1]] for k in range(P)] for t in range(n)]
        out["cigar_nops"] = nops
        return out

    # ---- Greedy's sequential mode across batches (shards of one file / chunks of a stream) ----
    def tail_summary(self, batch: DeviceBatch) -> np.ndarray:
        """asm_batch_tail_summary: uint8[256], what this batch does to the reference's two persistent buffers."""
        out = np.zeros(256, np.uint8)
        self._chk(self.lib.asm_batch_tail_summary(self.h, batch.ptr, out.ctypes.data))
        return out

    def resolve_tails(self, batch: DeviceBatch, state: Optional[np.ndarray] = None) -> None:
        """asm_batch_resolve_tails: make `batch` a sequential-mode batch whose first pair sees `state` (uint8[256] of 2-bit
        codes; None = a file's start) in the buffers."""
        st = None if state is None else np.ascontiguousarray(state, np.uint8)
        if st is not None and st.size != 256:
            raise ValueError("state must have 256 entries")
        self._chk(self.lib.asm_batch_resolve_tails(self.h, batch.ptr, None if st is None else st.ctypes.data))

    def pack_async(self, batch: DeviceBatch) -> None:
        self._chk(self.lib.asm_batch_pack_async(self.h, batch.ptr))

    # ---- device memory ----
    def malloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        self._chk(self.lib.asm_device_malloc(self.h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, ptr: int) -> None:
        self._chk(self.lib.asm_device_free(self.h, ptr))

    def to_host(self, ptr: int, count: int, dtype=np.int32) -> np.ndarray:
        out = np.zeros(count, dtype)
        self._chk(self.lib.asm_memcpy_d2h(self.h, out.ctypes.data, ptr, out.nbytes))
        return out

    def memset_async(self, ptr: int, value: int, nbytes: int) -> None:
        self._chk(self.lib.asm_memset_async(self.h, ptr, value, nbytes))

    # ---- the hot path ----
    def align_async(self, batch: DeviceBatch, aligner: int, params: Params, d_out: int) -> None:
        """One aligner over a resident batch into a device int32[n] buffer (enqueue only)."""
        self._chk(self.lib.asm_align_batch_async(self.h, batch.ptr, aligner, ctypes.byref(params), d_out))

    def align_hinted_async(self, batch: DeviceBatch, aligner: int, params: Params, d_hint: Optional[int], d_out: int) -> None:
        """align_async with a per-pair work estimate (device int32[n]) that only steers scheduling."""
        self._chk(self.lib.asm_align_batch_hinted_async(self.h, batch.ptr, aligner, ctypes.byref(params), d_hint, d_out))

    def align(self, batch: DeviceBatch, aligner: int, params: Params) -> np.ndarray:
        d_out = self.malloc(4 * max(batch.n, 1))
        try:
            self.align_async(batch, aligner, params, d_out)
            return self.to_host(d_out, batch.n)
        finally:
            self.free(d_out)

    # ---- filtering stage: bit-parallel LEAP (SIMD_ED) and SHD (LEAP_SIMD/main.cpp:95-101,186-195) ----
    def simd_ed_async(self, batch: DeviceBatch, ed_threshold: int, d_ed: int, shd: bool = True, mode: int = FILTER_CLEAN,
                      state: Optional[Sequence[int]] = None, ed_mode: int = 0) -> Optional[Tuple[int, ...]]:
        """SIMD_ED::init_levenshtein(ed_threshold, ED_GLOBAL, shd) + load_reads/calculate_masks/reset/run per pair:
        d_ed[i] = get_ED() when check_pass() else -1.  state = (final_ED, lane distance, converge_ED) carried into the
        first pair in FILTER_SEQUENTIAL mode; returns the state after the last pair (for the next chunk of the same file).
        ed_mode: init_levenshtein's ED_modes (LEAP_GLOBAL, the filter driver's; LEAP_LOCAL / LEAP_SEMI_FREE_BEGIN / LEAP_SEMI_FREE_END)."""
        st = None
        if state is not None:
            st = (ctypes.c_int32 * 3)(*[int(v) for v in state])
        self._chk(self.lib.asm_simd_ed_mode_batch_async(self.h, batch.ptr, int(ed_threshold), 1 if shd else 0, int(mode), int(ed_mode),
                                                        st, d_ed))
        return tuple(st) if st is not None else None

    def simd_ed(self, batch: DeviceBatch, ed_threshold: int, shd: bool = True, mode: int = FILTER_CLEAN,
                state: Optional[Sequence[int]] = None, ed_mode: int = 0) -> np.ndarray:
        d_out = self.malloc(4 * max(batch.n, 1))
        try:
            self.simd_ed_async(batch, ed_threshold, d_out, shd, mode, state, ed_mode)
            return self.to_host(d_out, batch.n)
        finally:
            self.free(d_out)

    def simd_ed_affine_async(self, batch: DeviceBatch, gap_threshold: int, af_threshold: int, x: int, o: int, e: int, d_ed: int,
                             shd_threshold: Optional[int] = None, mode: int = 0) -> None:
        """SIMD_ED::init_affine(gap_threshold, af_threshold, ED_GLOBAL, x, o, e[, true, shd_threshold]) + load_reads/calculate_masks/
        reset/run per pair, every pair from clean tables: d_ed[i] = get_ED() when check_pass() (1000000 for a pair exact at e = 0)
        else -1.  shd_threshold: init_affine's SHD_enable = true with that SHD_threshold (None: off, the reference's default)."""
        if mode != 0:  # init_affine's ED_modes (LEAP_LOCAL / LEAP_SEMI_FREE_BEGIN / LEAP_SEMI_FREE_END)
            self._chk(self.lib.asm_simd_ed_affine_mode_batch_async(self.h, batch.ptr, int(gap_threshold), int(af_threshold), int(x),
                                                                   int(o), int(e), -1 if shd_threshold is None else int(shd_threshold),
                                                                   int(mode), d_ed))
        elif shd_threshold is None:
            self._chk(self.lib.asm_simd_ed_affine_batch_async(self.h, batch.ptr, int(gap_threshold), int(af_threshold), int(x), int(o),
                                                              int(e), d_ed))
        else:
            self._chk(self.lib.asm_simd_ed_affine_shd_batch_async(self.h, batch.ptr, int(gap_threshold), int(af_threshold), int(x),
                                                                  int(o), int(e), int(shd_threshold), d_ed))

    def simd_ed_affine(self, batch: DeviceBatch, gap_threshold: int, af_threshold: int, x: int, o: int, e: int,
                       shd_threshold: Optional[int] = None, mode: int = 0) -> np.ndarray:
        d_out = self.malloc(4 * max(batch.n, 1))
        try:
            self.simd_ed_affine_async(batch, gap_threshold, af_threshold, x, o, e, d_out, shd_threshold, mode)
            return self.to_host(d_out, batch.n)
        finally:
            self.free(d_out)

    def shd_filter_async(self, batch: DeviceBatch, max_error: int, d_pass: int) -> None:
        """bit_vec_filter_avx(read planes, ref planes, length, max_error): d_pass[i] in {0, 1}."""
        self._chk(self.lib.asm_shd_filter_batch_async(self.h, batch.ptr, int(max_error), d_pass))

    def shd_filter(self, batch: DeviceBatch, max_error: int) -> np.ndarray:
        d_out = self.malloc(4 * max(batch.n, 1))
        try:
            self.shd_filter_async(batch, max_error, d_out)
            return self.to_host(d_out, batch.n)
        finally:
            self.free(d_out)

    def align_host(self, hb: HostBatch, aligner: int, params: Params, greedy_mode: int = GREEDY_CLEAN) -> np.ndarray:
        """asm_align_batch: host in, host out — `align(read, ref, k)` for every pair of the batch."""
        out = np.zeros(hb.n, np.int32)
        reads = np.ascontiguousarray(hb.reads, np.uint8)
        refs = np.ascontiguousarray(hb.refs, np.uint8)
        ro = np.ascontiguousarray(hb.read_off, np.uint32)
        fo = np.ascontiguousarray(hb.ref_off, np.uint32)
        self._chk(self.lib.asm_align_batch(self.h, aligner, hb.n, reads.ctypes.data, ro.ctypes.data, refs.ctypes.data,
                                           fo.ctypes.data, ctypes.byref(params), greedy_mode, out.ctypes.data))
        return out

    def greedy_cigar_async(self, batch: DeviceBatch, params: Params, d_pen: int, d_ops: int, cap: int, d_nops: int) -> None:
        """asm_greedy_cigar_batch_async into caller buffers (enqueue only): d_pen = device int32[n], d_ops = device uint16[n][cap]
        (count << 3 | op, see decode_cigars), d_nops = device uint8[n] (above cap: the row was truncated and holds its first cap
        entries; the count saturates at 255, which means "255 or more": cigar_rows_truncated)."""
        self._chk(self.lib.asm_greedy_cigar_batch_async(self.h, batch.ptr, ctypes.byref(params), d_pen, d_ops, int(cap), d_nops))

    def greedy_with_cigar(self, batch: DeviceBatch, params: Params, cap: int = 48):
        """-> (costs int32[n], CIGAR strings, nops) — hurdle_matrix::get_cost / get_CIGAR for every pair of the batch.  ValueError when
        a row did not fit into cap entries (decode_cigars): a shortened string is not handed back as a CIGAR."""
        n = batch.n
        d_pen, d_ops, d_nops = self.malloc(4 * max(n, 1)), self.malloc(2 * cap * max(n, 1)), self.malloc(max(n, 1))
        try:
            self.greedy_cigar_async(batch, params, d_pen, d_ops, cap, d_nops)
            costs = self.to_host(d_pen, n)
            ops = self.to_host(d_ops, n * cap, np.uint16).reshape(n, cap)
            nops = self.to_host(d_nops, n, np.uint8)
        finally:
            for p in (d_pen, d_ops, d_nops):
                self.free(p)
        return costs, decode_cigars(ops, nops, cap), nops

    def coverage(self, batch: DeviceBatch, params: Params, window: int = 64, cap: int = 64, want_nw_cigars: bool = False,
                 nw_cap: Optional[int] = None):
        """The harness's coverage metric for every pair: -> dict(cover uint8[n] (1/0/2), covered, undetermined,
        greedy_cost, greedy_cigars, greedy_nops[, nw_cigars, nw_nops]).  cap: entries per Greedy CIGAR row; nw_cap: entries per NW
        row (None: cap).  A pair whose Greedy row did not fit (greedy_nops > cap, or 255: the count saturates) has cover 2, is
        counted in `undetermined` and has None for its greedy_cigars entry; an NW row that did not fit has None in nw_cigars."""
        n = batch.n
        nw_cap = cap if nw_cap is None else int(nw_cap)
        d_pen, d_ops, d_nops = self.malloc(4 * max(n, 1)), self.malloc(2 * cap * max(n, 1)), self.malloc(max(n, 1))
        d_cov, d_cnt = self.malloc(max(n, 1)), self.malloc(16)
        d_nwo = self.malloc(2 * nw_cap * max(n, 1)) if want_nw_cigars else None
        d_nwn = self.malloc(max(n, 1)) if want_nw_cigars else None
        try:
            self._chk(self.lib.asm_greedy_cigar_batch_async(self.h, batch.ptr, ctypes.byref(params), d_pen, d_ops, cap,
                                                            d_nops))
            self.memset_async(d_cnt, 0, 16)
            self._chk(self.lib.asm_coverage(self.h, batch.ptr, ctypes.byref(params), d_ops, cap, d_nops, window, d_cov,
                                            d_nwo, nw_cap, d_nwn, d_cnt))
            cnt = self.to_host(d_cnt, 2, np.uint64)
            out = {"cover": self.to_host(d_cov, n, np.uint8), "covered": int(cnt[0]), "undetermined": int(cnt[1]),
                   "greedy_cost": self.to_host(d_pen, n)}
            gops = self.to_host(d_ops, n * cap, np.uint16).reshape(n, cap)
            out["greedy_nops"] = self.to_host(d_nops, n, np.uint8)
            out["greedy_cigars"] = decode_cigars(gops, out["greedy_nops"], cap, truncated="none")
            if want_nw_cigars:
                out["nw_nops"] = self.to_host(d_nwn, n, np.uint8)
                out["nw_cigars"] = decode_cigars(self.to_host(d_nwo, n * nw_cap, np.uint16).reshape(n, nw_cap), out["nw_nops"], nw_cap,
                                                 reverse=True, truncated="none")
            return out
        finally:
            for p in (d_pen, d_ops, d_nops, d_cov, d_cnt, d_nwo, d_nwn):
                if p:
                    self.free(p)

    def count_equal_async(self, d_a: int, d_b: int, n: int, d_count: int) -> None:
        self._chk(self.lib.asm_count_equal_async(self.h, d_a, d_b, n, d_count))

    def accuracy_async(self, d_nw: int, d_leap: Optional[int], d_greedy: Optional[int], n: int, d_counters: int,
                       d_answers: Optional[int] = None) -> None:
        """counters (uint64[4]) += {total, nw_ok, leap_ok, greedy_ok} — benchmark_utils.h:249-255."""
        self._chk(self.lib.asm_accuracy_async(self.h, d_nw, d_leap, d_greedy, d_answers, n, d_counters))

    def run_benchmark_async(self, batch: DeviceBatch, params: Params, d_nw: Optional[int], d_leap: Optional[int],
                            d_greedy: Optional[int], d_counters: Optional[int], repack: bool = True,
                            d_answers: Optional[int] = None) -> None:
        """`_run_benchmark` over the whole resident batch (pack, NW, LEAP, Greedy, counters) in one call.  repack: False / True
        (pack in stream order) / 2 (pipelined: this call's pack overlaps the previous call's aligners) / 3 (overlapped calls:
        alternate two sets of output arrays from call to call and end with pipeline_join_async)."""
        self._chk(self.lib.asm_run_benchmark_async(self.h, batch.ptr, ctypes.byref(params), int(repack), d_nw,
                                                   d_leap, d_greedy, d_answers, d_counters))

    def pipeline_join_async(self) -> None:
        """Orders everything the overlapped calls (repack=3) enqueued before what comes next on the handle's stream."""
        self._chk(self.lib.asm_pipeline_join_async(self.h))

    # ---- timing ----
    def profile_enable(self, max_calls: int, kernel_mask: int = 0xF) -> None:
        """The next max_calls run_benchmark_async calls time the selected kernels (bit 0 pack, 1 NW, 2 LEAP, 3 Greedy) with
        events on the launching streams."""
        self._chk(self.lib.asm_profile_enable(self.h, int(max_calls), int(kernel_mask)))

    def profile_read(self, cap_calls: int) -> np.ndarray:
        """-> float32[calls][4] = ms of (pack, nw, leap, greedy) per recorded call, -1 where not launched; synchronises."""
        ms = np.full((max(cap_calls, 1), 4), -1.0, np.float32)
        n = ctypes.c_int(0)
        self._chk(self.lib.asm_profile_read(self.h, ms.ctypes.data, int(cap_calls), ctypes.byref(n)))
        return ms[:min(n.value, cap_calls)]

    def timer(self) -> "Timer":
        return Timer(self)


CIGAR_NOPS_MAX = 255  # the pair aligners' row counts are bytes that saturate: 255 means "255 or more"


def cigar_rows_truncated(nops: np.ndarray, cap: int) -> np.ndarray:
    """bool per row: the row is not known to be whole — nops > cap (only cap entries are stored), or nops == 255 (saturated)."""
    nops = np.asarray(nops).astype(np.int64)
    return (nops > int(cap)) | (nops >= CIGAR_NOPS_MAX)


def decode_cigars(ops: np.ndarray, nops: np.ndarray, cap: int, reverse: bool = False, truncated: str = "raise"):
    """Encoded rows (count << 3 | op; op 0 'M', 1 'I', 2 'D', 3 '=', 4 'X') -> CIGAR strings.  A row that is not known to be whole
    (cigar_rows_truncated) is never handed back as if it were: truncated = "raise" (ValueError), "none" (None in its place), or
    "prefix" for a caller that reports the truncation itself (the mapper's CIGAR_TRUNCATED flag): the stored entries."""
    if truncated not in ("raise", "none", "prefix"):
        raise ValueError("truncated must be 'raise', 'none' or 'prefix'")
    letters = "MID=X???"
    cut = cigar_rows_truncated(nops, cap)
    if truncated == "raise" and cut.any():
        first = int(np.nonzero(cut)[0][0])
        raise ValueError(f"{int(cut.sum())} CIGAR rows are truncated (first: row {first} reports {int(nops[first])} entries, "
                         f"cap {cap}; 255 means 255 or more): give the call a larger cap")
    out = []
    for i in range(ops.shape[0]):
        if cut[i] and truncated == "none":
            out.append(None)
            continue
        row = ops[i, :min(int(nops[i]), cap)]
        if reverse:
            row = row[::-1]
        out.append("".join(f"{int(v) >> 3}{letters[int(v) & 7]}" for v in row))
    return out


def md_format(ops, read_on_strand, ref_window) -> str:
    """asm_md_format: the MD:Z tag of one record, on the host (no device).  ops: its CIGAR, as a string of M, I and D runs ("40M1D60M",
    as the map_* methods return it) or as an encoded row (count << 3 | op); read_on_strand: the read as the alignment sees it (the
    reverse complement for strand 1); ref_window: the reference bases [pos, end) of the record's sequence.  Both are upper-cased."""
    if isinstance(ops, (str, bytes)):
        import re

        text = ops.decode("ascii") if isinstance(ops, bytes) else ops
        runs = re.findall(r"(\d+)([MID])", text)
        if "".join(c + o for c, o in runs) != text:
            raise ValueError("a CIGAR of M, I and D runs is wanted")
        ops = [int(c) << 3 | "MID".index(o) for c, o in runs]
    row = np.ascontiguousarray(ops, np.uint16).reshape(-1)
    q, w = _as_bytes(read_on_strand), _as_bytes(ref_window)
    out = ctypes.create_string_buffer(12 * (len(w) + row.size + 2))  # a letter or a caret, and a number in front, per byte and run
    n = load_library().asm_md_format(row.ctypes.data if row.size else None, int(row.size), q, len(q), w, len(w), out, len(out))
    if n < 0:
        raise AsmError(n, load_library().asm_last_error(None).decode())
    return out.raw[:n].decode("ascii")


def bgzf_compress_host(data: bytes, eof: bool = True, level: int = BGZF_DEFLATE) -> bytes:
    """asm_bgzf_compress_host: Engine.bgzf_compress without a device, by the host build of the same encoder; the same bytes"""
    lib = load_library()
    data = bytes(data)
    cap = int(lib.asm_bgzf_bound(len(data), int(eof)))
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    rc = lib.asm_bgzf_compress_host(data if data else None, len(data), int(eof), int(level), out, cap, ctypes.byref(got))
    if rc != 0:
        raise AsmError(rc, lib.asm_last_error(None).decode())
    return out.raw[: got.value]


class Timer:
    """HIP events on the engine's stream."""

    def __init__(self, engine: Engine):
        self.e = engine
        self.t = ctypes.c_void_p()
        engine._chk(engine.lib.asm_timer_create(engine.h, ctypes.byref(self.t)))

    def start(self) -> None:
        self.e._chk(self.e.lib.asm_timer_start(self.e.h, self.t))

    def stop(self) -> None:
        self.e._chk(self.e.lib.asm_timer_stop(self.e.h, self.t))

    def elapsed_ms(self) -> float:
        ms = ctypes.c_float()
        self.e._chk(self.e.lib.asm_timer_elapsed_ms(self.e.h, self.t, ctypes.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            self.e.lib.asm_timer_destroy(self.e.h, self.t)
        except Exception:
            pass


def declared_symbols() -> Sequence[str]:
    """Function names declared in include/asm_mi355x.h (parsed from the header text)."""
    import re

    with open(HEADER_PATH) as fh:
        text = fh.read()
    return sorted(set(re.findall(r"\b(asm_[a-z0-9_]+)\s*\(", text)) - {"asm_handle", "asm_batch"})


# ---- multi-GPU: read pairs are independent, so the batch shards with no data-path collective ----
def shard_bounds(total: int, world: int, rank: int) -> Tuple[int, int]:
    """Strong-scaling split of `total` pairs into contiguous blocks of ceil(total/world): -> [lo, hi)."""
    per = (total + world - 1) // world
    lo = min(rank * per, total)
    return lo, min(lo + per, total)


def weak_shard_first(rank: int, pairs_per_rank: int) -> int:
    """Weak scaling: rank r owns pairs [r*n, (r+1)*n) of the seeded stream."""
    return rank * pairs_per_rank


def tail_state_advance(state: np.ndarray, summary: np.ndarray, n_pairs: int) -> np.ndarray:
    """asm_tail_state_advance (host only, needs no GPU): buffer state after a batch of n_pairs with the given summary."""
    lib = load_library()
    st = np.ascontiguousarray(state, np.uint8).copy()
    sm = np.ascontiguousarray(summary, np.uint8)
    rc = lib.asm_tail_state_advance(st.ctypes.data, sm.ctypes.data, int(n_pairs))
    if rc:
        raise AsmError(rc, lib.asm_last_error(None).decode())
    return st


def chain_tail_state(summary: np.ndarray, n_pairs: int, dist=None, device=None) -> np.ndarray:
    """The buffer state before THIS rank's shard of a file whose shards are laid out in rank order: one all-gather of every
    shard's 256-byte summary and size (the only exchange sequential mode needs), then a local fold over the shards before
    ours.  Rank 0, or no process group: zeros — a file's start (hurdle_matrix.h:136-137)."""
    state = np.zeros(256, np.uint8)
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return state
    import torch

    mine = torch.zeros(264, dtype=torch.uint8, device=device)
    mine[:256] = torch.from_numpy(np.ascontiguousarray(summary, np.uint8)).to(mine.device)
    mine[256:] = torch.from_numpy(np.frombuffer(np.int64(n_pairs).tobytes(), np.uint8).copy()).to(mine.device)
    parts = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, mine)
    for r in range(dist.get_rank()):
        row = parts[r].cpu().numpy()
        state = tail_state_advance(state, row[:256], int(np.frombuffer(row[256:].tobytes(), np.int64)[0]))
    return state


def allreduce_counters(counters, dist=None):
    """The one collective of the path: sum the {total, nw_ok, leap_ok, greedy_ok} int64 counters over ranks
    (RCCL over xGMI on GPUs — backend "nccl"; gloo in the CPU tests).  `counters` is a torch tensor."""
    if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(counters)
    return counters


def gather_penalties(local, dist=None, dst: int = 0):
    """Optional: collect the per-shard penalty tensors on rank `dst` (each peer sends over its own direct link; shards
    may differ in length by one pair).  Returns the list of shards on `dst`, None elsewhere."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return [local]
    import torch

    world = dist.get_world_size()
    sizes = [torch.zeros(1, dtype=torch.int64, device=local.device) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([local.numel()], dtype=torch.int64, device=local.device))
    longest = max(int(s.item()) for s in sizes)
    padded = torch.zeros(longest, dtype=local.dtype, device=local.device)
    padded[:local.numel()] = local
    bufs = [torch.empty(longest, dtype=local.dtype, device=local.device) for _ in range(world)] \
        if dist.get_rank() == dst else None
    dist.gather(padded, bufs, dst=dst)
    if dist.get_rank() != dst:
        return None
    return [b[:int(s.item())] for b, s in zip(bufs, sizes)]


def bgzf_decompressed_size(data: bytes) -> int:
    """asm_bgzf_decompressed_size: the bytes a BGZF container decodes to, from its members' headers and trailers; nothing is decoded"""
    lib = load_library()
    data = bytes(data)
    got = ctypes.c_size_t(0)
    rc = lib.asm_bgzf_decompressed_size(data if data else None, len(data), ctypes.byref(got))
    if rc != 0:
        raise AsmError(rc, lib.asm_last_error(None).decode())
    return int(got.value)


def bam_index_host(data: bytes) -> bytes:
    """asm_bam_index_host: the BAI index of a whole coordinate-sorted BAM file, by the host build of the core the device index is
    made of (docs/design/mapper.md, "BAM index"); no device"""
    lib = load_library()
    data = bytes(data)
    cap, got = 1 << 16, ctypes.c_size_t(0)
    for _ in range(2):
        out = ctypes.create_string_buffer(cap)
        rc = lib.asm_bam_index_host(data if data else None, len(data), out, cap, ctypes.byref(got))
        if rc == 0:
            return out.raw[: got.value]
        if got.value <= cap:
            break
        cap = got.value  # the size it needs
    raise AsmError(rc, lib.asm_last_error(None).decode())


def bgzf_decompress_host(data: bytes) -> bytes:
    """asm_bgzf_decompress_host: Engine.bgzf_decompress without a device, by the host build of the same decoder; the same bytes and
    the same errors"""
    lib = load_library()
    data = bytes(data)
    cap = bgzf_decompressed_size(data)
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    rc = lib.asm_bgzf_decompress_host(data if data else None, len(data), out, cap, ctypes.byref(got))
    if rc != 0:
        raise AsmError(rc, lib.asm_last_error(None).decode())
    return out.raw[: got.value]
