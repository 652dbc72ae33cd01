// The BAI index beside a sorted BAM file (contract and canonical form: docs/design/mapper.md, "BAM index"; SAM spec 5.2).  The sorted
// BAM calls build it on the device from what SamSortHold::flush leaves there (the records' sources and stream offsets in output order)
// and from the compressed sizes of the record stream's blocks, which BgzfStream keeps while it frames them (asm_bgzf.h).
//
// The first part holds no HIP: the record-field reader, the virtual-offset rule, the layout arithmetic of a reference's section, the
// byte emitters, and bai_build_host, a serial walk over the same functions that asm_bam_index_host and host/bai_host_check.cpp run
// (plain g++ under ASan + UBSan, tests/test_bai_host.py).  The kernels and bai_index_device follow; asm_capi.hip includes this file
// inside its extern "C" block, between asm_sam_sort.h and asm_map_file.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "asm_bam.h"       /* bam_reg2bin */
#include "asm_bgzf_walk.h" /* InfMember */

extern "C++" {

#define BAI_MAX_COORD (1u << 29)  /* BAI holds coordinates below it; an end may equal it */
#define BAI_PSEUDO_BIN 37450u
#define BAI_WINDOW_SHIFT 14       /* the linear index's windows of 16 kbp */
#define BAI_NONE 0xffffffffffffffffull /* a window no record touches; a key of an unplaced record */
#define BAI_PAYLOAD 65280u        /* BGZF_PAYLOAD: the record stream's cut */

/* ---- a record's fields, from its bytes at any alignment ---------------------------------------------------------------------------- */
template <class Src>
SAM_HD uint32_t bai_le16(Src p) {
    return (uint32_t)(uint8_t)p[0] | (uint32_t)(uint8_t)p[1] << 8;
}
template <class Src>
SAM_HD uint32_t bai_le32(Src p) {
    return bai_le16(p) | bai_le16(p + 2) << 16;
}
struct BaiRec {
    int32_t tid;      /* refID; placed: >= 0 */
    int32_t pos;
    uint32_t end;     /* pos + the reference bases of the CIGAR (M D N = X), pos + 1 with none; 0 when not placed */
    uint32_t bin;     /* the record's own bin field */
    uint32_t mapped;  /* flag bit 4 clear */
    uint32_t l_name, n_cigar;
};
/* rec points at block_size.  Reads rec[4, 36 + l_read_name + 4 n_cigar_op); the caller knows that the record holds them. */
template <class Src>
SAM_HD BaiRec bai_record_head(Src rec) {
    BaiRec r;
    r.tid = (int32_t)bai_le32(rec + 4), r.pos = (int32_t)bai_le32(rec + 8);
    r.l_name = (uint8_t)rec[12], r.bin = bai_le16(rec + 14), r.n_cigar = bai_le16(rec + 16);
    r.mapped = (bai_le16(rec + 18) & 4u) ? 0u : 1u;
    r.end = 0u;
    return r;
}
template <class Src>
SAM_HD BaiRec bai_record(Src rec) {
    BaiRec r = bai_record_head(rec);
    if (r.tid < 0) return r;
    uint32_t ref_len = 0u;
    Src c = rec + 36 + r.l_name;
    for (uint32_t i = 0; i < r.n_cigar; i++) {
        const uint32_t v = bai_le32(c + 4u * i), op = v & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ref_len += v >> 4;
    }
    r.end = (uint32_t)r.pos + (ref_len ? ref_len : 1u);
    return r;
}
/* the sort key of a placed record's run: the reference above the bin */
SAM_HD uint64_t bai_key(int32_t tid, uint32_t bin) { return tid < 0 ? BAI_NONE : (uint64_t)(uint32_t)tid << 16 | bin; }
SAM_HD uint32_t bai_first_window(uint32_t beg) { return beg >> BAI_WINDOW_SHIFT; }
SAM_HD uint32_t bai_last_window(uint32_t end) { return (end - 1u) >> BAI_WINDOW_SHIFT; }
/* the windows a sequence of len bases can have */
SAM_HD uint32_t bai_windows(uint64_t len) { return (uint32_t)((len + (1u << BAI_WINDOW_SHIFT) - 1u) >> BAI_WINDOW_SHIFT); }

/* The virtual offset of stream offset u, counted from the first record, which starts a fresh block: coff[b] is the file offset of the
 * record stream's block b, coff[number of blocks] that of the EOF block.  An in-block offset never equals the payload. */
SAM_HD uint64_t bai_voffset(const unsigned long long* coff, uint64_t head_bytes, uint64_t u) {
    return (head_bytes + coff[u / BAI_PAYLOAD]) << 16 | u % BAI_PAYLOAD;
}

/* ---- the layout of the file: 8 bytes (magic, n_ref), a section per reference, n_no_coor ------------------------------------------- */
/* a reference's section: n_bin, its nb real bins (bin, n_chunk) with nc chunks in all, the pseudo-bin when it has records, n_intv and
 * the windows */
SAM_HD uint64_t bai_section_bytes(uint64_t nb, uint64_t nc, uint32_t has, uint64_t n_intv) {
    return 4u + 8u * nb + 16u * nc + (has ? 40u : 0u) + 4u + 8u * n_intv;
}
/* in a section that starts at sec: the chunk that is number chunk_in_ref of the reference's chunks and lies in the reference's real
 * bin number bin_in_ref (both from 0); its bin's header lies 8 bytes in front of the bin's first chunk */
SAM_HD uint64_t bai_chunk_at(uint64_t sec, uint64_t bin_in_ref, uint64_t chunk_in_ref) { return sec + 4u + 8u * (bin_in_ref + 1u) + 16u * chunk_in_ref; }
SAM_HD uint64_t bai_pseudo_at(uint64_t sec, uint64_t nb, uint64_t nc) { return sec + 4u + 8u * nb + 16u * nc; }
SAM_HD uint64_t bai_linear_at(uint64_t sec, uint64_t nb, uint64_t nc, uint32_t has) { return bai_pseudo_at(sec, nb, nc) + (has ? 40u : 0u); }

/* the emitters: every field lies at a multiple of 4 of an image that starts 8-byte aligned */
SAM_HD void bai_put32(uint8_t* img, uint64_t at, uint32_t v) { __builtin_memcpy(__builtin_assume_aligned(img + at, 4), &v, 4); }
SAM_HD void bai_put64(uint8_t* img, uint64_t at, uint64_t v) { bai_put32(img, at, (uint32_t)v), bai_put32(img, at + 4u, (uint32_t)(v >> 32)); }
SAM_HD void bai_emit_file_head(uint8_t* img, uint32_t n_ref) { bai_put32(img, 0, 0x01494142u /* BAI\1 */), bai_put32(img, 4, n_ref); }
SAM_HD void bai_emit_bin(uint8_t* img, uint64_t first_chunk_at, uint32_t bin, uint32_t n_chunk) {
    bai_put32(img, first_chunk_at - 8u, bin), bai_put32(img, first_chunk_at - 4u, n_chunk);
}
SAM_HD void bai_emit_chunk(uint8_t* img, uint64_t at, uint64_t beg, uint64_t end) { bai_put64(img, at, beg), bai_put64(img, at + 8u, end); }
/* n_bin in front of the section, and behind its real bins the pseudo-bin (has) and n_intv */
SAM_HD void bai_emit_section(uint8_t* img, uint64_t sec, uint64_t nb, uint64_t nc, uint32_t has, uint64_t v_first, uint64_t v_end,
                             uint64_t n_mapped, uint64_t n_unmapped, uint32_t n_intv) {
    bai_put32(img, sec, (uint32_t)nb + (has ? 1u : 0u));
    const uint64_t at = bai_pseudo_at(sec, nb, nc);
    if (has) {
        bai_emit_bin(img, at + 8u, BAI_PSEUDO_BIN, 2u);
        bai_emit_chunk(img, at + 8u, v_first, v_end);
        bai_emit_chunk(img, at + 24u, n_mapped, n_unmapped);
    }
    bai_put32(img, bai_linear_at(sec, nb, nc, has), n_intv);
}
SAM_HD void bai_emit_window(uint8_t* img, uint64_t sec, uint64_t nb, uint64_t nc, uint32_t has, uint32_t w, uint64_t v) {
    bai_put64(img, bai_linear_at(sec, nb, nc, has) + 4u + 8u * w, v);
}

/* ---- the host build: a whole BAM file's uncompressed stream and its members -------------------------------------------------------- */
enum { BAI_OK = 0, BAI_E_MALFORMED = 1, BAI_E_ORDER = 2, BAI_E_COORD = 3 };
struct BaiHostResult {
    int status = BAI_OK;
    std::string what; /* the message behind the call's name */
    int64_t refs = 0, bins = 0, chunks = 0, intervals = 0, no_coor = 0;
};

/* The virtual offset of byte at of the uncompressed stream (total bytes, file of n bytes): the member that holds it; behind the last
 * byte, the first of the empty members at the file's end (the EOF block), or the file's end when there is none.  Calls come with
 * ascending at: *cursor goes along. */
inline uint64_t bai_voffset_members(const std::vector<InfMember>& m, size_t n, uint64_t at, size_t* cursor) {
    size_t k = *cursor;
    while (k < m.size() && m[k].out_off + m[k].isize <= at) k++;
    *cursor = k;
    if (k < m.size()) return (uint64_t)m[k].src_off << 16 | (at - m[k].out_off);
    size_t e = m.size();
    while (e > 0 && m[e - 1].isize == 0u) e--;
    return (uint64_t)(e < m.size() ? m[e].src_off : n) << 16;
}

/* stream[0, len): header and records of a coordinate-sorted BAM file; members: the file's cut (bgzf_walk); file_bytes: its length.
 * img: the index.  A serial walk: every record's fields, virtual offset, runs of equal (reference, bin), window minima and counts, the
 * runs sorted stably by (reference, bin), then the sections laid out and emitted by the functions above. */
inline BaiHostResult bai_build_host(const uint8_t* stream, size_t len, const std::vector<InfMember>& members, size_t file_bytes,
                                    std::vector<uint8_t>& img) {
    BaiHostResult res;
    const auto bad = [&res](int status, const std::string& what) {
        res.status = status, res.what = what;
        return res;
    };
    if (len < 12 || memcmp(stream, "BAM\1", 4) != 0) return bad(BAI_E_MALFORMED, "the stream does not start with the BAM magic");
    const uint64_t l_text = bai_le32(stream + 4);
    if (l_text > len - 12) return bad(BAI_E_MALFORMED, "the header text reaches past the end");
    size_t at = 8 + (size_t)l_text;
    const uint32_t n_ref = bai_le32(stream + at);
    at += 4;
    if (n_ref > 0x7fffffffu) return bad(BAI_E_MALFORMED, "n_ref is negative");
    for (uint32_t t = 0; t < n_ref; t++) {
        if (len - at < 4) return bad(BAI_E_MALFORMED, "the header's reference " + std::to_string(t) + " reaches past the end");
        const uint64_t l_name = bai_le32(stream + at);
        if (l_name > len - at - 4 || len - at - 4 - l_name < 4) return bad(BAI_E_MALFORMED, "the header's reference " + std::to_string(t) + " reaches past the end");
        at += 8 + (size_t)l_name;
    }
    struct Run {
        uint64_t key, beg, end;
    };
    struct Ref {
        uint64_t v_first = 0, v_end = 0, n_mapped = 0, n_unmapped = 0;
        uint32_t has = 0;
        std::vector<uint64_t> window;
    };
    std::vector<Run> runs;
    std::vector<Ref> refs(n_ref);
    size_t cursor = 0;
    uint64_t prev_tid = 0, prev_pos = 0, prev_key = BAI_NONE, no_coor = 0;
    for (int64_t r = 0; at < len; r++) {
        const std::string name = "record " + std::to_string(r);
        if (len - at < 36) return bad(BAI_E_MALFORMED, name + " reaches past the end");
        const uint64_t size = bai_le32(stream + at);
        if (size < 32 || size > len - at - 4) return bad(BAI_E_MALFORMED, name + " reaches past the end");
        const BaiRec head = bai_record_head(stream + at);
        if (head.tid < -1 || (head.tid >= 0 && (uint32_t)head.tid >= n_ref))
            return bad(BAI_E_MALFORMED, name + " has refID " + std::to_string(head.tid) + " (n_ref = " + std::to_string(n_ref) + ")");
        if (32 + (uint64_t)head.l_name + 4u * (uint64_t)head.n_cigar > size) return bad(BAI_E_MALFORMED, name + ": its CIGAR reaches past its end");
        if (head.tid >= 0 && head.pos < 0) return bad(BAI_E_MALFORMED, name + " has a refID and no position");
        const uint64_t tid = head.tid < 0 ? 0xffffffffull : (uint64_t)head.tid, pos = head.tid < 0 ? 0ull : (uint64_t)head.pos;
        if (r > 0 && (tid < prev_tid || (tid == prev_tid && pos < prev_pos)))
            return bad(BAI_E_ORDER, name + " lies below its predecessor: the file is not sorted by (refID, pos)");
        prev_tid = tid, prev_pos = pos;
        const uint64_t v = bai_voffset_members(members, file_bytes, at, &cursor);
        const size_t next = at + 4 + (size_t)size;
        size_t look = cursor;
        const uint64_t v_next = bai_voffset_members(members, file_bytes, next, &look);
        if (head.tid < 0) {
            no_coor++, prev_key = BAI_NONE, at = next;
            continue;
        }
        if ((uint32_t)head.pos > BAI_MAX_COORD) return bad(BAI_E_COORD, name + " lies above 2^29, which a .bai index cannot hold: such a reference needs a .csi index");
        uint64_t ref_len = 0;
        for (uint32_t i = 0; i < head.n_cigar; i++) {
            const uint32_t c = bai_le32(stream + at + 36 + head.l_name + 4u * i), op = c & 15u;
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ref_len += c >> 4;
        }
        if (pos + (ref_len ? ref_len : 1u) > BAI_MAX_COORD)
            return bad(BAI_E_COORD, name + " ends above 2^29, which a .bai index cannot hold: such a reference needs a .csi index");
        const BaiRec rec = bai_record(stream + at);
        if (rec.bin != bam_reg2bin(rec.pos, rec.end))
            return bad(BAI_E_MALFORMED, name + " has bin " + std::to_string(rec.bin) + ", reg2bin of its position and CIGAR is " +
                                            std::to_string(bam_reg2bin(rec.pos, rec.end)));
        Ref& ref = refs[(size_t)rec.tid];
        if (!ref.has) ref.has = 1u, ref.v_first = v;
        ref.v_end = v_next;
        (rec.mapped ? ref.n_mapped : ref.n_unmapped)++;
        const uint32_t w1 = bai_last_window(rec.end);
        if (ref.window.size() <= w1) ref.window.resize((size_t)w1 + 1, BAI_NONE);
        for (uint32_t w = bai_first_window((uint32_t)rec.pos); w <= w1; w++) ref.window[w] = std::min(ref.window[w], v);
        const uint64_t key = bai_key(rec.tid, rec.bin);
        if (key != prev_key) runs.push_back({key, v, v_next});
        else runs.back().end = v_next;
        prev_key = key, at = next;
    }
    std::stable_sort(runs.begin(), runs.end(), [](const Run& a, const Run& b) { return a.key < b.key; });
    /* the sections' sizes, then the bytes */
    std::vector<uint64_t> nb(n_ref, 0), nc(n_ref, 0), sec(n_ref + (size_t)1, 8);
    for (size_t j = 0; j < runs.size(); j++) {
        const size_t t = (size_t)(runs[j].key >> 16);
        nc[t]++;
        if (j == 0 || runs[j].key != runs[j - 1].key) nb[t]++, res.bins++;
    }
    for (uint32_t t = 0; t < n_ref; t++) {
        for (size_t w = refs[t].window.size(); w-- > 0;) /* an untouched window takes the next higher touched one's value */
            if (refs[t].window[w] == BAI_NONE) refs[t].window[w] = refs[t].window[w + 1];
        sec[t + 1] = sec[t] + bai_section_bytes(nb[t], nc[t], refs[t].has, refs[t].window.size());
        res.intervals += (int64_t)refs[t].window.size();
    }
    img.assign((size_t)sec[n_ref] + 8, 0);
    std::vector<uint64_t> aligned(img.size() / 8 + 1); /* the emitters store whole dwords */
    uint8_t* const out = (uint8_t*)aligned.data();
    bai_emit_file_head(out, n_ref);
    size_t j = 0;
    for (uint32_t t = 0; t < n_ref; t++) {
        const Ref& ref = refs[t];
        bai_emit_section(out, sec[t], nb[t], nc[t], ref.has, ref.v_first, ref.v_end, ref.n_mapped, ref.n_unmapped, (uint32_t)ref.window.size());
        for (size_t w = 0; w < ref.window.size(); w++) bai_emit_window(out, sec[t], nb[t], nc[t], ref.has, (uint32_t)w, ref.window[w]);
        uint64_t bin_in_ref = 0;
        for (const size_t j0 = j; j < j0 + nc[t]; bin_in_ref++) {
            size_t j1 = j;
            while (j1 < j0 + nc[t] && runs[j1].key == runs[j].key) j1++;
            bai_emit_bin(out, bai_chunk_at(sec[t], bin_in_ref, j - j0), (uint32_t)(runs[j].key & 0xffffu), (uint32_t)(j1 - j));
            for (; j < j1; j++) bai_emit_chunk(out, bai_chunk_at(sec[t], bin_in_ref, j - j0), runs[j].beg, runs[j].end);
        }
    }
    bai_put64(out, sec[n_ref], no_coor);
    memcpy(img.data(), out, img.size());
    res.refs = n_ref, res.chunks = (int64_t)runs.size(), res.no_coor = (int64_t)no_coor;
    return res;
}
/* the index of an empty record stream: no device work */
inline std::vector<uint8_t> bai_empty_image(uint32_t n_ref) {
    std::vector<uint64_t> aligned(((size_t)8 * n_ref + 16) / 8 + 1, 0);
    bai_emit_file_head((uint8_t*)aligned.data(), n_ref);
    const uint8_t* p = (const uint8_t*)aligned.data();
    return std::vector<uint8_t>(p, p + (size_t)8 * n_ref + 16);
}

#if defined(__HIPCC__)

typedef unsigned long long bai_u64;

/* What the record pass leaves per record i < n in output order, and for i = n the stream's end */
struct BaiRecTables {
    bai_u64* key;     /* [n] bai_key: reference above bin, BAI_NONE when not placed */
    bai_u64* v;       /* [n + 1] the virtual offset of the record's first byte; [n]: of the byte behind the last record */
    uint32_t* beg;    /* [n] */
    uint32_t* end;    /* [n] */
    uint32_t* mapped; /* [n + 1] 1: placed and flag bit 4 clear; [n] = 0 */
    uint32_t* head;   /* [n + 1] 1: a placed record that starts a run of equal keys; [n] = 0 */
};
/* per reference t < n_ref */
struct BaiRefTables {
    const uint32_t* win_base; /* [n_ref + 1] the exclusive sum of bai_windows(length) */
    bai_u64* window;          /* [win_base[n_ref]] the smallest v per window, BAI_NONE first */
    uint32_t* rec_first;      /* [n_ref + 1] the reference's first and last record; [n_ref]: the first record that is not placed */
    uint32_t* rec_last;
    uint32_t* run_first;      /* its first and last run in the sorted runs, its first and last real bin among all bins */
    uint32_t* run_last;
    uint32_t* bin_first;
    uint32_t* bin_last;
    uint32_t* n_intv;
    bai_u64* sec_size;        /* [n_ref + 1] bai_section_bytes; [n_ref] = 0 */
};
#define BAI_NO_RECORD 0xffffffffu

/* one thread per record, and one for the stream's end: the fields from the held bytes (byte loads: a body lies at any alignment) */
__global__ __launch_bounds__(256) void bai_record_kernel(const bai_u64* __restrict__ psrc, const bai_u64* __restrict__ off, bai_u64 n,
                                                         const bai_u64* __restrict__ coff, bai_u64 head_bytes, BaiRecTables t) {
    const bai_u64 i = (bai_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    t.v[i] = bai_voffset(coff, head_bytes, off[i]);
    if (i == n) {
        t.mapped[n] = 0u;
        return;
    }
    const BaiRec r = bai_record((SamGlobalSrc)(uintptr_t)psrc[i]);
    t.key[i] = bai_key(r.tid, r.bin);
    t.beg[i] = (uint32_t)r.pos, t.end[i] = r.end;
    t.mapped[i] = r.tid >= 0 ? r.mapped : 0u;
}

/* one thread per record and one behind them: the heads of the runs, the first and last record of every reference, and the window
 * minima.  A record leaves a window to its predecessor when that one reaches it too (it lies in front and so has the smaller offset),
 * so few atomics meet; a 64-bit minimum does not depend on the order. */
__global__ __launch_bounds__(256) void bai_mark_kernel(bai_u64 n, uint32_t n_ref, BaiRecTables t, BaiRefTables f) {
    const bai_u64 i = (bai_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const bai_u64 key = i < n ? t.key[i] : BAI_NONE, prev = i > 0 ? t.key[i - 1] : BAI_NONE;
    const bool placed = key != BAI_NONE, prev_placed = prev != BAI_NONE;
    const uint32_t tid = (uint32_t)(key >> 16), prev_tid = (uint32_t)(prev >> 16);
    t.head[i] = placed && (i == 0 || key != prev) ? 1u : 0u;
    if (placed && (!prev_placed || prev_tid != tid) && tid < n_ref) f.rec_first[tid] = (uint32_t)i;
    if (prev_placed && (!placed || prev_tid != tid) && prev_tid < n_ref) f.rec_last[prev_tid] = (uint32_t)(i - 1);
    if (!placed && (i == 0 || prev_placed)) f.rec_first[n_ref] = (uint32_t)i; /* i = n when every record is placed */
    if (!placed || tid >= n_ref) return;
    const uint32_t nwin = f.win_base[tid + 1] - f.win_base[tid];
    uint32_t w0 = bai_first_window(t.beg[i]);
    const uint32_t w1 = bai_last_window(t.end[i]);
    if (prev_placed && prev_tid == tid) {
        const uint32_t covered = bai_last_window(t.end[i - 1]) + 1u; /* the predecessor starts at or in front of beg */
        w0 = w0 > covered ? w0 : covered;
    }
    const bai_u64 v = t.v[i];
    for (uint32_t w = w0; w <= w1 && w < nwin; w++) atomicMin(&f.window[f.win_base[tid] + w], v);
}

/* one thread per record and one behind them, behind the exclusive sum rpos of head: run r's key and virtual offsets, r in file order */
__global__ __launch_bounds__(256) void bai_runs_kernel(bai_u64 n, BaiRecTables t, const uint32_t* __restrict__ rpos, bai_u64* __restrict__ run_key,
                                                       uint32_t* __restrict__ run_idx, bai_u64* __restrict__ run_beg, bai_u64* __restrict__ run_end) {
    const bai_u64 i = (bai_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const bool head = t.head[i] != 0u;
    const bool closes = i > 0 && t.key[i - 1] != BAI_NONE && (head || i == n || t.key[i] == BAI_NONE);
    const uint32_t r = rpos[i];
    if (closes) run_end[r - 1u] = t.v[i];
    if (head) run_key[r] = t.key[i], run_idx[r] = r, run_beg[r] = t.v[i];
}

/* one thread per sorted run j < nruns, and one behind them: the heads of the bins */
__global__ __launch_bounds__(256) void bai_bin_mark_kernel(const bai_u64* __restrict__ key, uint32_t nruns, uint32_t* __restrict__ bhead) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nruns) return;
    bhead[j] = j < nruns && (j == 0u || key[j] != key[j - 1u]) ? 1u : 0u;
}
/* ... behind the exclusive sum bpos of bhead: where every bin starts in the sorted runs (bin_start[number of bins] = nruns), and every
 * reference's first and last run and bin */
__global__ __launch_bounds__(256) void bai_bin_tables_kernel(const bai_u64* __restrict__ key, uint32_t nruns, uint32_t n_ref,
                                                             const uint32_t* __restrict__ bhead, const uint32_t* __restrict__ bpos,
                                                             uint32_t* __restrict__ bin_start, BaiRefTables f) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nruns) return;
    if (j == nruns || bhead[j]) bin_start[bpos[j]] = j;
    if (j == nruns) return;
    const uint32_t tid = (uint32_t)(key[j] >> 16);
    if (tid >= n_ref) return;
    const uint32_t bin = bpos[j] + bhead[j] - 1u; /* the bin of run j among all bins */
    if (j == 0u || (uint32_t)(key[j - 1u] >> 16) != tid) f.run_first[tid] = j, f.bin_first[tid] = bin;
    if (j + 1u == nruns || (uint32_t)(key[j + 1u] >> 16) != tid) f.run_last[tid] = j, f.bin_last[tid] = bin;
}

/* One wavefront per reference: the suffix pass of its windows from the top (an untouched window takes the next higher touched one's
 * value), n_intv = the highest touched window + 1, and the section's size. */
__global__ __launch_bounds__(64) void bai_windows_kernel(uint32_t n_ref, BaiRefTables f) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_ref) return;
    bai_u64* const win = f.window + f.win_base[t];
    const uint32_t nwin = f.win_base[t + 1u] - f.win_base[t];
    bai_u64 carry = BAI_NONE;
    uint32_t n_intv = 0u;
    for (uint32_t top = nwin; top > 0u; top = top > 64u ? top - 64u : 0u) { /* lane l: window top - 1 - l */
        const bool valid = lane < top;
        const bai_u64 x = valid ? win[top - 1u - lane] : BAI_NONE;
        const bai_u64 mask = __ballot(x != BAI_NONE);
        const bai_u64 upto = mask & (lane == 63u ? ~0ull : (2ull << lane) - 1ull); /* touched windows at or above this lane's */
        const int from = upto ? 63 - __builtin_clzll(upto) : (int)lane;
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, from), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), from);
        const bai_u64 y = upto ? ((bai_u64)hi << 32 | lo) : carry;
        if (valid) win[top - 1u - lane] = y; /* a touched window keeps its value; above the highest touched one BAI_NONE stays */
        if (mask != 0ull) {
            if (n_intv == 0u) n_intv = top - (uint32_t)__builtin_ctzll(mask);
            const int last = 63 - __builtin_clzll(mask);
            const uint32_t clo = (uint32_t)__shfl((int)(uint32_t)x, last), chi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), last);
            carry = (bai_u64)chi << 32 | clo;
        }
    }
    if (lane != 0u) return;
    const uint32_t has = f.rec_first[t] != BAI_NO_RECORD ? 1u : 0u;
    const uint32_t nb = f.run_first[t] != BAI_NO_RECORD ? f.bin_last[t] - f.bin_first[t] + 1u : 0u;
    const uint32_t nc = f.run_first[t] != BAI_NO_RECORD ? f.run_last[t] - f.run_first[t] + 1u : 0u;
    f.n_intv[t] = n_intv;
    f.sec_size[t] = bai_section_bytes(nb, nc, has, n_intv);
    if (t == 0u) f.sec_size[n_ref] = 0ull;
}

struct BaiEmitArgs {
    uint8_t* img;
    const bai_u64* sec_off;    /* [n_ref + 1] the exclusive sum of sec_size: a section starts at 8 + sec_off */
    const bai_u64* key;        /* the sorted runs */
    const uint32_t* idx;       /* sorted run -> run in file order */
    const bai_u64 *run_beg, *run_end;
    const uint32_t *bhead, *bpos, *bin_start;
    const uint32_t* cum_mapped; /* [n + 1] the exclusive sum of mapped */
    const bai_u64* v;
    uint32_t nruns, n_ref, nwin_all;
    bai_u64 n;
};
/* The image, one thread per item: sorted run j < nruns (its chunk, and its bin's header when it starts one); then reference t (n_bin,
 * pseudo-bin, n_intv); then window g of all references' windows (its reference by bisection); then one thread for magic, n_ref and
 * n_no_coor.  Every byte of the image has exactly one writer. */
__global__ __launch_bounds__(256) void bai_emit_kernel(BaiEmitArgs a, BaiRefTables f) {
    bai_u64 g = (bai_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < a.nruns) {
        const uint32_t j = (uint32_t)g, tid = (uint32_t)(a.key[j] >> 16);
        if (tid >= a.n_ref) return;
        const uint32_t bin = a.bpos[j] + a.bhead[j] - 1u;
        const bai_u64 at = bai_chunk_at(8u + a.sec_off[tid], bin - f.bin_first[tid], j - f.run_first[tid]);
        const uint32_t r = a.idx[j];
        bai_emit_chunk(a.img, at, a.run_beg[r], a.run_end[r]);
        if (a.bhead[j]) bai_emit_bin(a.img, at, (uint32_t)(a.key[j] & 0xffffu), a.bin_start[bin + 1u] - j);
        return;
    }
    g -= a.nruns;
    if (g < a.n_ref) {
        const uint32_t t = (uint32_t)g;
        const uint32_t has = f.rec_first[t] != BAI_NO_RECORD ? 1u : 0u;
        const uint32_t nb = f.run_first[t] != BAI_NO_RECORD ? f.bin_last[t] - f.bin_first[t] + 1u : 0u;
        const uint32_t nc = f.run_first[t] != BAI_NO_RECORD ? f.run_last[t] - f.run_first[t] + 1u : 0u;
        bai_u64 v_first = 0, v_end = 0, n_mapped = 0, n_unmapped = 0;
        if (has) {
            const uint32_t i0 = f.rec_first[t], i1 = f.rec_last[t] + 1u;
            v_first = a.v[i0], v_end = a.v[i1];
            n_mapped = a.cum_mapped[i1] - a.cum_mapped[i0], n_unmapped = (i1 - i0) - n_mapped;
        }
        bai_emit_section(a.img, 8u + a.sec_off[t], nb, nc, has, v_first, v_end, n_mapped, n_unmapped, f.n_intv[t]);
        return;
    }
    g -= a.n_ref;
    if (g < a.nwin_all) {
        uint32_t lo = 0u, hi = a.n_ref - 1u; /* the last reference with win_base <= g: references without windows share a base */
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (f.win_base[mid] <= g) lo = mid;
            else hi = mid - 1u;
        }
        const uint32_t t = lo, w = (uint32_t)g - f.win_base[t];
        if (w >= f.n_intv[t]) return;
        const uint32_t has = f.rec_first[t] != BAI_NO_RECORD ? 1u : 0u;
        const uint32_t nb = f.run_first[t] != BAI_NO_RECORD ? f.bin_last[t] - f.bin_first[t] + 1u : 0u;
        const uint32_t nc = f.run_first[t] != BAI_NO_RECORD ? f.run_last[t] - f.run_first[t] + 1u : 0u;
        bai_emit_window(a.img, 8u + a.sec_off[t], nb, nc, has, w, f.window[g]);
        return;
    }
    if (g == a.nwin_all) {
        bai_emit_file_head(a.img, a.n_ref);
        const uint32_t first_unplaced = f.rec_first[a.n_ref];
        bai_put64(a.img, 8u + a.sec_off[a.n_ref], a.n - (first_unplaced == BAI_NO_RECORD ? a.n : first_unplaced));
    }
}

/* hipcub's exclusive sum with a 64-bit count (n + 1 records may pass 2^31) */
template <class T>
static hipError_t bai_exclusive_sum(asm_handle* h, MapTmp& tmp, T* in, T* out, size_t n) {
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n, h->stream);
    if (e == hipSuccess) e = tmp.reserve(bytes);
    return e != hipSuccess ? e : hipcub::DeviceScan::ExclusiveSum(tmp.s.p, bytes, in, out, n, h->stream);
}

static int bai_write_failed(asm_handle* h, const char* who) { return fail(h, ASM_EINVAL, std::string(who) + ": writing the BAM index failed"); }
static int bai_write_file(asm_handle* h, const char* who, const std::string& path, const void* bytes, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return bai_write_failed(h, who);
    const bool ok = fwrite(bytes, 1, n, f) == n;
    return (fclose(f) == 0 && ok) ? (int)ASM_OK : bai_write_failed(h, who);
}

/* Behind MapOutput::finish of a sorted BAM call: the index of the file just written, to `path`.  s holds the records' sources and
 * stream offsets in output order (psrc, off) and the compressed sizes of the record stream's blocks (blk_size, which BgzfStream
 * filled); ref_len: the lengths of the index's n_ref sequences; head_bytes: the file's bytes in front of the record stream.  Every
 * table and the image are allocations of the hold.  Three waits: the number of runs, the image's size, the image. */
static int bai_index_device(SamSortHold& s, uint64_t head_bytes, const std::vector<uint32_t>& ref_len, const std::string& path) {
    asm_handle* h = s.h;
    const char* who = s.who;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n_ref = (uint32_t)ref_len.size();
    const size_t n = (size_t)s.st.lines;
    asm_bam_index_stats st = {};
    st.refs = n_ref;
    const auto done = [&](size_t bytes) {
        st.bytes = (int64_t)bytes;
        st.seconds_index = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        h->last_bai = st;
        return (int)ASM_OK;
    };
    if (n == 0 || n_ref == 0) { /* no placed record: two zero counts per sequence, and n_no_coor */
        std::vector<uint8_t> img = bai_empty_image(n_ref);
        const uint64_t no_coor = n;
        memcpy(img.data() + img.size() - 8, &no_coor, 8);
        st.no_coor = (int64_t)n;
        if (const int rc = bai_write_file(h, who, path, img.data(), img.size())) return rc;
        return done(img.size());
    }
    MapTmp tmp(h);
    /* the block table: coff = the exclusive sum of the blocks' compressed sizes */
    bai_u64* coff = nullptr;
    if (const int rc = s.alloc(&coff, sizeof(bai_u64) * (s.nblk + 1))) return rc;
    STREAM_TRY(who, bai_exclusive_sum(h, tmp, s.blk_size, coff, s.nblk + 1));
    /* the reference tables */
    std::vector<uint32_t> win_base(n_ref + (size_t)1, 0u);
    for (uint32_t t = 0; t < n_ref; t++) win_base[t + 1] = win_base[t] + bai_windows(ref_len[t]);
    const uint32_t nwin_all = win_base[n_ref];
    uint32_t *d_win_base = nullptr, *ref_u32 = nullptr;
    bai_u64 *window = nullptr, *sec_size = nullptr, *sec_off = nullptr;
    const size_t ref_cnt = (size_t)n_ref + 1;
    if (const int rc = s.alloc(&d_win_base, sizeof(uint32_t) * ref_cnt)) return rc;
    if (const int rc = s.alloc(&ref_u32, sizeof(uint32_t) * ref_cnt * 7)) return rc;
    if (const int rc = s.alloc(&window, sizeof(bai_u64) * ((size_t)nwin_all + 1))) return rc;
    if (const int rc = s.alloc(&sec_size, sizeof(bai_u64) * ref_cnt)) return rc;
    if (const int rc = s.alloc(&sec_off, sizeof(bai_u64) * ref_cnt)) return rc;
    BaiRefTables f = {d_win_base, window, ref_u32, ref_u32 + ref_cnt, ref_u32 + 2 * ref_cnt, ref_u32 + 3 * ref_cnt, ref_u32 + 4 * ref_cnt,
                      ref_u32 + 5 * ref_cnt, ref_u32 + 6 * ref_cnt, sec_size};
    STREAM_TRY(who, hipMemcpyAsync(d_win_base, win_base.data(), sizeof(uint32_t) * ref_cnt, hipMemcpyHostToDevice, h->stream));
    STREAM_TRY(who, hipMemsetAsync(ref_u32, 0xff, sizeof(uint32_t) * ref_cnt * 7, h->stream)); /* BAI_NO_RECORD */
    STREAM_TRY(who, hipMemsetAsync(window, 0xff, sizeof(bai_u64) * ((size_t)nwin_all + 1), h->stream)); /* BAI_NONE */
    /* the record pass, the marks, and the two scans over the records */
    BaiRecTables t = {};
    uint32_t *rpos = nullptr, *cum_mapped = nullptr;
    if (const int rc = s.alloc(&t.key, sizeof(bai_u64) * n)) return rc;
    if (const int rc = s.alloc(&t.v, sizeof(bai_u64) * (n + 1))) return rc;
    for (uint32_t** p : {&t.beg, &t.end, &t.mapped, &t.head, &rpos, &cum_mapped})
        if (const int rc = s.alloc(p, sizeof(uint32_t) * (n + 1))) return rc;
    const int grid = grid_for((int64_t)n + 1);
    STREAM_TRY(who, launch(h, bai_record_kernel, grid, ASM_BLOCK, (const bai_u64*)s.psrc, (const bai_u64*)s.off, (bai_u64)n, (const bai_u64*)coff,
                           (bai_u64)head_bytes, t));
    STREAM_TRY(who, launch(h, bai_mark_kernel, grid, ASM_BLOCK, (bai_u64)n, n_ref, t, f));
    STREAM_TRY(who, bai_exclusive_sum(h, tmp, t.head, rpos, n + 1));
    STREAM_TRY(who, bai_exclusive_sum(h, tmp, t.mapped, cum_mapped, n + 1));
    uint32_t nruns = 0;
    STREAM_TRY(who, fetch(h, {fetched(&nruns, (const uint32_t*)rpos + n)}));
    /* the runs: compacted in file order, sorted stably by (reference, bin), the bins' heads and the references' ends found */
    const size_t run_cnt = (size_t)nruns + 1;
    bai_u64 *run_key = nullptr, *run_key_s = nullptr, *run_beg = nullptr, *run_end = nullptr;
    uint32_t *run_idx = nullptr, *run_idx_s = nullptr, *bhead = nullptr, *bpos = nullptr, *bin_start = nullptr;
    for (bai_u64** p : {&run_key, &run_key_s, &run_beg, &run_end})
        if (const int rc = s.alloc(p, sizeof(bai_u64) * run_cnt)) return rc;
    for (uint32_t** p : {&run_idx, &run_idx_s, &bhead, &bpos, &bin_start})
        if (const int rc = s.alloc(p, sizeof(uint32_t) * run_cnt)) return rc;
    STREAM_TRY(who, launch(h, bai_runs_kernel, grid, ASM_BLOCK, (bai_u64)n, t, (const uint32_t*)rpos, run_key, run_idx, run_beg, run_end));
    if (nruns) {
        int tid_bits = 0;
        while (((uint64_t)n_ref >> tid_bits) != 0) tid_bits++;
        STREAM_TRY(who, map_sort_pairs(h, tmp, run_key, run_key_s, run_idx, run_idx_s, nruns, 16 + tid_bits));
    }
    const int run_grid = grid_for((int64_t)nruns + 1);
    STREAM_TRY(who, launch(h, bai_bin_mark_kernel, run_grid, ASM_BLOCK, (const bai_u64*)run_key_s, nruns, bhead));
    STREAM_TRY(who, bai_exclusive_sum(h, tmp, bhead, bpos, run_cnt));
    STREAM_TRY(who, launch(h, bai_bin_tables_kernel, run_grid, ASM_BLOCK, (const bai_u64*)run_key_s, nruns, n_ref, (const uint32_t*)bhead,
                           (const uint32_t*)bpos, bin_start, f));
    /* the windows' suffix pass and the sections' sizes, then where every section starts */
    STREAM_TRY(who, launch(h, bai_windows_kernel, n_ref, 64u, n_ref, f));
    STREAM_TRY(who, bai_exclusive_sum(h, tmp, sec_size, sec_off, ref_cnt));
    /* the image: its size is bounded by what the host knows, so it is allocated without a wait */
    uint64_t bound = 16;
    for (uint32_t r = 0; r < n_ref; r++) bound += bai_section_bytes(0, 0, 1u, win_base[r + 1] - win_base[r]);
    bound += (uint64_t)24 * nruns;
    uint8_t* img = nullptr;
    if (const int rc = s.alloc(&img, (size_t)bound + 8)) return rc;
    STREAM_TRY(who, hipMemsetAsync(img, 0, (size_t)bound + 8, h->stream));
    const BaiEmitArgs a = {img, sec_off, run_key_s, run_idx_s, run_beg, run_end, bhead, bpos, bin_start, cum_mapped, t.v, nruns, n_ref, nwin_all, (bai_u64)n};
    STREAM_TRY(who, launch(h, bai_emit_kernel, grid_for((int64_t)nruns + n_ref + nwin_all + 1), ASM_BLOCK, a, f));
    bai_u64 sections = 0;
    uint32_t nbins = 0;
    std::vector<uint32_t> n_intv(n_ref);
    STREAM_TRY(who, fetch(h, {fetched(&sections, (const bai_u64*)sec_off + n_ref), fetched(&nbins, (const uint32_t*)bpos + nruns),
                              fetched(n_intv.data(), (const uint32_t*)f.n_intv, n_ref)}));
    const size_t bytes = (size_t)sections + 16;
    if (bytes > bound + 8) return fail(h, ASM_EINVAL, std::string(who) + ": the BAM index is larger than its bound");
    std::vector<uint8_t> image(bytes);
    STREAM_TRY(who, hipMemcpyAsync(image.data(), img, bytes, hipMemcpyDeviceToHost, h->stream));
    STREAM_TRY(who, hipStreamSynchronize(h->stream));
    if (const int rc = bai_write_file(h, who, path, image.data(), bytes)) return rc;
    st.bins = nbins, st.chunks = nruns;
    for (uint32_t v : n_intv) st.intervals += v;
    memcpy(&st.no_coor, image.data() + bytes - 8, 8);
    return done(bytes);
}

#endif /* __HIPCC__ */

} /* extern "C++" */

#if defined(__HIPCC__)
static int bai_kind_check(asm_handle* h, int kind) {
    if (kind != ASM_BAM_INDEX_NONE && kind != ASM_BAM_INDEX_BAI)
        return fail(h, ASM_EINVAL, "asm_map_set_bam_index: kind must be ASM_BAM_INDEX_NONE (0) or ASM_BAM_INDEX_BAI (1)");
    return ASM_OK;
}
int asm_map_set_bam_index(asm_handle* h, int kind) {
    if (const int rc = bai_kind_check(h, kind)) return rc;
    if (!h) return fail(h, ASM_EINVAL, "asm_map_set_bam_index: NULL handle");
    h->bam_index = kind;
    return ASM_OK;
}
int asm_map_get_bam_index(const asm_handle* h) { return h ? h->bam_index : ASM_BAM_INDEX_NONE; }
int asm_map_last_bam_index(asm_handle* h, asm_bam_index_stats* out) {
    if (!h || !out) return fail(h, ASM_EINVAL, "asm_map_last_bam_index: NULL argument");
    *out = h->last_bai;
    return ASM_OK;
}
int asm_bam_index_host(const void* bam, size_t n, void* dst, size_t dst_cap, size_t* dst_len) {
    const std::string who = "asm_bam_index_host";
    if ((n && !bam) || !dst_len) return fail(nullptr, ASM_EINVAL, who + ": NULL argument");
    *dst_len = 0;
    std::vector<InfMember> members;
    size_t total = 0;
    const BgzfWalkError err = bgzf_walk((const uint8_t*)bam, n, &members, &total);
    if (err.status != BGZF_IN_OK) return bgzf_in_fail(nullptr, who, (const uint8_t*)bam, n, err);
    std::vector<uint8_t> stream(total);
    const unsigned long long bad_member = bgzf_inflate_host((const uint8_t*)bam, members, stream.data());
    if (bad_member != INF_NONE_BAD) return bgzf_member_fail(nullptr, who, members, bad_member);
    std::vector<uint8_t> img;
    const BaiHostResult r = bai_build_host(stream.data(), total, members, n, img);
    if (r.status != BAI_OK) return fail(nullptr, r.status == BAI_E_COORD ? ASM_EUNSUPPORTED : ASM_EINVAL, who + ": " + r.what);
    *dst_len = img.size();
    if (dst_cap < img.size() || !dst) return fail(nullptr, ASM_EINVAL, who + ": dst_cap is below the index's size (" + std::to_string(img.size()) + " bytes)");
    memcpy(dst, img.data(), img.size());
    return ASM_OK;
}
#endif /* __HIPCC__ */
