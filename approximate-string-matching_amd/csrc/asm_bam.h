// BAM records of the file calls under ASM_OUT_BAM (contract: docs/design/mapper.md, "BAM output"): the binary record of one output
// line, single-end or paired, in the shape of asm_sam.h.  bam_format<Sink> walks the fields of a record in order (SAM spec 4.2,
// little endian) and hands every piece to a sink:
//   BamSizeSink  adds the lengths                      (line_size_kernel<BamRecord, .>: one thread per record)
//   BamLaneSink  stores the bytes p = lane (mod 64)    (line_emit_kernel<BamRecord, .>: one wave per record, 64 contiguous bytes per store)
// so the size and the bytes cannot disagree.  What a record says is what sam_format's line says: the same own / lent rules, the same
// flag, MAPQ and tags in the same order; the loaders and the two kernels are asm_sam.h's, which take the record as their format tag
// (BamRecord; line_kernels picks the pair to launch).  bam_header_bytes builds what the file's record stream starts with.  The part
// above the kernels holds no HIP: host/bam_host_check.cpp compiles it with plain g++ under ASan + UBSan and runs the lane sink for
// lanes 0..63 in turn (tests/test_bam_host.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "asm_sam.h"

#define BAM_NAME_MAX 254u /* l_read_name is one byte and counts the NUL */

/* how a piece's output bytes come out of its n source bytes */
enum { BAM_COPY = 0, BAM_QUAL = 1, BAM_QUAL_REV = 2, BAM_SEQ = 3, BAM_SEQ_REV = 4, BAM_NO_QUAL = 5 };

/* the 4-bit code of a SEQ character as the SAM line shows it, over "=ACMGRSVTWYHKDBN"; a byte outside it is N */
SAM_HD uint32_t bam_base_code(char c) {
    if (c == 'A') return 1u;
    if (c == 'C') return 2u;
    if (c == 'G') return 4u;
    if (c == 'T') return 8u;
    if (c == 'N') return 15u;
    for (uint32_t k = 0; k < 15u; k++)
        if ("=ACMGRSVTWYHKDB"[k] == c) return k;
    return 15u;
}
SAM_HD uint32_t bam_out_len(uint32_t n, int mode) { return (mode == BAM_SEQ || mode == BAM_SEQ_REV) ? (n + 1u) / 2u : n; }
/* output byte idx of a piece; SEQ packs the SAM line's characters 2 idx and 2 idx + 1, the first in the high nibble */
SAM_HD char bam_src_byte(const char* s, uint32_t n, uint32_t idx, int mode) {
    if (mode == BAM_COPY) return s[idx];
    if (mode == BAM_QUAL) return (char)(s[idx] - 33);
    if (mode == BAM_QUAL_REV) return (char)(s[n - 1u - idx] - 33);
    if (mode == BAM_NO_QUAL) return (char)0xff;
    const int text = mode == BAM_SEQ_REV ? SAM_REVCOMP : SAM_UPPER;
    const uint32_t hi = bam_base_code(sam_src_byte(s, n, 2u * idx, text));
    const uint32_t lo = 2u * idx + 1u < n ? bam_base_code(sam_src_byte(s, n, 2u * idx + 1u, text)) : 0u;
    return (char)(hi << 4 | lo);
}

struct BamSizeSink {
    uint64_t cur = 0;
    SAM_HD void le(uint32_t, uint32_t n) { cur += n; }
    SAM_HD void bytes(const char*, uint32_t n, int mode) { cur += bam_out_len(n, mode); }
};

/* lane `lane` of SAM_LANES stores the bytes at positions p with p % SAM_LANES == lane, counted from the record's first byte */
struct BamLaneSink {
    char* out;
    uint32_t lane;
    uint64_t cur = 0;
    SAM_HD uint32_t first() const { return (lane - (uint32_t)cur) & (SAM_LANES - 1u); }
    SAM_HD void le(uint32_t v, uint32_t n) { /* the low n <= 4 bytes of v, lowest first */
        const uint32_t idx = first();
        if (idx < n) out[cur + idx] = (char)(v >> (8u * idx));
        cur += n;
    }
    SAM_HD void bytes(const char* s, uint32_t n, int mode) {
        const uint32_t m = bam_out_len(n, mode);
        for (uint32_t idx = first(); idx < m; idx += SAM_LANES) out[cur + idx] = bam_src_byte(s, n, idx, mode);
        cur += m;
    }
};

/* reg2bin of SAM spec 5.3 over [beg, end); beg = -1, end = 0 (an unplaced record) gives 4680 */
SAM_HD uint32_t bam_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0u;
}

/* an integer tag in htslib's smallest type: C up to 255, S, I; negative: c, s, i */
template <class Sink>
SAM_HD void bam_tag_int(Sink& o, char a, char b, int32_t v) {
    const uint32_t n = v >= 0 ? (v <= 255 ? 1u : v <= 65535 ? 2u : 4u) : (v >= -128 ? 1u : v >= -32768 ? 2u : 4u);
    const char type = v >= 0 ? (n == 1u ? 'C' : n == 2u ? 'S' : 'I') : (n == 1u ? 'c' : n == 2u ? 's' : 'i');
    o.le((uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)type << 16, 3u);
    o.le((uint32_t)v, n);
}

/* everything behind block_size: refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen read_name cigar seq
 * qual [NM XG [MD]] [XP] [XR] [NH HI XH], each as the column of sam_format's line says */
template <class Sink>
SAM_HD void bam_fields(const SamLine& l, Sink& o) {
    const SamRec& r = l.rec;
    const bool pair = l.paired != 0, own = l.mapped != 0, lent = pair && !own && l.mate_mapped;
    const uint32_t name_len = pair ? sam_pair_name_len(l.raw, r) : r.name_len;
    const uint32_t flag = pair ? 1u | (l.proper ? 2u : 0u) | (own ? 0u : 4u) | (l.mate_mapped ? 0u : 8u) | (own && l.strand ? 16u : 0u) |
                                     (l.mate_mapped && l.mate_strand ? 32u : 0u) | (l.mate ? 128u : 64u)
                               : own ? (l.strand ? 16u : 0u) | (l.rank ? 256u : 0u) : 4u;
    const uint32_t pos_x = own ? l.pos + 1u : lent ? l.mate_pos + 1u : 0u;
    const uint32_t pos_y = !pair ? 0u : l.mate_mapped ? l.mate_pos + 1u : own ? l.pos + 1u : 0u;
    const int32_t ref_id = own ? l.seq_id : lent ? l.mate_seq_id : -1;
    const int32_t next_id = pair && l.mate_mapped ? l.mate_seq_id : -1; /* '=' resolves to the RNAME column's tid, which is the mate's */
    const uint32_t n_cigar = own && l.nops <= (uint32_t)SAM_CIGAR_CAP ? l.nops : 0u;
    uint32_t ref_len = 0;
    for (uint32_t i = 0; i < n_cigar; i++)
        if ((l.ops[i] & 7) != 1) ref_len += (uint32_t)(l.ops[i] >> 3); /* M, D, = and X consume the reference */
    const int64_t pos = (int64_t)pos_x - 1;
    const uint32_t bin = bam_reg2bin(pos, n_cigar ? pos + (int64_t)ref_len : pos + 1);
    const bool reverse = own && l.strand;
    const uint32_t l_seq = own && l.rank ? 0u : r.seq_len;
    const bool minus = pair && l.tlen != 0 && !(l.mate ? pos_x < pos_y : pos_x <= pos_y);
    o.le((uint32_t)ref_id, 4u);
    o.le(pos_x - 1u, 4u);
    o.le((name_len + 1u) | (own ? (uint32_t)l.mapq & 0xffu : 0u) << 8 | bin << 16, 4u);
    o.le(n_cigar | flag << 16, 4u);
    o.le(l_seq, 4u);
    o.le((uint32_t)next_id, 4u);
    o.le(pos_y - 1u, 4u);
    o.le(!pair ? 0u : minus ? 0u - l.tlen : l.tlen, 4u);
    o.bytes(l.raw + r.name, name_len, BAM_COPY);
    o.le(0u, 1u);
    for (uint32_t i = 0; i < n_cigar; i++) {
        const uint32_t op = l.ops[i] & 7u; /* M I D = X of the rows -> 0 1 2 7 8 */
        o.le((uint32_t)(l.ops[i] >> 3) << 4 | (op < 3u ? op : op + 4u), 4u);
    }
    if (l_seq) {
        o.bytes(l.raw + r.seq, l_seq, reverse ? BAM_SEQ_REV : BAM_SEQ);
        if (r.qual_len == l_seq) o.bytes(l.raw + r.qual, l_seq, reverse ? BAM_QUAL_REV : BAM_QUAL);
        else o.bytes(l.raw, l_seq, BAM_NO_QUAL);
    }
    if (own) {
        bam_tag_int(o, 'N', 'M', l.dist);
        bam_tag_int(o, 'X', 'G', l.greedy_cost);
        if (l.md_len) {
            o.le((uint32_t)'M' | (uint32_t)'D' << 8 | (uint32_t)'Z' << 16, 3u);
            o.bytes(l.md, l.md_len, BAM_COPY);
            o.le(0u, 1u);
        }
    }
    if (pair && l.proper) bam_tag_int(o, 'X', 'P', (int32_t)l.n_concordant);
    if (pair && l.rescued) bam_tag_int(o, 'X', 'R', 1);
    if (own && l.all) {
        bam_tag_int(o, 'N', 'H', (int32_t)l.n_reported);
        bam_tag_int(o, 'H', 'I', (int32_t)(l.rank + 1u));
        bam_tag_int(o, 'X', 'H', (int32_t)l.n_hits);
    }
}

/* block_size (the bytes behind it), then the fields */
template <class Sink>
SAM_HD void bam_format(const SamLine& l, Sink& o) {
    BamSizeSink body;
    bam_fields(l, body);
    o.le((uint32_t)body.cur, 4u);
    bam_fields(l, o);
}

SAM_HD uint64_t bam_record_size(const SamLine& l) {
    BamSizeSink s;
    bam_format(l, s);
    return s.cur;
}
SAM_HD void bam_record_emit(const SamLine& l, char* out, uint32_t lane) {
    BamLaneSink s{out, lane};
    bam_format(l, s);
}
/* the QNAME bam_format writes is too long for a record */
SAM_HD bool bam_name_too_long(const char* raw, const SamRec& r, bool pair) {
    return (pair ? sam_pair_name_len(raw, r) : r.name_len) > BAM_NAME_MAX;
}

/* The BAM header (SAM spec 4.2) as the record stream's first bytes, unframed: magic, l_text, the text, n_ref, and per reference
 * sequence l_name, the name with its NUL and l_ref.  text: l_text bytes, which may be NULL when l_text is 0. */
inline std::vector<uint8_t> bam_header_bytes(const char* text, size_t l_text, const char* const* names, const uint32_t* lengths, size_t n_ref) {
    std::vector<uint8_t> out = {'B', 'A', 'M', 1};
    const auto u32 = [&out](uint64_t v) {
        for (int b = 0; b < 4; b++) out.push_back((uint8_t)(v >> (8 * b)));
    };
    u32(l_text);
    if (l_text) out.insert(out.end(), text, text + l_text);
    u32(n_ref);
    for (size_t r = 0; r < n_ref; r++) {
        const size_t l_name = strlen(names[r]) + 1;
        u32(l_name);
        out.insert(out.end(), names[r], names[r] + l_name);
        u32(lengths[r]);
    }
    return out;
}

#if defined(__HIPCC__)

struct BamRecord { /* the format tag of asm_sam.h's line_size_kernel and line_emit_kernel */
    SAM_HD static uint64_t size(const SamLine& l) { return bam_record_size(l); }
    SAM_HD static void emit(const SamLine& l, char* out, uint32_t lane) { bam_record_emit(l, out, lane); }
};

/* The size and the emit kernel of a file call's output lines, by format and call: the one place that tests the format for a launch */
struct LineKernels {
    void (*size)(SamArgs);
    void (*emit)(SamArgs);
};
template <bool PAIRED>
static LineKernels line_kernels(bool bam) {
    if (bam) return {line_size_kernel<BamRecord, PAIRED>, line_emit_kernel<BamRecord, PAIRED>};
    return {line_size_kernel<SamText, PAIRED>, line_emit_kernel<SamText, PAIRED>};
}

/* Records [0, n) of a device chunk (PAIRED: [2][n], mate 1 of every pair and then mate 2): min_long[f] = the smallest record of file f
 * whose QNAME no BAM record can hold, FASTQ_NO_RECORD-style 0xffffffff when there is none */
template <bool PAIRED>
__global__ __launch_bounds__(256) void bam_name_check_kernel(const char* __restrict__ raw, const SamRec* __restrict__ recs, long n,
                                                             uint32_t* __restrict__ min_long) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (PAIRED ? 2 * n : n)) return;
    if (bam_name_too_long(raw, recs[i], PAIRED)) atomicMin(&min_long[i >= n ? 1 : 0], (uint32_t)(i >= n ? i - n : i));
}
#endif /* __HIPCC__ */
