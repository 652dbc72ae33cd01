// SAM lines of asm_map_file and asm_map_pairs_file (contract: docs/design/mapper.md, "Files: FASTQ in, SAM out" and "Files: two
// FASTQ files in, paired SAM out"): the text of one output line, single-end or paired, written once for three users.  sam_format<Sink> walks the fields of a line in order and hands every piece to a sink:
//   SamSizeSink  adds the lengths                      (line_size_kernel<SamText, .>: one thread per line)
//   SamLaneSink  stores the bytes p = lane (mod 64)    (line_emit_kernel<SamText, .>: one wave per line, 64 contiguous bytes per store)
// so the size and the bytes cannot disagree.  The two kernels take the output format as a tag (SamText here, BamRecord in
// asm_bam.h, whose line_kernels picks the pair to launch).  The part above the kernels holds no HIP: host/sam_host_check.cpp
// compiles it with plain g++ under ASan + UBSan and runs the lane sink for lanes 0..63 in turn (tests/test_map_file_host.py,
// tests/test_map_pairs_file_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SAM_HD __host__ __device__ inline
#else
#define SAM_HD inline
#endif

#define SAM_LANES 64u
#define SAM_CIGAR_CAP 64 /* a row with more operations is written as '*' (asm-map's cigar_cap) */
#define SAM_NO_ITEM 0xffffffffu
#define SAM_LIT(o, s) (o).lit(s, (uint32_t)sizeof(s) - 1u) /* a string literal, shorter than SAM_LANES */

/* where a record's fields lie in the chunk's raw bytes (fastq_record_kernel) */
struct SamRec {
    uint32_t name, name_len; /* QNAME: the first word after '@' */
    uint32_t seq, seq_len;   /* without the line's CR */
    uint32_t qual, qual_len;
};

/* one output line */
struct SamLine {
    const char* raw; /* the chunk's bytes */
    SamRec rec;
    int mapped; /* 0: the unmapped line; the hit fields below are not read */
    int32_t seq_id;
    uint32_t pos;
    int32_t dist, greedy_cost;
    int32_t mapq; /* column 5 of a mapped line, by the call's MAPQ model (the loaders below; docs/design/mapper.md, "Mapping quality") */
    uint32_t strand, rank;
    const uint16_t* ops; /* count << 3 | op */
    uint32_t nops;
    const char* rname;
    uint32_t rname_len;
    int all; /* max_hits > 0: NH, HI and XH follow */
    uint32_t n_reported, n_hits;
    /* a record of a pair (asm_map_pairs_file); 0: a single-end line, and nothing below is read */
    int paired;
    uint32_t mate;                 /* 0: mate 1, 1: mate 2 */
    int proper, rescued;           /* the pair is proper; this record was rescued */
    int mate_mapped;               /* the other mate's record; the fields below are not read without it */
    int32_t mate_seq_id;
    uint32_t mate_pos, mate_strand;
    const char* mate_rname;
    uint32_t mate_rname_len;
    uint32_t tlen, n_concordant;   /* max(end) - min(pos) when both mates lie on one sequence, else 0 */
    /* the MD:Z tag of a mapped line (asm_md.h; asm_map_set_sam_tags); md_len 0: none, and md is not read */
    const char* md;
    uint32_t md_len;
};

enum { SAM_COPY = 0, SAM_UPPER = 1, SAM_REVCOMP = 2, SAM_REVERSE = 3 };

SAM_HD uint32_t sam_width(uint32_t v) { /* decimal digits of v */
    uint32_t w = 1;
    while (v >= 10u) v /= 10u, w++;
    return w;
}
SAM_HD char sam_digit(uint32_t v, uint32_t w, uint32_t idx) { /* character idx of v printed in w digits */
    for (uint32_t k = w - 1u - idx; k > 0; k--) v /= 10u;
    return (char)('0' + v % 10u);
}
SAM_HD char sam_upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
SAM_HD char sam_comp(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
SAM_HD char sam_src_byte(const char* s, uint32_t n, uint32_t idx, int mode) {
    return mode == SAM_COPY ? s[idx] : mode == SAM_UPPER ? sam_upper(s[idx]) : mode == SAM_REVERSE ? s[n - 1u - idx] : sam_comp(sam_upper(s[n - 1u - idx]));
}

/* bytes r .. r + 3 of the eight bytes lo, hi (little endian), r in [0, 3]: one v_alignbyte_b32 */
SAM_HD uint32_t sam_funnel(uint32_t hi, uint32_t lo, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * r));
#endif
}

struct SamSizeSink {
    uint64_t cur = 0;
    SAM_HD void ch(char) { cur++; }
    SAM_HD void lit(const char*, uint32_t n) { cur += n; }
    SAM_HD void num(uint32_t v) { cur += sam_width(v); }
    SAM_HD void bytes(const char*, uint32_t n, int) { cur += n; }
};

/* lane `lane` of SAM_LANES stores the bytes at positions p with p % SAM_LANES == lane, counted from the line's first byte */
struct SamLaneSink {
    char* out;
    uint32_t lane;
    uint64_t cur = 0;
    SAM_HD uint32_t first() const { return (lane - (uint32_t)cur) & (SAM_LANES - 1u); } /* this lane's first index into the next piece */
    SAM_HD void ch(char c) {
        if (first() == 0u) out[cur] = c;
        cur++;
    }
    SAM_HD void lit(const char* s, uint32_t n) { /* n < SAM_LANES */
        const uint32_t idx = first();
        if (idx < n) out[cur + idx] = s[idx];
        cur += n;
    }
    SAM_HD void num(uint32_t v) {
        const uint32_t w = sam_width(v), idx = first();
        if (idx < w) out[cur + idx] = sam_digit(v, w, idx);
        cur += w;
    }
    SAM_HD void bytes(const char* s, uint32_t n, int mode) {
        for (uint32_t idx = first(); idx < n; idx += SAM_LANES) out[cur + idx] = sam_src_byte(s, n, idx, mode);
        cur += n;
    }
};

template <class Sink>
SAM_HD void sam_int(Sink& o, int32_t v) {
    if (v < 0) o.ch('-');
    o.num(v < 0 ? 0u - (uint32_t)v : (uint32_t)v);
}

/* QNAME of a paired record: the first word without a trailing /1 or /2 (pair_name of host/asm_map.cpp) */
SAM_HD uint32_t sam_pair_name_len(const char* raw, const SamRec& r) {
    const uint32_t n = r.name_len;
    return (n >= 2u && raw[r.name + n - 2u] == '/' && (raw[r.name + n - 1u] == '1' || raw[r.name + n - 1u] == '2')) ? n - 2u : n;
}

/* QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL [NM XG [MD]] [XP] [XR] [NH HI XH]; a single-end line has RNEXT '*', PNEXT 0
 * and TLEN 0, a paired one borrows RNAME and POS from its mapped mate when it is unmapped itself (write_pairs of host/asm_map.cpp) */
template <class Sink>
SAM_HD void sam_format(const SamLine& l, Sink& o) {
    const SamRec& r = l.rec;
    const bool pair = l.paired != 0, own = l.mapped != 0, lent = pair && !own && l.mate_mapped;
    o.bytes(l.raw + r.name, pair ? sam_pair_name_len(l.raw, r) : r.name_len, SAM_COPY);
    o.ch('\t');
    if (pair)
        o.num(1u | (l.proper ? 2u : 0u) | (own ? 0u : 4u) | (l.mate_mapped ? 0u : 8u) | (own && l.strand ? 16u : 0u) |
              (l.mate_mapped && l.mate_strand ? 32u : 0u) | (l.mate ? 128u : 64u));
    else
        o.num(own ? (l.strand ? 16u : 0u) | (l.rank ? 256u : 0u) : 4u);
    o.ch('\t');
    /* POS columns of this line and of the mate's: each its own, else the other's, else 0 */
    const uint32_t pos_x = own ? l.pos + 1u : lent ? l.mate_pos + 1u : 0u;
    const uint32_t pos_y = !pair ? 0u : l.mate_mapped ? l.mate_pos + 1u : own ? l.pos + 1u : 0u;
    if (own) o.bytes(l.rname, l.rname_len, SAM_COPY);
    else if (lent) o.bytes(l.mate_rname, l.mate_rname_len, SAM_COPY);
    else o.ch('*');
    o.ch('\t');
    o.num(pos_x);
    o.ch('\t');
    if (own) sam_int(o, l.mapq);
    else o.ch('0');
    o.ch('\t');
    if (!own || l.nops > (uint32_t)SAM_CIGAR_CAP) {
        o.ch('*');
    } else {
        for (uint32_t i = 0; i < l.nops; i++) {
            o.num((uint32_t)(l.ops[i] >> 3));
            o.ch("MID=X???"[l.ops[i] & 7]);
        }
    }
    o.ch('\t');
    if (!pair || !l.mate_mapped) o.ch('*');
    else if (!own || l.mate_seq_id == l.seq_id) o.ch('=');
    else o.bytes(l.mate_rname, l.mate_rname_len, SAM_COPY);
    o.ch('\t');
    o.num(pos_y);
    o.ch('\t');
    /* +tlen on the mate with the smaller POS column, mate 1 when they are equal */
    if (pair && l.tlen != 0 && !(l.mate ? pos_x < pos_y : pos_x <= pos_y)) o.ch('-');
    o.num(pair ? l.tlen : 0u);
    o.ch('\t');
    if (own && l.rank) {
        SAM_LIT(o, "*\t*");
    } else {
        if (r.seq_len) o.bytes(l.raw + r.seq, r.seq_len, own && l.strand ? SAM_REVCOMP : SAM_UPPER);
        else o.ch('*');
        o.ch('\t');
        if (r.qual_len) o.bytes(l.raw + r.qual, r.qual_len, own && l.strand ? SAM_REVERSE : SAM_COPY);
        else o.ch('*');
    }
    if (own) {
        SAM_LIT(o, "\tNM:i:");
        sam_int(o, l.dist);
        SAM_LIT(o, "\tXG:i:");
        sam_int(o, l.greedy_cost);
        if (l.md_len) {
            SAM_LIT(o, "\tMD:Z:");
            o.bytes(l.md, l.md_len, SAM_COPY);
        }
    }
    if (pair && l.proper) {
        SAM_LIT(o, "\tXP:i:");
        o.num(l.n_concordant);
    }
    if (pair && l.rescued) SAM_LIT(o, "\tXR:i:1");
    if (own && l.all) {
        SAM_LIT(o, "\tNH:i:");
        o.num(l.n_reported);
        SAM_LIT(o, "\tHI:i:");
        o.num(l.rank + 1u);
        SAM_LIT(o, "\tXH:i:");
        o.num(l.n_hits);
    }
    o.ch('\n');
}

SAM_HD uint64_t sam_line_size(const SamLine& l) {
    SamSizeSink s;
    sam_format(l, s);
    return s.cur;
}
SAM_HD void sam_line_emit(const SamLine& l, char* out, uint32_t lane) {
    SamLaneSink s{out, lane};
    sam_format(l, s);
}

/* The coordinate-sort key of the line sam_format writes for l (asm_map_file_sorted, asm_sam_sort.h): tid << 32 | POS, where tid is
 * the sequence whose name stands in the RNAME column (n_seqs for '*', which sorts behind every sequence) and POS the number in the
 * POS column.  own and lent are sam_format's: an unmapped mate that borrows RNAME and POS sorts with its mapped mate.
 * tests/test_sam_sort_host.py reads the key back from the text of every case. */
SAM_HD uint64_t sam_sort_key(const SamLine& l, int32_t n_seqs) {
    const bool pair = l.paired != 0, own = l.mapped != 0, lent = pair && !own && l.mate_mapped;
    const uint32_t tid = own ? (uint32_t)l.seq_id : lent ? (uint32_t)l.mate_seq_id : (uint32_t)n_seqs;
    const uint32_t pos_x = own ? l.pos + 1u : lent ? l.mate_pos + 1u : 0u;
    return (uint64_t)tid << 32 | pos_x;
}

#if defined(__HIPCC__)
#include "asm_map.h"

/* what the SAM kernels read of a chunk: the records, the line list (line -> record, item) and the finished items */
struct SamArgs {
    const char* raw;
    const SamRec* recs;
    const int32_t* rec_read;    /* record -> library read, -1: not sent (empty or too long) */
    long nrec, nlines;
    const uint32_t* line_rec;
    const uint32_t* line_item;  /* SAM_NO_ITEM: the record was not sent */
    const MapHit* hits;         /* per item */
    const uint16_t* ops;        /* [items][SAM_CIGAR_CAP] */
    const uint8_t* nops;
    const uint8_t* mapq;        /* per item: its MAPQ byte (ASM_MAPQ_GAP); NULL: the reference model, read off the record's greedy_cost */
    const char* md;             /* per item: its MD row, [items][MD_ROW_CAP] (map_md_kernel); NULL: the tag is off */
    const uint8_t* md_len;      /* per item: the row's bytes in use, 0: the line carries no MD */
    const uint32_t* ibase;      /* all hits: first item of every library read (n + 1); NULL: item i is read i */
    const uint32_t* n_hits;     /* all hits: loci per library read, uncapped */
    const char* names;          /* RNAME table: the names back to back */
    const uint32_t* name_off;   /* n_seqs + 1 */
    uint32_t* line_cnt;         /* nrec + 1 */
    const uint32_t* line_base;  /* its exclusive scan */
    unsigned long long* size;   /* nlines + 1 */
    const unsigned long long* off; /* its exclusive scan */
    unsigned long long* n_mapped;  /* += lines of rank 0 that are mapped */
    char* out;
    /* asm_map_pairs_file (the <true> kernels): nrec pairs, recs = [2][nrec] (mate 1 of every pair, then mate 2), rec_read = pair ->
     * sent pair; hits, ops and nops = [2][n_sent]; line 2q + x is mate x of pair q and the line list is not read */
    const uint8_t* pair_state;     /* per sent pair: MAP_PAIR_* */
    const uint32_t* n_conc;        /* per sent pair */
    long n_sent;
    unsigned long long* n_proper;  /* += proper pairs */
    unsigned long long* n_rescued; /* += rescued records */
};

/* lines per record: one, or with all hits one per item of its read */
__global__ __launch_bounds__(256) void sam_line_count_kernel(SamArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.nrec) return;
    uint32_t c = 0u;
    if (i < a.nrec) {
        const int32_t rd = a.rec_read[i];
        c = (rd < 0 || !a.ibase) ? 1u : a.ibase[rd + 1] - a.ibase[rd];
    }
    a.line_cnt[i] = c; /* entry nrec = 0: the scan's last entry is the total */
}

__global__ __launch_bounds__(256) void sam_line_fill_kernel(SamArgs a, uint32_t* __restrict__ line_rec, uint32_t* __restrict__ line_item) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nrec) return;
    const int32_t rd = a.rec_read[i];
    const uint32_t l0 = a.line_base[i], cnt = a.line_base[i + 1] - l0;
    const uint32_t it0 = rd < 0 ? SAM_NO_ITEM : a.ibase ? a.ibase[rd] : (uint32_t)rd;
    for (uint32_t t = 0; t < cnt; t++) {
        line_rec[l0 + t] = (uint32_t)i;
        line_item[l0 + t] = rd < 0 ? SAM_NO_ITEM : it0 + t;
    }
}

/* line 2q + x of a chunk of pairs: mate x of pair q, with what the line shows of the other mate; the pair flags and tlen by the
 * rules of asm_map_pairs (map_pairs_primary) */
__device__ inline SamLine sam_load_pair_line(const SamArgs& a, long l) {
    SamLine s = {};
    const long q = l >> 1;
    const uint32_t x = (uint32_t)(l & 1);
    s.raw = a.raw, s.rec = a.recs[(long)x * a.nrec + q], s.paired = 1, s.mate = x;
    const int32_t rd = a.rec_read[q];
    if (rd < 0) return s;
    const long ix = (long)x * a.n_sent + rd, iy = (long)(1u - x) * a.n_sent + rd;
    const MapHit h = a.hits[ix], g = a.hits[iy];
    const uint32_t st = a.pair_state[rd];
    s.proper = st == MAP_PAIR_CONCORDANT || st == MAP_PAIR_RESCUED1 || st == MAP_PAIR_RESCUED2;
    s.rescued = st == (x ? MAP_PAIR_RESCUED2 : MAP_PAIR_RESCUED1);
    s.n_concordant = a.n_conc[rd];
    if (h.flags & MAP_F_MAPPED) {
        s.mapped = 1, s.seq_id = h.seq_id, s.pos = h.pos, s.dist = h.dist, s.greedy_cost = h.greedy_cost, s.strand = h.strand;
        s.mapq = a.mapq ? (int32_t)a.mapq[ix] : map_mapq_reference(true, h.greedy_cost);
        s.ops = a.ops + (size_t)ix * SAM_CIGAR_CAP, s.nops = a.nops[ix];
        s.rname = a.names + a.name_off[h.seq_id], s.rname_len = a.name_off[h.seq_id + 1] - a.name_off[h.seq_id];
        if (a.md) s.md = a.md + (size_t)ix * MD_ROW_CAP, s.md_len = a.md_len[ix];
    }
    if (g.flags & MAP_F_MAPPED) {
        s.mate_mapped = 1, s.mate_seq_id = g.seq_id, s.mate_pos = g.pos, s.mate_strand = g.strand;
        s.mate_rname = a.names + a.name_off[g.seq_id], s.mate_rname_len = a.name_off[g.seq_id + 1] - a.name_off[g.seq_id];
    }
    if (s.mapped && s.mate_mapped && h.seq_id == g.seq_id) s.tlen = (h.end > g.end ? h.end : g.end) - (h.pos < g.pos ? h.pos : g.pos);
    return s;
}

__device__ inline SamLine sam_load_line(const SamArgs& a, long l) {
    SamLine s = {};
    const uint32_t rec = a.line_rec[l], it = a.line_item[l];
    s.raw = a.raw, s.rec = a.recs[rec];
    if (it == SAM_NO_ITEM) return s;
    const MapHit h = a.hits[it];
    if (!(h.flags & MAP_F_MAPPED)) return s;
    s.mapped = 1, s.seq_id = h.seq_id, s.pos = h.pos, s.dist = h.dist, s.greedy_cost = h.greedy_cost, s.strand = h.strand;
    s.mapq = a.mapq ? (int32_t)a.mapq[it] : map_mapq_reference(true, h.greedy_cost);
    s.ops = a.ops + (size_t)it * SAM_CIGAR_CAP, s.nops = a.nops[it];
    s.rname = a.names + a.name_off[h.seq_id], s.rname_len = a.name_off[h.seq_id + 1] - a.name_off[h.seq_id];
    if (a.md) s.md = a.md + (size_t)it * MD_ROW_CAP, s.md_len = a.md_len[it];
    if (a.ibase) {
        const int32_t rd = a.rec_read[rec];
        s.all = 1, s.rank = it - a.ibase[rd], s.n_reported = a.ibase[rd + 1] - a.ibase[rd], s.n_hits = a.n_hits[rd];
    }
    return s;
}

/* The two kernels below serve both calls and both output formats.  PAIRED picks the load step at compile time (one body holding
 * both makes the compiler merge their stores into the line through a pointer, which costs a stack slot and the single-end path a third
 * more registers); FMT is what a line becomes: size(line) bytes, which emit(line, out, lane) stores (SamText; BamRecord of asm_bam.h) */
template <bool PAIRED>
__device__ inline SamLine sam_load(const SamArgs& a, long l) {
    if constexpr (PAIRED) return sam_load_pair_line(a, l);
    else return sam_load_line(a, l);
}

struct SamText {
    SAM_HD static uint64_t size(const SamLine& l) { return sam_line_size(l); }
    SAM_HD static void emit(const SamLine& l, char* out, uint32_t lane) { sam_line_emit(l, out, lane); }
};

/* one thread per line: its exact byte length */
template <class FMT, bool PAIRED>
__global__ __launch_bounds__(256) void line_size_kernel(SamArgs a) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool primary = false, proper = false, rescued = false;
    if (l < a.nlines) {
        const SamLine s = sam_load<PAIRED>(a, l);
        a.size[l] = FMT::size(s);
        primary = s.mapped && s.rank == 0u;
        proper = s.paired && s.proper && s.mate == 0u, rescued = s.paired && s.rescued;
    } else if (l == a.nlines) {
        a.size[l] = 0ull;
    }
    const unsigned long long m = __ballot(primary);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.n_mapped, (unsigned long long)__popcll(m));
    if constexpr (PAIRED) { /* the counts of a chunk of pairs */
        const unsigned long long mp = __ballot(proper), mr = __ballot(rescued);
        if ((threadIdx.x & 63) == 0 && mp) atomicAdd(a.n_proper, (unsigned long long)__popcll(mp));
        if ((threadIdx.x & 63) == 0 && mr) atomicAdd(a.n_rescued, (unsigned long long)__popcll(mr));
    }
}

/* one wave per line: every lane walks the line's pieces and stores its own bytes, 64 contiguous bytes per store */
template <class FMT, bool PAIRED>
__global__ __launch_bounds__(256) void line_emit_kernel(SamArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long l = wave; l < a.nlines; l += nwaves) FMT::emit(sam_load<PAIRED>(a, l), a.out + a.off[l], lane);
}
#endif /* __HIPCC__ */
