// SAM lines of asm_map_file (contract: docs/design/mapper.md, "Files: FASTQ in, SAM out"): the text of one output line, written
// once for three users.  sam_format<Sink> walks the fields of a line in order and hands every piece to a sink:
//   SamSizeSink  adds the lengths                      (sam_size_kernel: one thread per line)
//   SamLaneSink  stores the bytes p = lane (mod 64)    (sam_emit_kernel: one wave per line, 64 contiguous bytes per store)
// so the size and the bytes cannot disagree.  The part above the kernels holds no HIP: host/sam_host_check.cpp compiles it with
// plain g++ under ASan + UBSan and runs the lane sink for lanes 0..63 in turn (tests/test_map_file_host.py).
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
    uint32_t strand, rank;
    const uint16_t* ops; /* count << 3 | op */
    uint32_t nops;
    const char* rname;
    uint32_t rname_len;
    int all; /* max_hits > 0: NH, HI and XH follow */
    uint32_t n_reported, n_hits;
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

/* QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ QUAL [NM XG [NH HI XH]] */
template <class Sink>
SAM_HD void sam_format(const SamLine& l, Sink& o) {
    const SamRec& r = l.rec;
    o.bytes(l.raw + r.name, r.name_len, SAM_COPY);
    if (!l.mapped) {
        SAM_LIT(o, "\t4\t*\t0\t0\t*\t*\t0\t0\t");
        if (r.seq_len) o.bytes(l.raw + r.seq, r.seq_len, SAM_UPPER);
        else o.ch('*');
        o.ch('\t');
        if (r.qual_len) o.bytes(l.raw + r.qual, r.qual_len, SAM_COPY);
        else o.ch('*');
        o.ch('\n');
        return;
    }
    o.ch('\t');
    o.num((l.strand ? 16u : 0u) | (l.rank ? 256u : 0u));
    o.ch('\t');
    o.bytes(l.rname, l.rname_len, SAM_COPY);
    o.ch('\t');
    o.num(l.pos + 1u);
    o.ch('\t');
    sam_int(o, l.greedy_cost + 60 < 254 ? l.greedy_cost + 60 : 254);
    o.ch('\t');
    if (l.nops > (uint32_t)SAM_CIGAR_CAP) {
        o.ch('*');
    } else {
        for (uint32_t i = 0; i < l.nops; i++) {
            o.num((uint32_t)(l.ops[i] >> 3));
            o.ch("MID=X???"[l.ops[i] & 7]);
        }
    }
    SAM_LIT(o, "\t*\t0\t0\t");
    if (l.rank) {
        SAM_LIT(o, "*\t*");
    } else {
        o.bytes(l.raw + r.seq, r.seq_len, l.strand ? SAM_REVCOMP : SAM_UPPER);
        o.ch('\t');
        if (r.qual_len) o.bytes(l.raw + r.qual, r.qual_len, l.strand ? SAM_REVERSE : SAM_COPY);
        else o.ch('*');
    }
    SAM_LIT(o, "\tNM:i:");
    sam_int(o, l.dist);
    SAM_LIT(o, "\tXG:i:");
    sam_int(o, l.greedy_cost);
    if (l.all) {
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

__device__ inline SamLine sam_load_line(const SamArgs& a, long l) {
    SamLine s = {};
    const uint32_t rec = a.line_rec[l], it = a.line_item[l];
    s.raw = a.raw, s.rec = a.recs[rec];
    if (it == SAM_NO_ITEM) return s;
    const MapHit h = a.hits[it];
    if (!(h.flags & MAP_F_MAPPED)) return s;
    s.mapped = 1, s.seq_id = h.seq_id, s.pos = h.pos, s.dist = h.dist, s.greedy_cost = h.greedy_cost, s.strand = h.strand;
    s.ops = a.ops + (size_t)it * SAM_CIGAR_CAP, s.nops = a.nops[it];
    s.rname = a.names + a.name_off[h.seq_id], s.rname_len = a.name_off[h.seq_id + 1] - a.name_off[h.seq_id];
    if (a.ibase) {
        const int32_t rd = a.rec_read[rec];
        s.all = 1, s.rank = it - a.ibase[rd], s.n_reported = a.ibase[rd + 1] - a.ibase[rd], s.n_hits = a.n_hits[rd];
    }
    return s;
}

/* one thread per line: its exact byte length */
__global__ __launch_bounds__(256) void sam_size_kernel(SamArgs a) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool primary = false;
    if (l < a.nlines) {
        const SamLine s = sam_load_line(a, l);
        a.size[l] = sam_line_size(s);
        primary = s.mapped && s.rank == 0u;
    } else if (l == a.nlines) {
        a.size[l] = 0ull;
    }
    const unsigned long long m = __ballot(primary);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.n_mapped, (unsigned long long)__popcll(m));
}

/* one wave per line: every lane walks the line's pieces and stores its own bytes, 64 contiguous bytes per store */
__global__ __launch_bounds__(256) void sam_emit_kernel(SamArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long l = wave; l < a.nlines; l += nwaves) sam_line_emit(sam_load_line(a, l), a.out + a.off[l], lane);
}
#endif /* __HIPCC__ */
