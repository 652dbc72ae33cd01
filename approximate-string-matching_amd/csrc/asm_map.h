// Read mapper kernels (asm_index_build / asm_map_reads; contract: docs/design/mapper.md).
//
// Byte rule here: A, C, G and T match only themselves; every other byte (N, IUPAC codes, ...) mismatches everything, another N
// included.  This is NOT the pack kernel's rule (which turns every non-base byte into A); Greedy, run on the mapped windows
// afterwards, keeps the pack kernel's rule.
//
// Index:   map_upper_kernel (text to upper case), map_kmer_key_kernel (2-bit key of every k-mer that lies inside one sequence
//          and holds only bases; 4^k = "no k-mer here"), hipcub radix sort of (key, position), map_bucket_offsets_kernel
//          (off[b] = first sorted slot with key >= b, 4^k + 1 entries).
// Mapping: work item = (read, strand, piece); map_seed_count_kernel sizes each item's bucket, an exclusive scan numbers the
//          candidates, map_seed_emit_kernel writes those of one round [c0, c1) (a candidate = a piece found exactly = one
//          verification window), map_verify_kernel<W> runs semi-global Myers/Hyyro over the window and folds the window's best
//          (d, strand, seq, end) into the read's packed key with an integer atomicMin, map_finish_kernel<W> finds the start
//          (reverse global bit-vector pass), runs a banded DP under the byte rule and writes the CIGAR, and map_greedy_*
//          gather the Greedy windows of the mapped reads.
// All hits (asm_map_reads_all): map_verify_all_kernel<W> appends every window's maximal intervals of ends within e to a run
//          buffer, a radix sort orders them by (read, strand, position), map_select_count_kernel / map_select_emit_kernel merge
//          them into loci and list the reported ones as items (read, packed key), and the finish and Greedy kernels run once per
//          item.
// Pairs (asm_map_pairs): the mates' run records as for all hits, map_loci_emit_kernel lists each read's loci, map_pair_kernel
//          picks the best concordant pair per pair with two pointers over the mates' lists, map_rescue_kernel<W> searches a mapped
//          mate's insert window for its partner (tiles of ends, 64-bit atomicMin per anchor), map_rescue_pick_kernel keeps the
//          better rescued pair, and the finish and Greedy run on one item per read.
// Secondary pairs (asm_map_pairs_all): the front of asm_map_pairs unchanged, then map_pair_count_kernel counts each pair's eligible
//          concordant pairs, a scan lays out their items, map_pair_emit_kernel lists ranks >= 1 in pair order, and the items' finish
//          and Greedy run as for all hits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "asm_bits.h"

#define MAP_MAX_READ 511      /* longest read: ceil(511 / 64) = 8 pattern words */
#define MAP_MAX_ERRORS 15     /* 4 bits of the packed key; also the banded traceback's half-width */
#define MAP_BAND (2 * MAP_MAX_ERRORS + 1)
#define MAP_MAX_SEQS (1 << 26) /* 26 bits of the packed key */
#define MAP_NO_KEY 0xffffffffffffffffull
#define MAP_BAD_CAND 0xffffffffu

/* asm_map_hit.flags (include/asm_mi355x.h) */
#define MAP_F_MAPPED 1u
#define MAP_F_TOO_SHORT 2u
#define MAP_F_SEED_CAPPED 4u
#define MAP_F_CIGAR_TRUNCATED 8u

struct MapCand {  /* one verification window: T[ws, we) (global text positions) of sequence r for strand s of read `read` */
    uint32_t read; /* MAP_BAD_CAND: the k-mer hit did not extend to the whole piece */
    uint32_t ws, we;
    uint32_t rs;   /* r << 1 | s */
};

/* What a device hit record looks like; the same layout as asm_map_hit of the C ABI (checked in asm_capi.hip). */
struct MapHit {
    int32_t seq_id;
    uint32_t pos, end;
    int16_t dist;
    uint8_t strand, flags;
    int32_t greedy_cost;
};

ASM_DEV uint32_t map_code(uint8_t c) { /* upper-case input: A 0, C 1, G 2, T 3, anything else 4 */
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
ASM_DEV uint8_t map_comp(uint8_t c) {
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
/* byte p of q_s (s = 1: reverse complement) */
ASM_DEV uint8_t map_read_byte(const char* q, uint32_t m, uint32_t s, uint32_t p) {
    return s ? map_comp((uint8_t)q[m - 1u - p]) : (uint8_t)q[p];
}
/* sequence holding global position t: the last r with seq_off[r] <= t (empty sequences are skipped over) */
ASM_DEV uint32_t map_seq_of(const unsigned long long* seq_off, uint32_t n_seqs, unsigned long long t) {
    uint32_t lo = 0, hi = n_seqs; /* seq_off[lo] <= t < seq_off[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seq_off[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void map_upper_kernel(char* __restrict__ s, unsigned long long n) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const char c = s[i];
        if (c >= 'a' && c <= 'z') s[i] = (char)(c - 32);
    }
}

__global__ __launch_bounds__(256) void map_kmer_key_kernel(const char* __restrict__ text, unsigned long long len,
                                                           const unsigned long long* __restrict__ seq_off, uint32_t n_seqs, int k,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t none = 1u << (2 * k);
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < len;
         t += (unsigned long long)gridDim.x * blockDim.x) {
        uint32_t key = none;
        const uint32_t r = map_seq_of(seq_off, n_seqs, t);
        if (t + (unsigned long long)k <= seq_off[r + 1]) {
            uint32_t acc = 0, bad = 0;
            for (int q = 0; q < k; q++) {
                const uint32_t c = map_code((uint8_t)text[t + q]);
                bad |= c >> 2;
                acc = (acc << 2) | (c & 3u);
            }
            if (!bad) key = acc;
        }
        keys[t] = key;
        vals[t] = (uint32_t)t;
    }
}

/* off[b] = number of sorted keys below b, for b in [0, nb) */
__global__ __launch_bounds__(256) void map_bucket_offsets_kernel(const uint32_t* __restrict__ sorted, unsigned long long n,
                                                                 uint32_t nb, uint32_t* __restrict__ off) {
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += gridDim.x * blockDim.x) {
        unsigned long long lo = 0, hi = n;
        while (lo < hi) {
            const unsigned long long mid = (lo + hi) >> 1;
            if (sorted[mid] < b) lo = mid + 1; else hi = mid;
        }
        off[b] = (uint32_t)lo;
    }
}

struct MapSeedArgs {
    const char* reads;          /* upper-cased, concatenated */
    const uint32_t* roff;       /* n + 1 */
    long n;
    int S, P, k, e, max_occ;    /* strands, pieces (= e + 1), k-mer length, max errors, bucket cap (0 = none) */
    const char* text;           /* index text, upper case */
    const uint32_t* ix_off;     /* 4^k + 1 */
    const uint32_t* ix_pos;
    const unsigned long long* seq_off;
    uint32_t n_seqs;
};

/* the piece of work item w: read, strand, read offset, length and first k-mer key; false when it cannot seed (too short a read,
 * a non-base byte in the piece) */
ASM_DEV bool map_piece(const MapSeedArgs& a, long w, uint32_t& read, uint32_t& s, uint32_t& o, uint32_t& plen, uint32_t& key) {
    const long per = (long)a.S * a.P;
    read = (uint32_t)(w / per);
    const uint32_t rem = (uint32_t)(w % per);
    s = rem / (uint32_t)a.P;
    const uint32_t piece = rem % (uint32_t)a.P;
    const uint32_t r0 = a.roff[read], m = a.roff[read + 1] - r0;
    if (m < (uint32_t)(a.P * a.k)) return false;
    const uint32_t L = m / (uint32_t)a.P;
    o = piece * L;
    plen = piece == (uint32_t)a.P - 1u ? m - o : L;
    uint32_t acc = 0, bad = 0;
    for (uint32_t q = 0; q < plen; q++) {
        const uint32_t c = map_code(map_read_byte(a.reads + r0, m, s, o + q));
        bad |= c >> 2;
        if (q < (uint32_t)a.k) acc = (acc << 2) | (c & 3u);
    }
    key = acc;
    return !bad;
}

__global__ __launch_bounds__(256) void map_seed_count_kernel(MapSeedArgs a, unsigned long long* __restrict__ cnt,
                                                             uint32_t* __restrict__ flags) {
    const long nw = a.n * a.S * a.P;
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (long)gridDim.x * blockDim.x) {
        uint32_t read, s, o, plen, key;
        unsigned long long c = 0;
        if (map_piece(a, w, read, s, o, plen, key)) {
            c = a.ix_off[key + 1] - a.ix_off[key];
            if (a.max_occ > 0 && c > (unsigned long long)a.max_occ) {
                c = 0;
                atomicOr(flags + read, MAP_F_SEED_CAPPED);
            }
        }
        cnt[w] = c;
    }
}

/* candidates [c0, c1) of the exclusive scan `base` into cand[0, c1 - c0) */
__global__ __launch_bounds__(256) void map_seed_emit_kernel(MapSeedArgs a, const unsigned long long* __restrict__ base,
                                                            const unsigned long long* __restrict__ cnt, unsigned long long c0,
                                                            unsigned long long c1, MapCand* __restrict__ cand) {
    const long nw = a.n * a.S * a.P;
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (long)gridDim.x * blockDim.x) {
        const unsigned long long b = base[w], c = cnt[w];
        if (!c || b + c <= c0 || b >= c1) continue;
        uint32_t read, s, o, plen, key;
        map_piece(a, w, read, s, o, plen, key);
        const uint32_t r0 = a.roff[read], m = a.roff[read + 1] - r0;
        const unsigned long long qlo = b < c0 ? c0 - b : 0ull, qhi = b + c > c1 ? c1 - b : c;
        const uint32_t first = a.ix_off[key];
        for (unsigned long long q = qlo; q < qhi; q++) {
            const unsigned long long t = a.ix_pos[first + q];
            const uint32_t r = map_seq_of(a.seq_off, a.n_seqs, t);
            const unsigned long long s0 = a.seq_off[r], s1 = a.seq_off[r + 1];
            bool ok = t + plen <= s1;
            for (uint32_t p = (uint32_t)a.k; ok && p < plen; p++) ok = (uint8_t)a.text[t + p] == map_read_byte(a.reads + r0, m, s, o + p);
            MapCand x;
            x.read = ok ? read : MAP_BAD_CAND;
            const long long lo = (long long)t - (long long)o - a.e, hi = (long long)t - (long long)o + (long long)m + a.e;
            x.ws = (uint32_t)(lo < (long long)s0 ? (long long)s0 : lo);
            x.we = (uint32_t)(hi > (long long)s1 ? (long long)s1 : hi);
            x.rs = r << 1 | s;
            cand[b + q - c0] = x;
        }
    }
}

/* One column step of a 64-row block of Myers' bit-vector algorithm (Hyyro's block form).  hin / return: the horizontal delta
 * entering at the block's top / leaving at its bottom, in {-1, 0, +1}.  Bits above the pattern's last row carry junk that never
 * reaches lower bits (carries and shifts only move upwards). */
ASM_DEV int map_myers_step(uint64_t& Pv, uint64_t& Mv, uint64_t Eq, int hin, uint64_t& Ph_out, uint64_t& Mh_out) {
    const uint64_t hneg = hin < 0 ? 1ull : 0ull;
    const uint64_t Xv = Eq | Mv;
    Eq |= hneg;
    const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    uint64_t Ph = Mv | ~(Xh | Pv);
    uint64_t Mh = Pv & Xh;
    Ph_out = Ph, Mh_out = Mh;
    const int hout = (int)(Ph >> 63) - (int)(Mh >> 63);
    Ph <<= 1;
    Mh <<= 1;
    Mh |= hneg;
    Ph |= hin > 0 ? 1ull : 0ull;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return hout;
}

/* Peq masks of the pattern q_s (rev = 1: read backwards, i.e. the pattern is q_s reversed); a non-base byte sets no bit */
template <int W>
ASM_DEV void map_build_peq(const char* q, uint32_t m, uint32_t s, bool rev, uint64_t (&peq)[4][W]) {
#pragma unroll
    for (int w = 0; w < W; w++) {
        uint64_t a = 0, c = 0, g = 0, t = 0;
        const uint32_t p0 = (uint32_t)w * 64u;
        for (uint32_t p = p0; p < m && p < p0 + 64u; p++) {
            const uint32_t code = map_code(map_read_byte(q, m, s, rev ? m - 1u - p : p));
            const uint64_t bit = 1ull << (p - p0);
            a |= code == 0u ? bit : 0ull;
            c |= code == 1u ? bit : 0ull;
            g |= code == 2u ? bit : 0ull;
            t |= code == 3u ? bit : 0ull;
        }
        peq[0][w] = a, peq[1][w] = c, peq[2][w] = g, peq[3][w] = t;
    }
}

/* One text column over all words of a pattern of m rows; returns the change of the last row's score. */
template <int W>
ASM_DEV int map_column(uint64_t (&Pv)[W], uint64_t (&Mv)[W], const uint64_t (&peq)[4][W], uint32_t code, int nw, uint32_t last_bit,
                       int hin0) {
    int h = hin0, delta = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        if (w < nw) {
            const uint64_t Eq = code == 0u ? peq[0][w] : code == 1u ? peq[1][w] : code == 2u ? peq[2][w] : code == 3u ? peq[3][w] : 0ull;
            uint64_t Ph, Mh;
            h = map_myers_step(Pv[w], Mv[w], Eq, h, Ph, Mh);
            if (w == nw - 1) delta = (int)((Ph >> last_bit) & 1ull) - (int)((Mh >> last_bit) & 1ull);
        }
    }
    return delta;
}

/* thread per candidate: the window's best (d, end) and the read's atomicMin over the packed key
 * d << 59 | s << 58 | r << 32 | end (end local to sequence r, exclusive) */
template <int W>
__global__ __launch_bounds__(256) void map_verify_kernel(const MapCand* __restrict__ cand, unsigned long long nc,
                                                         const char* __restrict__ reads, const uint32_t* __restrict__ roff,
                                                         const char* __restrict__ text, const unsigned long long* __restrict__ seq_off,
                                                         int e, unsigned long long* __restrict__ keys) {
    for (unsigned long long c = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; c < nc;
         c += (unsigned long long)gridDim.x * blockDim.x) {
        const MapCand x = cand[c];
        if (x.read == MAP_BAD_CAND) continue;
        const uint32_t r0 = roff[x.read], m = roff[x.read + 1] - r0, s = x.rs & 1u, r = x.rs >> 1;
        uint64_t peq[4][W];
        map_build_peq<W>(reads + r0, m, s, false, peq);
        uint64_t Pv[W], Mv[W];
#pragma unroll
        for (int w = 0; w < W; w++) Pv[w] = ~0ull, Mv[w] = 0ull;
        const int nw = (int)((m + 63u) >> 6);
        const uint32_t last_bit = (m - 1u) & 63u;
        int score = (int)m, best = e + 1;
        uint32_t best_t = 0;
        for (uint32_t t = x.ws; t < x.we; t++) {
            score += map_column<W>(Pv, Mv, peq, map_code((uint8_t)text[t]), nw, last_bit, 0);
            if (score < best) best = score, best_t = t + 1u; /* first end reaching the minimum */
        }
        if (best <= e) {
            const unsigned long long key = (unsigned long long)best << 59 | (unsigned long long)s << 58 |
                                           (unsigned long long)r << 32 | (unsigned long long)(best_t - (uint32_t)seq_off[r]);
            atomicMin(keys + x.read, key);
        }
    }
}

/* ---- all hits (asm_map_reads_all): every locus within e, not only the best ------------------------------------------------
 * A window reports each maximal interval of ends with D_w <= e as a run record: key = read << 33 | s << 32 | lo and val =
 * dmin << 20 | (jmin - lo) << 10 | (hi - lo), where lo, hi and jmin are inclusive global positions (the last text byte of an
 * occurrence; the exclusive end is one more), so that map_seq_of(lo) is the sequence.  A window spans at most 511 + 2 * 15
 * positions, so both offsets fit 10 bits. */
#define MAP_RUN_READ_SHIFT 33
#define MAP_RUN_SPAN_BITS 10

/* a slot in the run buffer for each active lane: one atomicAdd per wave (lanes of a wave close intervals at the same column) */
ASM_DEV unsigned long long map_wave_slot(unsigned long long* counter) {
    const uint64_t mask = __ballot(1);
    const int lane = (int)(threadIdx.x & 63u), leader = __ffsll((long long)mask) - 1;
    const uint32_t below = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)base, leader), hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), leader);
    return ((unsigned long long)hi << 32 | lo) + below;
}

ASM_DEV void map_put_run(unsigned long long* counter, unsigned long long cap, unsigned long long* __restrict__ rkey,
                         uint32_t* __restrict__ rval, uint32_t read, uint32_t s, uint32_t lo, uint32_t hi, int dmin, uint32_t jmin) {
    const unsigned long long slot = map_wave_slot(counter); /* the counter always advances: the host sees how many did not fit */
    if (slot < cap) {
        rkey[slot] = (unsigned long long)read << MAP_RUN_READ_SHIFT | (unsigned long long)s << 32 | lo;
        rval[slot] = (uint32_t)dmin << 20 | (jmin - lo) << MAP_RUN_SPAN_BITS | (hi - lo);
    }
}

/* thread per candidate: the column loop of map_verify_kernel<W>, but every maximal interval of ends with D_w <= e is appended to
 * the run buffer (see above) instead of folding the window's best into an atomicMin */
template <int W>
__global__ __launch_bounds__(256) void map_verify_all_kernel(const MapCand* __restrict__ cand, unsigned long long nc,
                                                             const char* __restrict__ reads, const uint32_t* __restrict__ roff,
                                                             const char* __restrict__ text, int e, unsigned long long* counter,
                                                             unsigned long long cap, unsigned long long* __restrict__ rkey,
                                                             uint32_t* __restrict__ rval) {
    for (unsigned long long c = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; c < nc;
         c += (unsigned long long)gridDim.x * blockDim.x) {
        const MapCand x = cand[c];
        if (x.read == MAP_BAD_CAND) continue;
        const uint32_t r0 = roff[x.read], m = roff[x.read + 1] - r0, s = x.rs & 1u;
        uint64_t peq[4][W];
        map_build_peq<W>(reads + r0, m, s, false, peq);
        uint64_t Pv[W], Mv[W];
#pragma unroll
        for (int w = 0; w < W; w++) Pv[w] = ~0ull, Mv[w] = 0ull;
        const int nw = (int)((m + 63u) >> 6);
        const uint32_t last_bit = (m - 1u) & 63u;
        int score = (int)m, dmin = e + 1;
        uint32_t lo = 0, jmin = 0;
        for (uint32_t t = x.ws; t < x.we; t++) {
            score += map_column<W>(Pv, Mv, peq, map_code((uint8_t)text[t]), nw, last_bit, 0);
            if (score <= e) {
                if (dmin > e) lo = t, dmin = score, jmin = t; /* an interval opens */
                else if (score < dmin) dmin = score, jmin = t;
            } else if (dmin <= e) {
                map_put_run(counter, cap, rkey, rval, x.read, s, lo, t - 1u, dmin, jmin);
                dmin = e + 1;
            }
        }
        if (dmin <= e) map_put_run(counter, cap, rkey, rval, x.read, s, lo, x.we - 1u, dmin, jmin);
    }
}

/* first index of the sorted run keys whose read is >= `read` */
ASM_DEV unsigned long long map_run_lower(const unsigned long long* rkey, unsigned long long nr, unsigned long long read) {
    unsigned long long lo = 0, hi = nr;
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if ((rkey[mid] >> MAP_RUN_READ_SHIFT) < read) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* Walk the sorted run records [b, e) of one read and call f(s, r, d, j) once per locus, in (s, r, j) order: records of the same
 * strand and sequence merge when they overlap or touch (lo <= hi + 1); d = min dmin, j = the smallest jmin among the records
 * reaching it (inclusive global position). */
template <class F>
ASM_DEV void map_walk_loci(const unsigned long long* __restrict__ rkey, const uint32_t* __restrict__ rval, unsigned long long b,
                           unsigned long long e, const unsigned long long* __restrict__ seq_off, uint32_t n_seqs, F&& f) {
    uint32_t cs = 0, cr = 0, chi = 0, cj = 0;
    int cd = -1;
    unsigned long long cend = 0; /* end of sequence cr (exclusive, global) */
    for (unsigned long long q = b; q < e; q++) {
        const unsigned long long k = rkey[q];
        const uint32_t v = rval[q], s = (uint32_t)(k >> 32) & 1u, lo = (uint32_t)k;
        const uint32_t hi = lo + (v & ((1u << MAP_RUN_SPAN_BITS) - 1u)), j = lo + ((v >> MAP_RUN_SPAN_BITS) & ((1u << MAP_RUN_SPAN_BITS) - 1u));
        const int d = (int)(v >> 20);
        if (cd >= 0 && s == cs && (unsigned long long)lo < cend && lo <= chi + 1u) {
            if (hi > chi) chi = hi;
            if (d < cd || (d == cd && j < cj)) cd = d, cj = j;
            continue;
        }
        if (cd >= 0) f(cs, cr, cd, cj);
        cs = s, cr = map_seq_of(seq_off, n_seqs, lo), cend = seq_off[cr + 1], chi = hi, cd = d, cj = j;
    }
    if (cd >= 0) f(cs, cr, cd, cj);
}

struct MapSelectArgs {
    const unsigned long long* rkey; /* sorted */
    const uint32_t* rval;
    unsigned long long nr;
    long n;                          /* reads */
    int e, strata, max_hits;
    const unsigned long long* seq_off;
    uint32_t n_seqs;
    const uint32_t* roff;
    uint32_t* n_hits;                /* per read: loci with d <= min(e, d_best + strata) */
    uint32_t* d_best;                /* per read (count pass), 0 when n_hits = 0 */
    const uint32_t* ibase;           /* per read: first item (emit pass) */
    const unsigned long long* dbase; /* per read: dirs offset of its first item (emit pass) */
    uint32_t* iread;                 /* per item */
    unsigned long long* ikey;        /* per item: d << 59 | s << 58 | r << 32 | j (exclusive, local to r); MAP_NO_KEY = unmapped */
    unsigned long long* idirs;       /* per item */
};

/* thread per read: d_best and n_hits of its loci */
__global__ __launch_bounds__(256) void map_select_count_kernel(MapSelectArgs a) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        const unsigned long long b = map_run_lower(a.rkey, a.nr, (unsigned long long)i), e = map_run_lower(a.rkey, a.nr, (unsigned long long)i + 1);
        int best = a.e + 1;
        map_walk_loci(a.rkey, a.rval, b, e, a.seq_off, a.n_seqs, [&](uint32_t, uint32_t, int d, uint32_t) { best = d < best ? d : best; });
        const int lim = best + a.strata < a.e ? best + a.strata : a.e;
        uint32_t cnt = 0;
        if (best <= a.e)
            map_walk_loci(a.rkey, a.rval, b, e, a.seq_off, a.n_seqs, [&](uint32_t, uint32_t, int d, uint32_t) { cnt += d <= lim; });
        a.n_hits[i] = cnt;
        a.d_best[i] = best <= a.e ? (uint32_t)best : 0u;
    }
}

/* thread per read: its items in (d, s, r, j) order, one walk per d level from d_best up (the walk itself is in (s, r, j) order);
 * a read without loci gets one item with MAP_NO_KEY (the unmapped record) */
__global__ __launch_bounds__(256) void map_select_emit_kernel(MapSelectArgs a) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        const uint32_t q0 = a.ibase[i], m = a.roff[i + 1] - a.roff[i];
        const unsigned long long db = a.dbase[i];
        const uint32_t nh = a.n_hits[i], want = nh < (uint32_t)a.max_hits ? nh : (uint32_t)a.max_hits;
        if (!nh) {
            a.iread[q0] = (uint32_t)i, a.ikey[q0] = MAP_NO_KEY, a.idirs[q0] = db;
            continue;
        }
        const unsigned long long b = map_run_lower(a.rkey, a.nr, (unsigned long long)i), e = map_run_lower(a.rkey, a.nr, (unsigned long long)i + 1);
        uint32_t k = 0;
        for (int lvl = (int)a.d_best[i]; lvl <= a.e && k < want; lvl++)
            map_walk_loci(a.rkey, a.rval, b, e, a.seq_off, a.n_seqs, [&](uint32_t s, uint32_t r, int d, uint32_t j) {
                if (d != lvl || k >= want) return;
                const unsigned long long jl = (unsigned long long)j + 1ull - a.seq_off[r];
                a.iread[q0 + k] = (uint32_t)i;
                a.ikey[q0 + k] = (unsigned long long)d << 59 | (unsigned long long)s << 58 | (unsigned long long)r << 32 | jl;
                a.idirs[q0 + k] = db + (unsigned long long)k * (m + 1u);
                k++;
            });
    }
}

/* ---- paired-end reads (asm_map_pairs) ---------------------------------------------------------------------------------------
 * A chunk of np pairs is mapped as 2 np reads: mate 1 of pair p is read p, mate 2 is read np + p.  The run records are those of
 * asm_map_reads_all; each read's loci are listed in walk order, (s, r, j), as packed keys d << 59 | s << 58 | r << 32 | j (j
 * exclusive, local to r).  Masking d off a key leaves (s, r, j), so a list is sorted by that and its s = 1 part follows its s = 0
 * part.  The pairing picks one item per read (a locus key, or MAP_NO_KEY), so the finish runs on the identity list. */
#define MAP_RESCUE_TILE 128 /* ends per rescue thread */
#define MAP_KEY_D(k) ((int)((k) >> 59))
#define MAP_KEY_S(k) ((uint32_t)((k) >> 58) & 1u)
#define MAP_KEY_R(k) ((uint32_t)((k) >> 32) & (MAP_MAX_SEQS - 1))
#define MAP_KEY_J(k) ((uint32_t)(k))

/* per pair (asm_map_pairs): what the pairing decided */
#define MAP_PAIR_NONE 0u       /* no proper pair: each mate its best hit */
#define MAP_PAIR_CONCORDANT 1u
#define MAP_PAIR_RESCUE 2u     /* no concordant pair, rescue on: the rescue kernels decide */
#define MAP_PAIR_RESCUED1 3u   /* mate 1 rescued (anchor mate 2) */
#define MAP_PAIR_RESCUED2 4u   /* mate 2 rescued (anchor mate 1) */

ASM_DEV unsigned long long map_pack_key(int d, uint32_t s, uint32_t r, uint32_t j) {
    return (unsigned long long)d << 59 | (unsigned long long)s << 58 | (unsigned long long)r << 32 | j;
}

/* thread per read: its loci keys into lkey[lbase[i], ...) in walk order (n_hits of map_select_count_kernel with strata = e), the
 * first index of its s = 1 part into lsplit[i], and its smallest key (the best hit; MAP_NO_KEY without loci) into lbest[i] */
__global__ __launch_bounds__(256) void map_loci_emit_kernel(MapSelectArgs a, const uint32_t* __restrict__ lbase,
                                                            unsigned long long* __restrict__ lkey, uint32_t* __restrict__ lsplit,
                                                            unsigned long long* __restrict__ lbest) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        const unsigned long long b = map_run_lower(a.rkey, a.nr, (unsigned long long)i), e = map_run_lower(a.rkey, a.nr, (unsigned long long)i + 1);
        uint32_t k = lbase[i], split = 0xffffffffu;
        unsigned long long best = MAP_NO_KEY;
        map_walk_loci(a.rkey, a.rval, b, e, a.seq_off, a.n_seqs, [&](uint32_t s, uint32_t r, int d, uint32_t j) {
            const unsigned long long key = map_pack_key(d, s, r, (uint32_t)((unsigned long long)j + 1ull - a.seq_off[r]));
            if (s && split == 0xffffffffu) split = k;
            best = key < best ? key : best;
            lkey[k++] = key;
        });
        lsplit[i] = split == 0xffffffffu ? k : split;
        lbest[i] = best;
    }
}

struct MapPairArgs {
    long np;                           /* pairs; mate 1 = read p, mate 2 = read np + p */
    const uint32_t* roff;              /* 2 np + 1 */
    const uint32_t* lbase;             /* 2 np + 1: loci of read i are lkey[lbase[i], lbase[i + 1]) */
    const uint32_t* lsplit;            /* 2 np: the first of them with s = 1 */
    const unsigned long long* lbest;   /* 2 np: the smallest of them (MAP_NO_KEY: none) */
    const unsigned long long* lkey;
    int min_insert, max_insert, rescue; /* rescue < 0: off */
    unsigned long long* ikey;          /* per read: the item key (MAP_NO_KEY = unmapped) */
    uint32_t* n_conc;                  /* per pair */
    uint8_t* state;                    /* per pair: MAP_PAIR_* */
    uint32_t* anchors;                 /* rescue anchors: read index of the anchor mate, appended */
    uint32_t* n_anchors;
    const unsigned long long* rslot;   /* per read (the rescued mate): d << 32 | j, ~0 = nothing */
    const unsigned long long* seq_off;
};

/* the pair order (d_A + d_B, s_A, r, j_A, j_B) as two words */
struct MapPairRank {
    unsigned long long hi, lo;
};
ASM_DEV MapPairRank map_pair_rank(unsigned long long kA, unsigned long long kB) {
    MapPairRank x;
    x.hi = (unsigned long long)(MAP_KEY_D(kA) + MAP_KEY_D(kB)) << 27 | (unsigned long long)MAP_KEY_S(kA) << 26 | MAP_KEY_R(kA);
    x.lo = (unsigned long long)MAP_KEY_J(kA) << 32 | MAP_KEY_J(kB);
    return x;
}
ASM_DEV bool map_rank_less(const MapPairRank& a, const MapPairRank& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

/* The concordant pairs with F = a locus of list f (s = 0 part [f0, f1), mate length mF) and R = a locus of list g (s = 1 part
 * [g0, g1)): for F in (r, j) order, the R with the same r and j_R in [j_F - mF + min_insert, j_F - mF + max_insert] are a
 * contiguous range of g that only moves forward.  fn(kF, kR) per concordant combination. */
template <class Fn>
ASM_DEV void map_sweep(const unsigned long long* __restrict__ lkey, uint32_t f0, uint32_t f1, uint32_t g0, uint32_t g1, uint32_t mF,
                       int min_insert, int max_insert, Fn&& fn) {
    const unsigned long long RJ = (1ull << 58) - 1ull; /* (r, j) bits of a key */
    uint32_t lo = g0, hi = g0;
    for (uint32_t x = f0; x < f1; x++) {
        const unsigned long long kF = lkey[x];
        const long long r = (long long)MAP_KEY_R(kF), base = (long long)MAP_KEY_J(kF) - (long long)mF;
        const long long jlo = base + min_insert, jhi = base + max_insert;
        if (jhi < 1) continue; /* loci ends are >= 1 */
        const unsigned long long want_lo = (unsigned long long)r << 32 | (unsigned long long)(jlo < 0 ? 0 : jlo > 0xffffffffll ? 0xffffffffll : jlo);
        const unsigned long long want_hi = (unsigned long long)r << 32 | (unsigned long long)(jhi > 0xffffffffll ? 0xffffffffll : jhi);
        while (lo < g1 && (lkey[lo] & RJ) < want_lo) lo++;
        if (hi < lo) hi = lo;
        while (hi < g1 && (lkey[hi] & RJ) <= want_hi) hi++;
        for (uint32_t y = lo; y < hi; y++) fn(kF, lkey[y]);
    }
}

/* thread per pair: the best concordant pair by pair order and n_concordant (the pairs with its d sum), else each mate's best hit
 * (its smallest key) and, with rescue on, each mapped mate as a rescue anchor */
__global__ __launch_bounds__(256) void map_pair_kernel(MapPairArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.np; p += (long)gridDim.x * blockDim.x) {
        const long A = p, B = a.np + p;
        const uint32_t mA = a.roff[A + 1] - a.roff[A], mB = a.roff[B + 1] - a.roff[B];
        const uint32_t a0 = a.lbase[A], a1 = a.lbase[A + 1], b0 = a.lbase[B], b1 = a.lbase[B + 1];
        const uint32_t as = a.lsplit[A], bs = a.lsplit[B];
        MapPairRank best = {~0ull, ~0ull};
        unsigned long long kbA = MAP_NO_KEY, kbB = MAP_NO_KEY;
        uint32_t cnt = 0;
        auto visit = [&](unsigned long long kA, unsigned long long kB) {
            const MapPairRank x = map_pair_rank(kA, kB);
            const unsigned long long sum = x.hi >> 27, bsum = best.hi >> 27;
            if (sum < bsum) cnt = 1;
            else if (sum == bsum && cnt != 0xffffffffu) cnt++;
            if (map_rank_less(x, best)) best = x, kbA = kA, kbB = kB;
        };
        map_sweep(a.lkey, a0, as, bs, b1, mA, a.min_insert, a.max_insert, [&](unsigned long long kF, unsigned long long kR) { visit(kF, kR); });
        map_sweep(a.lkey, b0, bs, as, a1, mB, a.min_insert, a.max_insert, [&](unsigned long long kF, unsigned long long kR) { visit(kR, kF); });
        a.n_conc[p] = cnt;
        if (cnt) {
            a.ikey[A] = kbA, a.ikey[B] = kbB, a.state[p] = (uint8_t)MAP_PAIR_CONCORDANT;
            continue;
        }
        const unsigned long long fA = a.lbest[A], fB = a.lbest[B]; /* the first locus in (d, s, r, j) order: the best hit */
        a.ikey[A] = fA, a.ikey[B] = fB;
        const bool resc = a.rescue >= 0 && (fA != MAP_NO_KEY || fB != MAP_NO_KEY);
        a.state[p] = (uint8_t)(resc ? MAP_PAIR_RESCUE : MAP_PAIR_NONE);
        if (resc) {
            const uint32_t na = (fA != MAP_NO_KEY) + (fB != MAP_NO_KEY);
            uint32_t slot = atomicAdd(a.n_anchors, na);
            if (fA != MAP_NO_KEY) a.anchors[slot++] = (uint32_t)A;
            if (fB != MAP_NO_KEY) a.anchors[slot] = (uint32_t)B;
        }
    }
}

/* the partner of read x and the window of ends [jlo, jhi] (local to the anchor's sequence, clipped to [1, len_r]) in which it is
 * searched on strand 1 - s_X; false when the window is empty */
ASM_DEV bool map_rescue_window(const MapPairArgs& a, uint32_t x, uint32_t& b, uint32_t& mb, long long& jlo, long long& jhi) {
    b = x < (uint32_t)a.np ? x + (uint32_t)a.np : x - (uint32_t)a.np;
    const uint32_t mx = a.roff[x + 1] - a.roff[x];
    mb = a.roff[b + 1] - a.roff[b];
    const unsigned long long k = a.ikey[x];
    const uint32_t r = MAP_KEY_R(k);
    const long long j = (long long)MAP_KEY_J(k), len_r = (long long)(a.seq_off[r + 1] - a.seq_off[r]);
    if (!MAP_KEY_S(k)) jlo = j - mx + a.min_insert, jhi = j - mx + a.max_insert;
    else jlo = j + mb - a.max_insert, jhi = j + mb - a.min_insert;
    jlo = jlo < 1 ? 1 : jlo;
    jhi = jhi > len_r ? len_r : jhi;
    return jlo <= jhi;
}

/* thread per (anchor, tile of MAP_RESCUE_TILE ends): a semi-global Myers/Hyyro pass of the partner q_b (strand 1 - s_X) that starts
 * mb + rescue columns before the tile, so that D is exact wherever D <= rescue; the tile's smallest (D, j) with D <= rescue and
 * D < mb is folded into rslot[b] with a 64-bit atomicMin.  Every anchor has ntile tiles; the anchor count is read on the device. */
template <int W>
__global__ __launch_bounds__(256) void map_rescue_kernel(MapPairArgs a, const char* __restrict__ reads, const char* __restrict__ text,
                                                         uint32_t ntile, unsigned long long* __restrict__ rslot) {
    const unsigned long long nt = (unsigned long long)*a.n_anchors * ntile;
    for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < nt;
         g += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t x = a.anchors[g / ntile], tile = (uint32_t)(g % ntile);
        uint32_t b, mb;
        long long jlo, jhi;
        if (!map_rescue_window(a, x, b, mb, jlo, jhi)) continue;
        const long long tlo = jlo + (long long)tile * MAP_RESCUE_TILE;
        if (tlo > jhi) continue;
        const long long thi = tlo + MAP_RESCUE_TILE - 1 < jhi ? tlo + MAP_RESCUE_TILE - 1 : jhi;
        const unsigned long long k = a.ikey[x];
        const uint32_t s = 1u - MAP_KEY_S(k), r = MAP_KEY_R(k);
        const long long c0 = tlo - (long long)mb - a.rescue; /* first text column (0-based): the smallest start that can reach D <= rescue */
        uint64_t peq[4][W];
        map_build_peq<W>(reads + a.roff[b], mb, s, false, peq);
        uint64_t Pv[W], Mv[W];
#pragma unroll
        for (int w = 0; w < W; w++) Pv[w] = ~0ull, Mv[w] = 0ull;
        const int nw = (int)((mb + 63u) >> 6);
        const uint32_t last_bit = (mb - 1u) & 63u;
        const char* tx = text + a.seq_off[r];
        int score = (int)mb, best = a.rescue + 1;
        uint32_t best_j = 0;
        for (long long t = c0 < 0 ? 0 : c0; t < thi; t++) {
            score += map_column<W>(Pv, Mv, peq, map_code((uint8_t)tx[t]), nw, last_bit, 0);
            if (t + 1 >= tlo && score < best) best = score, best_j = (uint32_t)(t + 1); /* first end reaching the minimum */
        }
        if (best <= a.rescue && best < (int)mb) atomicMin(rslot + b, (unsigned long long)best << 32 | best_j);
    }
}

/* thread per pair in MAP_PAIR_RESCUE: the rescued pair of each anchor (anchor X, rescued locus Y = (d, 1 - s_X, r_X, j)), the one
 * smaller in pair order wins; its rescued mate's item key is written */
__global__ __launch_bounds__(256) void map_rescue_pick_kernel(MapPairArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.np; p += (long)gridDim.x * blockDim.x) {
        if (a.state[p] != MAP_PAIR_RESCUE) continue;
        const long A = p, B = a.np + p;
        const unsigned long long kA = a.ikey[A], kB = a.ikey[B];
        MapPairRank best = {~0ull, ~0ull};
        unsigned long long key = MAP_NO_KEY;
        long who = -1;
        for (int x = 0; x < 2; x++) {
            const long Y = x ? A : B; /* the rescued mate; the anchor is the other one */
            const unsigned long long kX = x ? kB : kA, slot = a.rslot[Y];
            if (kX == MAP_NO_KEY || slot == ~0ull) continue;
            const unsigned long long kY = map_pack_key((int)(slot >> 32), 1u - MAP_KEY_S(kX), MAP_KEY_R(kX), (uint32_t)slot);
            const MapPairRank rk = x ? map_pair_rank(kY, kX) : map_pair_rank(kX, kY);
            if (map_rank_less(rk, best)) best = rk, key = kY, who = Y;
        }
        if (who < 0) {
            a.state[p] = (uint8_t)MAP_PAIR_NONE;
            continue;
        }
        a.ikey[who] = key;
        a.state[p] = (uint8_t)(who == A ? MAP_PAIR_RESCUED1 : MAP_PAIR_RESCUED2);
    }
}

/* ---- secondary pairs (asm_map_pairs_all) -----------------------------------------------------------------------------------------
 * The eligible pairs of pair p are its concordant combinations with d_A + d_B <= sum_best + strata.  In pair order they come, per d
 * sum, as the s_A = 0 half and then the s_A = 1 half, each in (r, j_A, j_B) order; map_pair_walk lists either half in that order. */
struct MapPairAllArgs {
    MapPairArgs pa;                   /* the pairing's loci lists, item keys and states */
    int strata, max_pairs;
    uint32_t* n_pairs;                /* per pair: eligible pairs (uncapped, saturating) */
    uint32_t* sums;                   /* per pair: bit s set when an eligible pair has d sum s (s <= 30) */
    unsigned long long* nitem;        /* np + 1: secondary items per pair, 2 (min(n_pairs, max_pairs) - 1) */
    unsigned long long* ndirs;        /* np + 1: their dirs words, (m_A + 1) + (m_B + 1) per secondary pair */
    const unsigned long long* ibase;  /* np: exclusive scan of nitem */
    const unsigned long long* dbase;  /* np: exclusive scan of ndirs */
    uint32_t* iread;                  /* per secondary item: its read */
    unsigned long long* ikey;         /* per secondary item: its locus key */
    unsigned long long* idirs;        /* per secondary item: its dirs offset */
};

/* For each key kA of [f0, f1) (one mate's loci of one strand, (r, j) order), the keys kB of [g0, g1) (the other mate's loci of the
 * other strand) with the same r and j_B in [j_A + clo, j_A + chi], in (r, j_B) order: a window that only moves forward.  fn(kA, kB)
 * returns false to stop; then so does the walk (returns false). */
template <class Fn>
ASM_DEV bool map_pair_walk(const unsigned long long* __restrict__ lkey, uint32_t f0, uint32_t f1, uint32_t g0, uint32_t g1, long long clo,
                           long long chi, Fn&& fn) {
    const unsigned long long RJ = (1ull << 58) - 1ull; /* (r, j) bits of a key */
    uint32_t lo = g0, hi = g0;
    for (uint32_t x = f0; x < f1; x++) {
        const unsigned long long kA = lkey[x];
        const long long r = (long long)MAP_KEY_R(kA), jlo = (long long)MAP_KEY_J(kA) + clo, jhi = (long long)MAP_KEY_J(kA) + chi;
        if (jhi < 1) continue; /* loci ends are >= 1 */
        const unsigned long long want_lo = (unsigned long long)r << 32 | (unsigned long long)(jlo < 0 ? 0 : jlo > 0xffffffffll ? 0xffffffffll : jlo);
        const unsigned long long want_hi = (unsigned long long)r << 32 | (unsigned long long)(jhi > 0xffffffffll ? 0xffffffffll : jhi);
        while (lo < g1 && (lkey[lo] & RJ) < want_lo) lo++;
        if (hi < lo) hi = lo;
        while (hi < g1 && (lkey[hi] & RJ) <= want_hi) hi++;
        for (uint32_t y = lo; y < hi; y++)
            if (!fn(kA, lkey[y])) return false;
    }
    return true;
}

/* both halves of pair p in pair order within a sum: s_A = 0 (F = A: j_B in [j_A - m_A + min, j_A - m_A + max]), then s_A = 1
 * (F = B: j_B in [j_A + m_B - max, j_A + m_B - min]) */
template <class Fn>
ASM_DEV void map_pair_walk_both(const MapPairArgs& a, long p, Fn&& fn) {
    const long A = p, B = a.np + p;
    const long long mA = (long long)(a.roff[A + 1] - a.roff[A]), mB = (long long)(a.roff[B + 1] - a.roff[B]);
    const uint32_t a0 = a.lbase[A], a1 = a.lbase[A + 1], b0 = a.lbase[B], b1 = a.lbase[B + 1], as = a.lsplit[A], bs = a.lsplit[B];
    if (map_pair_walk(a.lkey, a0, as, bs, b1, a.min_insert - mA, a.max_insert - mA, fn))
        map_pair_walk(a.lkey, as, a1, b0, bs, mB - a.max_insert, mB - a.min_insert, fn);
}

/* thread per pair: n_pairs, the d sums that occur among the eligible pairs and the secondary items' sizes (0 unless CONCORDANT;
 * sum_best is the d sum of the pair map_pair_kernel reported) */
__global__ __launch_bounds__(256) void map_pair_count_kernel(MapPairAllArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.pa.np; p += (long)gridDim.x * blockDim.x) {
        uint32_t cnt = 0, mask = 0;
        unsigned long long ni = 0, nd = 0;
        if (a.pa.state[p] == MAP_PAIR_CONCORDANT) {
            const long A = p, B = a.pa.np + p;
            const int lim = MAP_KEY_D(a.pa.ikey[A]) + MAP_KEY_D(a.pa.ikey[B]) + a.strata;
            map_pair_walk_both(a.pa, p, [&](unsigned long long kA, unsigned long long kB) {
                const int s = MAP_KEY_D(kA) + MAP_KEY_D(kB);
                if (s <= lim) {
                    if (cnt != 0xffffffffu) cnt++;
                    mask |= 1u << s;
                }
                return true;
            });
            const uint32_t sec = cnt ? (cnt < (uint32_t)a.max_pairs ? cnt : (uint32_t)a.max_pairs) - 1u : 0u; /* cnt >= 1 here */
            ni = 2ull * sec;
            nd = (unsigned long long)sec * (a.pa.roff[A + 1] - a.pa.roff[A] + a.pa.roff[B + 1] - a.pa.roff[B] + 2u);
        }
        a.n_pairs[p] = cnt, a.sums[p] = mask, a.nitem[p] = ni, a.ndirs[p] = nd;
    }
}

/* thread per pair with n_pairs >= 2: the occurring sums in ascending order, each sum's pairs in pair order; rank 0 (the pair
 * map_pair_kernel reported) is skipped and the next min(n_pairs, max_pairs) - 1 become items (A, B) at ibase[p] */
__global__ __launch_bounds__(256) void map_pair_emit_kernel(MapPairAllArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.pa.np; p += (long)gridDim.x * blockDim.x) {
        const uint32_t np_ = a.n_pairs[p], want = np_ < (uint32_t)a.max_pairs ? np_ : (uint32_t)a.max_pairs;
        if (want < 2u) continue;
        const long A = p, B = a.pa.np + p;
        const uint32_t mA = a.pa.roff[A + 1] - a.pa.roff[A], mB = a.pa.roff[B + 1] - a.pa.roff[B];
        unsigned long long q = a.ibase[p], dw = a.dbase[p];
        uint32_t k = 0, mask = a.sums[p];
        while (mask && k < want) {
            const int s = __ffs(mask) - 1;
            mask &= mask - 1u;
            map_pair_walk_both(a.pa, p, [&](unsigned long long kA, unsigned long long kB) {
                if (MAP_KEY_D(kA) + MAP_KEY_D(kB) != s) return true;
                if (k) {
                    a.iread[q] = (uint32_t)A, a.ikey[q] = kA, a.idirs[q] = dw;
                    a.iread[q + 1] = (uint32_t)B, a.ikey[q + 1] = kB, a.idirs[q + 1] = dw + mA + 1u;
                    q += 2, dw += mA + mB + 2u;
                }
                return ++k < want;
            });
        }
    }
}

struct MapFinishArgs {
    const char* reads;
    const uint32_t* roff;
    long n;
    int e, P, k, cap;
    const char* text;
    const unsigned long long* seq_off;
    const unsigned long long* keys;     /* per item */
    const uint32_t* flags;              /* per read */
    const uint32_t* iread;              /* ITEMS: per item, its read (else the identity list: item i is read i) */
    const unsigned long long* idirs;    /* ITEMS: per item, its dirs offset (else roff[i] + i) */
    uint64_t* dirs;      /* (m + 1) words per item */
    MapHit* hits;        /* per item */
    uint16_t* ops;       /* [n items][cap] */
    uint8_t* nops;
};

/* thread per item (a read and a packed key; n = items): start (largest i reaching d with end j), banded traceback under the byte
 * rule, CIGAR, hit record.  ITEMS = false is the identity list of asm_map_reads (its own instantiation, so that the indirection
 * costs that call nothing). */
template <int W, bool ITEMS>
__global__ __launch_bounds__(256) void map_finish_kernel(MapFinishArgs a) {
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < a.n; it += (long)gridDim.x * blockDim.x) {
        const long i = ITEMS ? (long)a.iread[it] : it;
        const uint32_t r0 = a.roff[i], m = a.roff[i + 1] - r0;
        const char* q = a.reads + r0;
        const unsigned long long key = a.keys[it];
        MapHit h;
        h.seq_id = -1, h.pos = 0, h.end = 0, h.dist = -1, h.strand = 0, h.greedy_cost = -1;
        uint32_t fl = a.flags[i];
        if (m < (uint32_t)(a.P * a.k)) fl |= MAP_F_TOO_SHORT;
        if (key == MAP_NO_KEY) {
            h.flags = (uint8_t)fl;
            a.hits[it] = h;
            a.nops[it] = 0;
            continue;
        }
        const int d = (int)(key >> 59);
        const uint32_t s = (uint32_t)(key >> 58) & 1u, r = (uint32_t)(key >> 32) & (MAP_MAX_SEQS - 1), j = (uint32_t)key;
        const unsigned long long s0 = a.seq_off[r];
        /* start: reverse global pass over T[lo, j) against q_s reversed; the first length L whose distance is d gives the largest i */
        const uint32_t lo = j >= m + (uint32_t)d ? j - m - (uint32_t)d : 0u;
        uint32_t start = lo;
        {
            uint64_t peq[4][W];
            map_build_peq<W>(q, m, s, true, peq);
            uint64_t Pv[W], Mv[W];
#pragma unroll
            for (int w = 0; w < W; w++) Pv[w] = ~0ull, Mv[w] = 0ull;
            const int nw = (int)((m + 63u) >> 6);
            const uint32_t last_bit = (m - 1u) & 63u;
            int score = (int)m;
            for (uint32_t t = j; t > lo; t--) {
                score += map_column<W>(Pv, Mv, peq, map_code((uint8_t)a.text[s0 + t - 1u]), nw, last_bit, 1);
                if (score == d) {
                    start = t - 1u;
                    break;
                }
            }
        }
        /* banded DP: rows a = 0..m (read), columns b = 0..n (T[start, j)), lanes l <-> diagonal b - a = l - MAP_MAX_ERRORS;
         * dirs: 2 bits per lane, 0 diagonal, 1 up (I), 2 left (D); ties prefer diagonal, then I, then D */
        const int n = (int)(j - start);
        const int INF = 2 * MAP_MAX_ERRORS + 2;
        uint64_t* dirs = a.dirs + (ITEMS ? a.idirs[it] : (unsigned long long)(r0 + (uint32_t)i));
        const char* tx = a.text + s0 + start;
        int row[MAP_BAND];
        uint32_t tw[MAP_BAND]; /* code of text column b = a + delta (1-based: T[start + b - 1]); 5 = outside */
#pragma unroll
        for (int l = 0; l < MAP_BAND; l++) {
            const int dl = l - MAP_MAX_ERRORS;
            row[l] = (dl >= 0 && dl <= n && dl <= d) ? dl : INF;
            const int b = dl; /* row a = 0 before the first shift: column b = delta, its text byte is consumed at row 1 */
            tw[l] = (b >= 0 && b < n) ? map_code((uint8_t)tx[b]) : 5u;
        }
        dirs[0] = 0xaaaaaaaaaaaaaaaaull; /* row 0: left */
        for (int ar = 1; ar <= (int)m; ar++) {
            const uint32_t rc = map_code(map_read_byte(q, m, s, (uint32_t)ar - 1u));
            uint64_t dw = 0;
            int left = INF;
#pragma unroll
            for (int l = 0; l < MAP_BAND; l++) {
                const int dl = l - MAP_MAX_ERRORS, b = ar + dl;
                int v = INF;
                uint32_t dir = 0;
                if (b >= 0 && b <= n && dl >= -d && dl <= d) {
                    /* tw[l] holds the code of T[start + b - 1] at this row (set on the previous row's shift) */
                    const int diag = row[l] + ((rc < 4u && rc == tw[l]) ? 0 : 1);
                    const int up = l + 1 < MAP_BAND ? row[l + 1] + 1 : INF;
                    const int lf = left + 1;
                    v = diag, dir = 0u;
                    if (up < v) v = up, dir = 1u;
                    if (lf < v) v = lf, dir = 2u;
                    if (b == 0) v = up, dir = 1u;
                    if (v > INF) v = INF;
                }
                dw |= (uint64_t)dir << (2 * l);
                left = v;
                row[l] = v; /* row[l + 1] (read above as `up`) is still the previous row's value */
            }
            dirs[ar] = dw;
            /* next row: column of lane l moves one to the right */
#pragma unroll
            for (int l = 0; l < MAP_BAND - 1; l++) tw[l] = tw[l + 1];
            const int bn = ar + 1 + (MAP_BAND - 1 - MAP_MAX_ERRORS); /* column of the last lane on the next row */
            tw[MAP_BAND - 1] = (bn >= 1 && bn <= n) ? map_code((uint8_t)tx[bn - 1]) : 5u;
        }
        /* traceback from (m, n), twice: count the runs, then write them forward */
        int runs = 0;
        for (int pass = 0; pass < 2; pass++) {
            int ar = (int)m, l = n - (int)m + MAP_MAX_ERRORS, k = 0;
            uint32_t op = 7u, len = 0;
            while (ar > 0 || l != MAP_MAX_ERRORS) {
                const uint32_t dir = (uint32_t)(dirs[ar] >> (2 * l)) & 3u;
                const uint32_t o = dir == 0u ? 0u : dir == 1u ? 1u : 2u; /* M, I, D */
                if (o != op && len) {
                    if (pass == 1 && runs - 1 - k < a.cap) a.ops[it * a.cap + (runs - 1 - k)] = (uint16_t)(len << 3 | op);
                    k++;
                    len = 0;
                }
                op = o;
                len++;
                if (dir == 0u) ar--;
                else if (dir == 1u) ar--, l++;
                else l--;
            }
            if (len) {
                if (pass == 1 && runs - 1 - k < a.cap) a.ops[it * a.cap + (runs - 1 - k)] = (uint16_t)(len << 3 | op);
                k++;
            }
            runs = k;
        }
        if (runs > a.cap) fl |= MAP_F_CIGAR_TRUNCATED;
        a.nops[it] = (uint8_t)(runs > 255 ? 255 : runs);
        h.seq_id = (int32_t)r, h.pos = start, h.end = j, h.dist = (int16_t)d, h.strand = (uint8_t)s;
        h.flags = (uint8_t)(fl | MAP_F_MAPPED);
        a.hits[it] = h;
    }
}

/* Greedy windows of the mapped items (list = their indices into hits; iread = each item's read, NULL when item i is read i):
 * T_r[w, min(w + m + 1, len_r)) with w = pos ? pos - 1 : 0, clipped to the read's own sequence.  lens[q] = (read length, window
 * length); the gather writes q_s and the window. */
__global__ __launch_bounds__(256) void map_greedy_lengths_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ iread,
                                                                 long nl, const uint32_t* __restrict__ roff,
                                                                 const MapHit* __restrict__ hits, const unsigned long long* __restrict__ seq_off,
                                                                 uint32_t* __restrict__ qlen, uint32_t* __restrict__ wlen) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nl) return;
    if (q == nl) { /* exclusive scans over nl + 1 entries give the totals */
        qlen[nl] = 0u, wlen[nl] = 0u;
        return;
    }
    const uint32_t it = list[q], i = iread ? iread[it] : it, m = roff[i + 1] - roff[i];
    const MapHit h = hits[it];
    const unsigned long long len_r = seq_off[h.seq_id + 1] - seq_off[h.seq_id];
    const unsigned long long w = h.pos ? h.pos - 1u : 0u, e = w + m + 1ull < len_r ? w + m + 1ull : len_r;
    qlen[q] = m;
    wlen[q] = (uint32_t)(e - w);
}

__global__ __launch_bounds__(256) void map_greedy_gather_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ iread,
                                                                long nl, const char* __restrict__ reads,
                                                                const uint32_t* __restrict__ roff, const MapHit* __restrict__ hits,
                                                                const char* __restrict__ text, const unsigned long long* __restrict__ seq_off,
                                                                const uint32_t* __restrict__ qoff, const uint32_t* __restrict__ woff,
                                                                char* __restrict__ qout, char* __restrict__ wout) {
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    for (long q = wave; q < nl; q += nwaves) { /* one wave per window */
        const uint32_t it = list[q], i = iread ? iread[it] : it, r0 = roff[i], m = roff[i + 1] - r0;
        const MapHit h = hits[it];
        const unsigned long long w = seq_off[h.seq_id] + (h.pos ? h.pos - 1u : 0u);
        for (uint32_t p = (uint32_t)lane; p < m; p += 64u) qout[qoff[q] + p] = (char)map_read_byte(reads + r0, m, h.strand, p);
        const uint32_t o = woff[q], len = woff[q + 1] - o;
        for (uint32_t p = (uint32_t)lane; p < len; p += 64u) wout[o + p] = text[w + p];
    }
}

/* The finish stage with the records left on the device (asm_map_file): which items are mapped (n + 1 entries, the last 0, for the
 * exclusive scan that numbers them), their list, and Greedy's costs into their records. */
__global__ __launch_bounds__(256) void map_mapped_flag_kernel(const MapHit* __restrict__ hits, long n, uint32_t* __restrict__ flag) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n) flag[q] = (q < n && (hits[q].flags & MAP_F_MAPPED)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void map_mapped_list_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ slot, long n,
                                                              uint32_t* __restrict__ list) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n && flag[q]) list[slot[q]] = (uint32_t)q;
}

__global__ __launch_bounds__(256) void map_cost_kernel(const uint32_t* __restrict__ list, const int32_t* __restrict__ cost, long nl,
                                                       MapHit* __restrict__ hits) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nl) hits[list[q]].greedy_cost = cost[q];
}
