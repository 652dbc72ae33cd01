// Per-thread core of the read mapper (kernels: asm_map.h, contract: docs/design/mapper.md): what one thread computes about one work
// item, written once, with no HIP in it (no atomics, no wave intrinsics, no block index).  hipcc compiles it into the kernels, plain
// g++ into host/map_host_check.cpp, the serial mirror of the pipeline that tests/test_map_core_host.py runs under ASan + UBSan.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define MAP_HD __host__ __device__ __forceinline__
#else
#define MAP_HD static inline
#endif

#define MAP_MAX_READ 511      /* longest read: ceil(511 / 64) = 8 pattern words */
#define MAP_MAX_ERRORS 15     /* 4 bits of the packed key; also the banded traceback's half-width */
#define MAP_BAND (2 * MAP_MAX_ERRORS + 1)
#define MAP_MAX_SEQS (1 << 26) /* 26 bits of the packed key */
#define MAP_NO_KEY 0xffffffffffffffffull
#define MAP_BAD_CAND 0xffffffffu
#define MAP_RESCUE_TILE 128 /* ends per rescue thread */

#define MAP_F_MAPPED 1u /* asm_map_hit.flags (include/asm_mi355x.h) */
#define MAP_F_TOO_SHORT 2u
#define MAP_F_SEED_CAPPED 4u
#define MAP_F_CIGAR_TRUNCATED 8u
struct MapCand {  /* one verification window: T[ws, we) (global text positions) of sequence r for strand s of read `read` */
    uint32_t read; /* MAP_BAD_CAND: the k-mer hit did not extend to the whole piece */
    uint32_t ws, we;
    uint32_t rs;   /* r << 1 | s */
};
struct MapHit { /* a device hit record: the layout of asm_map_hit of the C ABI (checked in asm_map_host.h) */
    int32_t seq_id;
    uint32_t pos, end;
    int16_t dist;
    uint8_t strand, flags;
    int32_t greedy_cost;
};
#define MAP_HIT_UNMAPPED {-1, 0, 0, -1, 0, 0, -1} /* the unmapped record, as MapHit or asm_map_hit */
/* upper-case input: A 0, C 1, G 2, T 3, anything else 4 */
MAP_HD uint32_t map_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
MAP_HD uint8_t map_comp(uint8_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
MAP_HD uint8_t map_read_byte(const char* q, uint32_t m, uint32_t s, uint32_t p) { /* byte p of q_s (s = 1: reverse complement) */
    return s ? map_comp((uint8_t)q[m - 1u - p]) : (uint8_t)q[p];
}
/* sequence holding global position t: the last r with seq_off[r] <= t (empty sequences are skipped over) */
MAP_HD uint32_t map_seq_of(const unsigned long long* seq_off, uint32_t n_seqs, unsigned long long t) {
    uint32_t lo = 0, hi = n_seqs; /* seq_off[lo] <= t < seq_off[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seq_off[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
/* packed locus key d << 59 | s << 58 | r << 32 | j (j = exclusive end, local to sequence r): an integer minimum over keys is the tie
 * order (d, s, r, j), masking d off leaves (s, r, j); MAP_NO_KEY = unmapped */
#define MAP_KEY_D(k) ((int)((k) >> 59))
#define MAP_KEY_S(k) ((uint32_t)((k) >> 58) & 1u)
#define MAP_KEY_R(k) ((uint32_t)((k) >> 32) & (MAP_MAX_SEQS - 1))
#define MAP_KEY_J(k) ((uint32_t)(k))
#define MAP_KEY_RJ(k) ((k) & ((1ull << 58) - 1ull))
MAP_HD unsigned long long map_pack_key(int d, uint32_t s, uint32_t r, uint32_t j) {
    return (unsigned long long)d << 59 | (unsigned long long)s << 58 | (unsigned long long)r << 32 | j;
}

/* run record (all hits), one maximal interval of ends with D <= e of one window: key = read << 33 | s << 32 | lo and val = dmin << 20 |
 * (jmin - lo) << 10 | (hi - lo), where lo, hi and jmin are inclusive global positions (the last text byte of an occurrence; the
 * exclusive end is one more), so that map_seq_of(lo) is the sequence.  A window spans at most 511 + 2 * 15 positions, so both
 * offsets fit 10 bits. */
#define MAP_RUN_READ_SHIFT 33
#define MAP_RUN_SPAN_BITS 10
MAP_HD void map_run_pack(uint32_t read, uint32_t s, uint32_t lo, uint32_t hi, int dmin, uint32_t jmin, unsigned long long& key, uint32_t& val) {
    key = (unsigned long long)read << MAP_RUN_READ_SHIFT | (unsigned long long)s << 32 | lo;
    val = (uint32_t)dmin << (2 * MAP_RUN_SPAN_BITS) | (jmin - lo) << MAP_RUN_SPAN_BITS | (hi - lo);
}
MAP_HD void map_run_unpack(unsigned long long key, uint32_t val, uint32_t& s, uint32_t& lo, uint32_t& hi, int& dmin, uint32_t& jmin) {
    const uint32_t span = (1u << MAP_RUN_SPAN_BITS) - 1u;
    s = (uint32_t)(key >> 32) & 1u, lo = (uint32_t)key;
    hi = lo + (val & span), jmin = lo + ((val >> MAP_RUN_SPAN_BITS) & span), dmin = (int)(val >> (2 * MAP_RUN_SPAN_BITS));
}
/* 2-bit key of the first k of the n bytes byte(0), ..., byte(n - 1); false when one of the n is no base */
template <class B>
MAP_HD bool map_kmer_key(B&& byte, uint32_t n, uint32_t k, uint32_t& key) {
    uint32_t acc = 0, bad = 0;
    for (uint32_t q = 0; q < n; q++) {
        const uint32_t c = map_code(byte(q));
        bad |= c >> 2;
        if (q < k) acc = (acc << 2) | (c & 3u);
    }
    key = acc;
    return !bad;
}
struct MapSeedArgs {
    const char* reads;               /* upper-cased, concatenated */
    const uint32_t* roff;            /* n + 1 */
    long n;
    int S, P, k, e, max_occ;         /* strands, pieces (= e + 1), k-mer length, max errors, bucket cap (0 = none) */
    const char* text;                /* index text, upper case */
    const uint32_t *ix_off, *ix_pos; /* 4^k + 1 bucket offsets; positions sorted by k-mer */
    const unsigned long long* seq_off;
    uint32_t n_seqs;
};
struct MapPiece {
    uint32_t read, s, o, plen, key; /* read, strand, offset in q_s, length, key of its first k-mer */
    uint32_t r0, m;                 /* the read's bytes: reads[r0, r0 + m) */
};
/* the piece of work item w = (read, strand, piece); false when it cannot seed (too short a read, a non-base byte in the piece) */
MAP_HD bool map_piece(const MapSeedArgs& a, long w, MapPiece& pc) {
    const long per = (long)a.S * a.P;
    pc.read = (uint32_t)(w / per);
    const uint32_t rem = (uint32_t)(w % per), piece = rem % (uint32_t)a.P;
    pc.s = rem / (uint32_t)a.P;
    pc.r0 = a.roff[pc.read], pc.m = a.roff[pc.read + 1] - pc.r0;
    if (pc.m < (uint32_t)(a.P * a.k)) return false;
    const uint32_t L = pc.m / (uint32_t)a.P;
    pc.o = piece * L;
    pc.plen = piece == (uint32_t)a.P - 1u ? pc.m - pc.o : L;
    return map_kmer_key([&](uint32_t q) { return map_read_byte(a.reads + pc.r0, pc.m, pc.s, pc.o + q); }, pc.plen, (uint32_t)a.k, pc.key);
}

/* the candidate of a piece whose first k-mer occurs at global position t: MAP_BAD_CAND unless the rest of the piece follows inside the
 * same sequence; the window is the piece's diagonal widened by e on both sides and clipped to the sequence */
MAP_HD MapCand map_candidate(const MapSeedArgs& a, const MapPiece& pc, unsigned long long t) {
    const uint32_t r = map_seq_of(a.seq_off, a.n_seqs, t);
    const unsigned long long s0 = a.seq_off[r], s1 = a.seq_off[r + 1];
    bool ok = t + pc.plen <= s1;
    for (uint32_t p = (uint32_t)a.k; ok && p < pc.plen; p++)
        ok = (uint8_t)a.text[t + p] == map_read_byte(a.reads + pc.r0, pc.m, pc.s, pc.o + p);
    MapCand x;
    x.read = ok ? pc.read : MAP_BAD_CAND;
    const long long lo = (long long)t - (long long)pc.o - a.e, hi = (long long)t - (long long)pc.o + (long long)pc.m + a.e;
    x.ws = (uint32_t)(lo < (long long)s0 ? (long long)s0 : lo);
    x.we = (uint32_t)(hi > (long long)s1 ? (long long)s1 : hi);
    x.rs = r << 1 | pc.s;
    return x;
}

/* One column step of a 64-row block of Myers' bit-vector algorithm (Hyyro's block form).  hin / return: the horizontal delta entering
 * at the block's top / leaving at its bottom.  Bits above the pattern's last row carry junk that never reaches lower bits. */
MAP_HD int map_myers_step(uint64_t& Pv, uint64_t& Mv, uint64_t Eq, int hin, uint64_t& Ph_out, uint64_t& Mh_out) {
    const uint64_t hneg = hin < 0 ? 1ull : 0ull, Xv = Eq | Mv;
    Eq |= hneg;
    const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    uint64_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
    Ph_out = Ph, Mh_out = Mh;
    const int hout = (int)(Ph >> 63) - (int)(Mh >> 63);
    Ph = Ph << 1 | (hin > 0 ? 1ull : 0ull);
    Mh = Mh << 1 | hneg;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return hout;
}

/* Peq masks of the pattern q_s (rev = 1: read backwards, i.e. the pattern is q_s reversed); a non-base byte sets no bit */
template <int W>
MAP_HD void map_build_peq(const char* q, uint32_t m, uint32_t s, bool rev, uint64_t (&peq)[4][W]) {
#pragma unroll
    for (int w = 0; w < W; w++) {
        uint64_t a = 0, c = 0, g = 0, t = 0;
        const uint32_t p0 = (uint32_t)w * 64u;
        for (uint32_t p = p0; p < m && p < p0 + 64u; p++) {
            const uint32_t code = map_code(map_read_byte(q, m, s, rev ? m - 1u - p : p));
            const uint64_t bit = 1ull << (p - p0);
            a |= code == 0u ? bit : 0ull, c |= code == 1u ? bit : 0ull;
            g |= code == 2u ? bit : 0ull, t |= code == 3u ? bit : 0ull;
        }
        peq[0][w] = a, peq[1][w] = c, peq[2][w] = g, peq[3][w] = t;
    }
}

/* One text column over all words of a pattern of m rows; returns the change of the last row's score. */
template <int W>
MAP_HD int map_column(uint64_t (&Pv)[W], uint64_t (&Mv)[W], const uint64_t (&peq)[4][W], uint32_t code, int nw, uint32_t last_bit, int hin0) {
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

/* The column state of a pattern of m <= 64 W rows.  map_myers_init: the column before the first text byte (score m); map_myers_next
 * takes one text byte's code and the delta entering row 0 (0: semi-global, 1: global) and returns the last row's score. */
template <int W>
struct MapMyers {
    uint64_t peq[4][W], Pv[W], Mv[W];
    int nw, score;
    uint32_t last_bit;
};
template <int W>
MAP_HD void map_myers_init(MapMyers<W>& y, const char* q, uint32_t m, uint32_t s, bool rev) {
    map_build_peq<W>(q, m, s, rev, y.peq);
#pragma unroll
    for (int w = 0; w < W; w++) y.Pv[w] = ~0ull, y.Mv[w] = 0ull;
    y.nw = (int)((m + 63u) >> 6), y.last_bit = (m - 1u) & 63u, y.score = (int)m;
}
template <int W>
MAP_HD int map_myers_next(MapMyers<W>& y, uint32_t code, int hin) {
    return y.score += map_column<W>(y.Pv, y.Mv, y.peq, code, y.nw, y.last_bit, hin);
}

/* Best end of q_s in text[t0, t1): the smallest score below `limit` among the exclusive ends >= first (earlier columns only warm the
 * state up) and the first end reaching it.  Returns the score, `limit` when no end is below it. */
template <int W, class T>
MAP_HD int map_best_end(const char* q, uint32_t m, uint32_t s, const char* text, T t0, T t1, T first, int limit, T& best_end) {
    MapMyers<W> my;
    map_myers_init(my, q, m, s, false);
    int best = limit;
    for (T t = t0; t < t1; t++) {
        const int score = map_myers_next(my, map_code((uint8_t)text[t]), 0);
        if (t + 1 >= first && score < best) best = score, best_end = t + 1; /* first end reaching the minimum */
    }
    return best;
}

/* Every maximal interval of ends of q_s in text[ws, we) with D <= e: emit(lo, hi, dmin, jmin), positions of the last text byte
 * (inclusive), jmin the first one reaching dmin. */
template <int W, class F>
MAP_HD void map_scan_runs(const char* q, uint32_t m, uint32_t s, const char* text, uint32_t ws, uint32_t we, int e, F&& emit) {
    MapMyers<W> my;
    map_myers_init(my, q, m, s, false);
    int dmin = e + 1;
    uint32_t lo = 0, jmin = 0;
    for (uint32_t t = ws; t < we; t++) {
        const int score = map_myers_next(my, map_code((uint8_t)text[t]), 0);
        if (score <= e) {
            if (dmin > e) lo = t, dmin = score, jmin = t; /* an interval opens */
            else if (score < dmin) dmin = score, jmin = t;
        } else if (dmin <= e) {
            emit(lo, t - 1u, dmin, jmin);
            dmin = e + 1;
        }
    }
    if (dmin <= e) emit(lo, we - 1u, dmin, jmin);
}

/* Start of the occurrence of q_s that ends at j (exclusive, local to the sequence tx) with distance d: a reverse global pass over
 * tx[lo, j), lo = max(j - m - d, 0), against q_s reversed; the first length whose distance is d gives the largest start. */
template <int W>
MAP_HD uint32_t map_find_start(const char* q, uint32_t m, uint32_t s, const char* tx, uint32_t j, int d) {
    const uint32_t lo = j >= m + (uint32_t)d ? j - m - (uint32_t)d : 0u;
    MapMyers<W> my;
    map_myers_init(my, q, m, s, true);
    for (uint32_t t = j; t > lo; t--)
        if (map_myers_next(my, map_code((uint8_t)tx[t - 1u]), 1) == d) return t - 1u;
    return lo;
}

/* first index of the sorted run keys whose read is >= `read` */
MAP_HD unsigned long long map_run_lower(const unsigned long long* rkey, unsigned long long nr, unsigned long long read) {
    unsigned long long lo = 0, hi = nr;
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if ((rkey[mid] >> MAP_RUN_READ_SHIFT) < read) lo = mid + 1; else hi = mid;
    }
    return lo;
}
struct MapRange { unsigned long long b, e; };
MAP_HD MapRange map_read_runs(const unsigned long long* rkey, unsigned long long nr, long i) { /* the records [b, e) of read i */
    return {map_run_lower(rkey, nr, (unsigned long long)i), map_run_lower(rkey, nr, (unsigned long long)i + 1)};
}

/* Walk the sorted run records [b, e) of one read and call f(s, r, d, j) once per locus, in (s, r, j) order: records of the same
 * strand and sequence merge when they overlap or touch (lo <= hi + 1); d = min dmin, j = the smallest jmin among the records
 * reaching it (inclusive global position). */
template <class F>
MAP_HD void map_walk_loci(const unsigned long long* __restrict__ rkey, const uint32_t* __restrict__ rval, unsigned long long b,
                          unsigned long long e, const unsigned long long* __restrict__ seq_off, uint32_t n_seqs, F&& f) {
    uint32_t cs = 0, cr = 0, chi = 0, cj = 0;
    int cd = -1;
    unsigned long long cend = 0; /* end of sequence cr (exclusive, global) */
    for (unsigned long long q = b; q < e; q++) {
        uint32_t s, lo, hi, j;
        int d;
        map_run_unpack(rkey[q], rval[q], s, lo, hi, d, j);
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
MAP_HD unsigned long long map_locus_key(const unsigned long long* seq_off, uint32_t s, uint32_t r, int d, uint32_t j) {
    return map_pack_key(d, s, r, (uint32_t)((unsigned long long)j + 1ull - seq_off[r])); /* the end: exclusive, local to r */
}

/* Paired-end reads: a chunk of np pairs is mapped as 2 np reads, mate 1 of pair p is read p, mate 2 is read np + p.  Each read's loci
 * are listed in walk order, (s, r, j), as packed keys, so a list is sorted by (s, r, j) and its s = 1 part follows its s = 0 part. */
#define MAP_PAIR_NONE 0u       /* no proper pair: each mate its best hit */
#define MAP_PAIR_CONCORDANT 1u
#define MAP_PAIR_RESCUE 2u     /* no concordant pair, rescue on: the rescue kernels decide */
#define MAP_PAIR_RESCUED1 3u   /* mate 1 rescued (anchor mate 2) */
#define MAP_PAIR_RESCUED2 4u   /* mate 2 rescued (anchor mate 1) */
struct MapPairArgs {
    long np;                               /* pairs; mate 1 = read p, mate 2 = read np + p */
    const uint32_t *roff, *lbase, *lsplit; /* 2 np (+ 1): loci of read i are lkey[lbase[i], lbase[i + 1]), from lsplit[i] on s = 1 */
    const unsigned long long *lbest, *lkey; /* lbest: 2 np, the smallest of them (MAP_NO_KEY: none) */
    int min_insert, max_insert, rescue;    /* rescue < 0: off */
    unsigned long long* ikey;              /* per read: the item key (MAP_NO_KEY = unmapped) */
    uint32_t* n_conc;                      /* per pair */
    uint8_t* state;                        /* per pair: MAP_PAIR_* */
    uint32_t *anchors, *n_anchors;         /* rescue anchors: read index of the anchor mate, appended */
    const unsigned long long *rslot, *seq_off; /* rslot: per read (the rescued mate) d << 32 | j, ~0 = nothing */
};
struct MapPairRank { unsigned long long hi, lo; }; /* the pair order (d_A + d_B, s_A, r, j_A, j_B) as two words */
MAP_HD MapPairRank map_pair_rank(unsigned long long kA, unsigned long long kB) {
    MapPairRank x;
    x.hi = (unsigned long long)(MAP_KEY_D(kA) + MAP_KEY_D(kB)) << 27 | (unsigned long long)MAP_KEY_S(kA) << 26 | MAP_KEY_R(kA);
    x.lo = (unsigned long long)MAP_KEY_J(kA) << 32 | MAP_KEY_J(kB);
    return x;
}
MAP_HD bool map_rank_less(const MapPairRank& a, const MapPairRank& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

/* For each key kA of [f0, f1) (one mate's loci of one strand, (r, j) order), the keys kB of [g0, g1) (the other mate's loci of the
 * other strand) with the same r and j_B in [j_A + clo, j_A + chi], in (r, j_B) order: a window that only moves forward.  fn(kA, kB)
 * returns false to stop; then so does the walk (returns false). */
template <class Fn>
MAP_HD bool map_pair_walk(const unsigned long long* __restrict__ lkey, uint32_t f0, uint32_t f1, uint32_t g0, uint32_t g1, long long clo,
                          long long chi, Fn&& fn) {
    uint32_t lo = g0, hi = g0;
    for (uint32_t x = f0; x < f1; x++) {
        const unsigned long long kA = lkey[x];
        const long long r = (long long)MAP_KEY_R(kA), jlo = (long long)MAP_KEY_J(kA) + clo, jhi = (long long)MAP_KEY_J(kA) + chi;
        if (jhi < 1) continue; /* loci ends are >= 1 */
        const unsigned long long want_lo = (unsigned long long)r << 32 | (unsigned long long)(jlo < 0 ? 0 : jlo > 0xffffffffll ? 0xffffffffll : jlo);
        const unsigned long long want_hi = (unsigned long long)r << 32 | (unsigned long long)(jhi > 0xffffffffll ? 0xffffffffll : jhi);
        while (lo < g1 && MAP_KEY_RJ(lkey[lo]) < want_lo) lo++;
        if (hi < lo) hi = lo;
        while (hi < g1 && MAP_KEY_RJ(lkey[hi]) <= want_hi) hi++;
        for (uint32_t y = lo; y < hi; y++)
            if (!fn(kA, lkey[y])) return false;
    }
    return true;
}

/* The concordant combinations (kA, kB) of pair p, both halves in pair order within a d sum: s_A = 0 (A forward: j_B in
 * [j_A - m_A + min, j_A - m_A + max]), then s_A = 1 (B forward: j_B in [j_A + m_B - max, j_A + m_B - min]) */
template <class Fn>
MAP_HD void map_pair_walk_both(const MapPairArgs& a, long p, Fn&& fn) {
    const long A = p, B = a.np + p;
    const long long mA = (long long)(a.roff[A + 1] - a.roff[A]), mB = (long long)(a.roff[B + 1] - a.roff[B]);
    const uint32_t a0 = a.lbase[A], a1 = a.lbase[A + 1], b0 = a.lbase[B], b1 = a.lbase[B + 1], as = a.lsplit[A], bs = a.lsplit[B];
    if (map_pair_walk(a.lkey, a0, as, bs, b1, a.min_insert - mA, a.max_insert - mA, fn))
        map_pair_walk(a.lkey, as, a1, b0, bs, mB - a.max_insert, mB - a.min_insert, fn);
}

/* The best concordant pair of pair p by pair order and cnt = n_concordant, the combinations with its d sum (saturating; 0: none).
 * Pair ranks are distinct (two combinations differ in a locus), so neither depends on the order in which the walk visits them. */
struct MapPairBest { unsigned long long kA, kB; uint32_t cnt; };
MAP_HD MapPairBest map_pair_best(const MapPairArgs& a, long p) {
    MapPairBest o = {MAP_NO_KEY, MAP_NO_KEY, 0u};
    MapPairRank best = {~0ull, ~0ull};
    map_pair_walk_both(a, p, [&](unsigned long long kA, unsigned long long kB) {
        const MapPairRank x = map_pair_rank(kA, kB);
        const unsigned long long sum = x.hi >> 27, bsum = best.hi >> 27;
        if (sum < bsum) o.cnt = 1;
        else if (sum == bsum && o.cnt != 0xffffffffu) o.cnt++;
        if (map_rank_less(x, best)) best = x, o.kA = kA, o.kB = kB;
        return true;
    });
    return o;
}

/* the partner of read x and the window of ends [jlo, jhi] (local to the anchor's sequence, clipped to [1, len_r]) in which it is
 * searched on strand 1 - s_X; false when the window is empty */
MAP_HD bool map_rescue_window(const MapPairArgs& a, uint32_t x, uint32_t& b, uint32_t& mb, long long& jlo, long long& jhi) {
    b = x < (uint32_t)a.np ? x + (uint32_t)a.np : x - (uint32_t)a.np;
    const uint32_t mx = a.roff[x + 1] - a.roff[x];
    mb = a.roff[b + 1] - a.roff[b];
    const unsigned long long k = a.ikey[x];
    const uint32_t r = MAP_KEY_R(k);
    const long long j = (long long)MAP_KEY_J(k), len_r = (long long)(a.seq_off[r + 1] - a.seq_off[r]);
    if (!MAP_KEY_S(k)) jlo = j - mx + a.min_insert, jhi = j - mx + a.max_insert;
    else jlo = j + mb - a.max_insert, jhi = j + mb - a.min_insert;
    jlo = jlo < 1 ? 1 : jlo, jhi = jhi > len_r ? len_r : jhi;
    return jlo <= jhi;
}

/* Tile `tile` (MAP_RESCUE_TILE ends) of anchor x's window: a semi-global pass of the partner q_b that starts mb + rescue columns before
 * the tile, so that D is exact wherever D <= rescue.  True when an end has D <= rescue and D < mb; slot = D << 32 | j of the smallest. */
template <int W>
MAP_HD bool map_rescue_tile(const MapPairArgs& a, const char* reads, const char* text, uint32_t x, uint32_t tile, uint32_t& b,
                            unsigned long long& slot) {
    uint32_t mb;
    long long jlo, jhi;
    if (!map_rescue_window(a, x, b, mb, jlo, jhi)) return false;
    const long long tlo = jlo + (long long)tile * MAP_RESCUE_TILE;
    if (tlo > jhi) return false;
    const long long thi = tlo + MAP_RESCUE_TILE - 1 < jhi ? tlo + MAP_RESCUE_TILE - 1 : jhi;
    const unsigned long long k = a.ikey[x];
    const long long c0 = tlo - (long long)mb - a.rescue; /* first text column (0-based): the smallest start that can reach D <= rescue */
    long long best_j = 0;
    const int best = map_best_end<W, long long>(reads + a.roff[b], mb, 1u - MAP_KEY_S(k), text + a.seq_off[MAP_KEY_R(k)], c0 < 0 ? 0 : c0, thi, tlo, a.rescue + 1, best_j);
    slot = (unsigned long long)best << 32 | (uint32_t)best_j;
    return best <= a.rescue && best < (int)mb;
}

/* Pair p in MAP_PAIR_RESCUE: the rescued pair of each anchor (anchor X, rescued locus Y = (d, 1 - s_X, r_X, j)), the one smaller in
 * pair order wins.  Returns the read of the rescued mate and its item key, -1 when neither anchor found its partner. */
MAP_HD long map_rescue_pick(const MapPairArgs& a, long p, unsigned long long& key) {
    const long A = p, B = a.np + p;
    const unsigned long long kA = a.ikey[A], kB = a.ikey[B];
    MapPairRank best = {~0ull, ~0ull};
    long who = -1;
    key = MAP_NO_KEY;
    for (int x = 0; x < 2; x++) {
        const long Y = x ? A : B; /* the rescued mate; the anchor is the other one */
        const unsigned long long kX = x ? kB : kA, slot = a.rslot[Y];
        if (kX == MAP_NO_KEY || slot == ~0ull) continue;
        const unsigned long long kY = map_pack_key((int)(slot >> 32), 1u - MAP_KEY_S(kX), MAP_KEY_R(kX), (uint32_t)slot);
        const MapPairRank rk = x ? map_pair_rank(kY, kX) : map_pair_rank(kX, kY);
        if (map_rank_less(rk, best)) best = rk, key = kY, who = Y;
    }
    return who;
}

/* Secondary pairs: the eligible pairs of pair p are its concordant combinations with d_A + d_B <= lim; within a d sum pair order is
 * map_pair_walk_both's order.  cnt = how many (saturating), mask = bit s set when one of them has d sum s (s <= 30). */
MAP_HD void map_pair_count(const MapPairArgs& a, long p, int lim, uint32_t& cnt, uint32_t& mask) {
    cnt = 0, mask = 0;
    map_pair_walk_both(a, p, [&](unsigned long long kA, unsigned long long kB) {
        const int s = MAP_KEY_D(kA) + MAP_KEY_D(kB);
        if (s <= lim) {
            if (cnt != 0xffffffffu) cnt++;
            mask |= 1u << s;
        }
        return true;
    });
}
/* fn(k, kA, kB) for the first `want` eligible pairs in pair order, k = 0, 1, ...: the sums of `mask` ascending, one walk per sum */
template <class Fn>
MAP_HD void map_pair_ranked(const MapPairArgs& a, long p, uint32_t mask, uint32_t want, Fn&& fn) {
    uint32_t k = 0;
    while (mask && k < want) {
        const int s = __builtin_ctz(mask);
        mask &= mask - 1u;
        map_pair_walk_both(a, p, [&](unsigned long long kA, unsigned long long kB) {
            if (MAP_KEY_D(kA) + MAP_KEY_D(kB) != s) return true;
            fn(k, kA, kB);
            return ++k < want;
        });
    }
}

/* ---- mapping quality (docs/design/mapper.md, "Mapping quality") ----
 * MAP_MAPQ_REFERENCE: min(254, 60 + greedy_cost) of a mapped record; MAP_MAPQ_GAP: T(n, g) from what the exact search proves, the
 * number n of loci (pairs) that tie for the best and a lower bound g >= 1 on the edit gap to the nearest alternative.  An unmapped
 * record has 0 under both. */
#define MAP_MAPQ_REFERENCE 0
#define MAP_MAPQ_GAP 1
#define MAP_MAPQ_CAPPED 20u /* the most a read with skipped buckets, or a rescued mate, may claim: a gap of 1 */
MAP_HD int map_mapq_reference(bool mapped, int greedy_cost) { return !mapped ? 0 : greedy_cost + 60 < 254 ? greedy_cost + 60 : 254; }
MAP_HD uint32_t map_mapq_table(uint32_t n, int g) {
    if (n == 0u) return 0u;
    if (n == 1u) return g >= 3 ? 60u : g >= 1 ? 20u * (uint32_t)g : 0u;
    return n == 2u ? 3u : n <= 4u ? 1u : 0u;
}
/* One read's loci folded: d1 = the smallest d (e + 1: no locus), n1 = the loci at d1, d2 = the smallest d > d1 (e + 1: none, the
 * search proves that nothing closer exists), best = the smallest locus key (MAP_NO_KEY: no locus), the best hit. */
struct MapMapqRead {
    int d1, d2;
    uint32_t n1;
    unsigned long long best;
};
MAP_HD MapMapqRead map_mapq_read(const unsigned long long* __restrict__ rkey, const uint32_t* __restrict__ rval, unsigned long long b,
                                 unsigned long long e_, const unsigned long long* __restrict__ seq_off, uint32_t n_seqs, int e) {
    MapMapqRead o = {e + 1, e + 1, 0u, MAP_NO_KEY};
    map_walk_loci(rkey, rval, b, e_, seq_off, n_seqs, [&](uint32_t s, uint32_t r, int d, uint32_t j) {
        const unsigned long long key = map_locus_key(seq_off, s, r, d, j);
        o.best = key < o.best ? key : o.best;
        if (d < o.d1) o.d2 = o.d1, o.d1 = d, o.n1 = 1u;
        else if (d == o.d1) o.n1++;
        else if (d < o.d2) o.d2 = d;
    });
    return o;
}
/* Q_read of a folded read with the per-read flags fl; 0 without a locus */
MAP_HD uint32_t map_mapq_read_q(const MapMapqRead& x, uint32_t fl) {
    const uint32_t q = map_mapq_table(x.n1, x.d2 - x.d1);
    return (fl & MAP_F_SEED_CAPPED) && q > MAP_MAPQ_CAPPED ? MAP_MAPQ_CAPPED : q;
}
/* Q_locus: the single-end value of a record at the locus `key` of a read with (d1, Q_read) */
MAP_HD uint32_t map_mapq_locus(unsigned long long key, int d1, uint32_t q_read) {
    return key != MAP_NO_KEY && MAP_KEY_D(key) == d1 ? q_read : 0u;
}
/* One pair's concordant combinations folded: S1 = the best d sum, N1 = the combinations with it (saturating, n_concordant; 0: none),
 * S2 = the smallest d sum > S1 (-1: none) */
struct MapMapqPair {
    int S1, S2;
    uint32_t N1;
};
MAP_HD MapMapqPair map_mapq_pair(const MapPairArgs& a, long p) {
    MapMapqPair o = {-1, -1, 0u};
    map_pair_walk_both(a, p, [&](unsigned long long kA, unsigned long long kB) {
        const int s = MAP_KEY_D(kA) + MAP_KEY_D(kB);
        if (o.N1 == 0u || s < o.S1) o.S2 = o.S1, o.S1 = s, o.N1 = 1u;
        else if (s == o.S1) o.N1 += o.N1 != 0xffffffffu;
        else if (o.S2 < 0 || s < o.S2) o.S2 = s;
        return true;
    });
    return o;
}
/* Q_pair of a folded pair whose best pair's mates lie at d_A and d_B; fl: both mates' per-read flags or-ed.  The second term of
 * g bounds every pair that uses a locus the search did not see: it lies beyond e, the mate it replaces within max(d_A, d_B). */
MAP_HD uint32_t map_mapq_pair_q(const MapMapqPair& x, int dA, int dB, int e, uint32_t fl) {
    int g = e + 1 - (dA > dB ? dA : dB);
    if (x.S2 >= 0 && x.S2 - x.S1 < g) g = x.S2 - x.S1;
    const uint32_t q = map_mapq_table(x.N1, g);
    return (fl & MAP_F_SEED_CAPPED) && q > MAP_MAPQ_CAPPED ? MAP_MAPQ_CAPPED : q;
}
/* The two records of a pair in state st whose items lie at kA and kB: qA, qB.  rq, rd1: each mate's Q_read and d1; q_pair: of the
 * pair (read only when CONCORDANT). */
MAP_HD void map_mapq_pair_records(uint32_t st, unsigned long long kA, unsigned long long kB, uint32_t rqA, uint32_t rqB, int d1A, int d1B,
                                  uint32_t q_pair, uint32_t& qA, uint32_t& qB) {
    qA = map_mapq_locus(kA, d1A, rqA), qB = map_mapq_locus(kB, d1B, rqB); /* no proper pair: each mate its single-end value */
    if (st == MAP_PAIR_CONCORDANT) {
        qA = qA > q_pair ? qA : q_pair, qB = qB > q_pair ? qB : q_pair;
    } else if (st == MAP_PAIR_RESCUED1) { /* the anchor (mate 2) keeps its value; the rescued mate: no gap above 1 */
        qA = qB < MAP_MAPQ_CAPPED ? qB : MAP_MAPQ_CAPPED;
    } else if (st == MAP_PAIR_RESCUED2) {
        qB = qA < MAP_MAPQ_CAPPED ? qA : MAP_MAPQ_CAPPED;
    }
}
/* A secondary pair's two records (items kA, kB of a pair whose best d sum is S1): a pair that ties for the best is treated as the
 * best one, one with a larger sum gets 0 */
MAP_HD void map_mapq_secondary(unsigned long long kA, unsigned long long kB, int S1, uint32_t rqA, uint32_t rqB, int d1A, int d1B,
                               uint32_t q_pair, uint32_t& qA, uint32_t& qB) {
    qA = qB = 0u;
    if (MAP_KEY_D(kA) + MAP_KEY_D(kB) == S1) map_mapq_pair_records(MAP_PAIR_CONCORDANT, kA, kB, rqA, rqB, d1A, d1B, q_pair, qA, qB);
}

/* Banded DP of q_s against tx[0, n): rows a = 0..m (read), columns b = 0..n, lanes l <-> diagonal b - a = l - MAP_MAX_ERRORS, only
 * the diagonals within d; dirs[a]: 2 bits per lane, 0 diagonal, 1 up (I), 2 left (D); ties prefer diagonal, then I, then D. */
MAP_HD void map_band_fill(const char* q, uint32_t m, uint32_t s, const char* tx, int n, int d, uint64_t* dirs) {
    const int INF = 2 * MAP_MAX_ERRORS + 2;
    int row[MAP_BAND];
    uint32_t tw[MAP_BAND]; /* code of text column b = a + delta (1-based: tx[b - 1]); 5 = outside */
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
                /* tw[l] holds the code of tx[b - 1] at this row (set on the previous row's shift) */
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
            left = row[l] = v; /* row[l + 1] (read above as `up`) is still the previous row's value */
        }
        dirs[ar] = dw;
        /* next row: column of lane l moves one to the right */
#pragma unroll
        for (int l = 0; l < MAP_BAND - 1; l++) tw[l] = tw[l + 1];
        const int bn = ar + 1 + (MAP_BAND - 1 - MAP_MAX_ERRORS); /* column of the last lane on the next row */
        tw[MAP_BAND - 1] = (bn >= 1 && bn <= n) ? map_code((uint8_t)tx[bn - 1]) : 5u;
    }
}

/* Traceback from (m, n) over dirs, twice: count the runs, then write the first min(runs, cap) of them forward into ops as
 * len << 3 | op (0 M, 1 I, 2 D).  Returns the number of runs. */
MAP_HD int map_traceback(const uint64_t* dirs, uint32_t m, int n, uint16_t* ops, int cap) {
    int runs = 0;
    for (int pass = 0; pass < 2; pass++) {
        int ar = (int)m, l = n - (int)m + MAP_MAX_ERRORS, k = 0;
        uint32_t op = 7u, len = 0;
        auto close_run = [&] { /* the traceback meets the runs last to first */
            if (pass == 1 && runs - 1 - k < cap) ops[runs - 1 - k] = (uint16_t)(len << 3 | op);
            k++;
        };
        while (ar > 0 || l != MAP_MAX_ERRORS) {
            const uint32_t dir = (uint32_t)(dirs[ar] >> (2 * l)) & 3u;
            const uint32_t o = dir == 0u ? 0u : dir == 1u ? 1u : 2u; /* M, I, D */
            if (o != op && len) close_run(), len = 0;
            op = o, len++;
            if (dir == 0u) ar--;
            else if (dir == 1u) ar--, l++;
            else l--;
        }
        if (len) close_run();
        runs = k;
    }
    return runs;
}

/* One item: the read q (m bytes, flags fl) at the locus `key`, or unmapped (MAP_NO_KEY).  Writes its CIGAR row (cap entries at
 * ops; dirs: m + 1 words of scratch) and returns its record; nops = the CIGAR's runs (255 at most), whatever cap is. */
template <int W>
MAP_HD MapHit map_finish_item(const char* q, uint32_t m, unsigned long long key, uint32_t fl, const char* text,
                              const unsigned long long* seq_off, uint64_t* dirs, uint16_t* ops, int cap, uint8_t& nops) {
    MapHit h = MAP_HIT_UNMAPPED;
    int runs = 0;
    if (key != MAP_NO_KEY) {
        const int d = MAP_KEY_D(key);
        const uint32_t s = MAP_KEY_S(key), r = MAP_KEY_R(key), j = MAP_KEY_J(key);
        const char* tx = text + seq_off[r];
        const uint32_t start = map_find_start<W>(q, m, s, tx, j, d);
        const int n = (int)(j - start);
        map_band_fill(q, m, s, tx + start, n, d, dirs);
        runs = map_traceback(dirs, m, n, ops, cap);
        if (runs > cap) fl |= MAP_F_CIGAR_TRUNCATED;
        h.seq_id = (int32_t)r, h.pos = start, h.end = j, h.dist = (int16_t)d, h.strand = (uint8_t)s;
        fl |= MAP_F_MAPPED;
    }
    nops = (uint8_t)(runs > 255 ? 255 : runs); /* one store: nops is the item's slot in global memory */
    h.flags = (uint8_t)fl;
    return h;
}
