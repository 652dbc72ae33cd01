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
// Mapping quality (ASM_MAPQ_GAP only): map_mapq_kernel folds each read's sorted run records into (d1, n1, d2), its MAPQ bytes and,
//          for the best-hit calls, its best key (they take the run path then, not the atomicMin); map_pair_mapq_kernel folds each
//          pair's concordant combinations and writes both records' bytes; map_pair_item_mapq_kernel does the secondary pairs.
// MD tag (the file calls under ASM_SAM_TAG_MD only): map_md_kernel writes every finished item's MD:Z row (the rule: asm_md.h) next
//          to its record, from the item's CIGAR row, its read and the text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "asm_bits.h"
#include "asm_map_core.h"
#include "asm_md.h"

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
        uint32_t key = none, acc;
        const uint32_t r = map_seq_of(seq_off, n_seqs, t);
        const bool inside = t + (unsigned long long)k <= seq_off[r + 1]; /* the k-mer lies inside one sequence */
        if (inside && map_kmer_key([&](uint32_t q) { return (uint8_t)text[t + q]; }, (uint32_t)k, (uint32_t)k, acc)) key = acc;
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

__global__ __launch_bounds__(256) void map_seed_count_kernel(MapSeedArgs a, unsigned long long* __restrict__ cnt,
                                                             uint32_t* __restrict__ flags) {
    const long nw = a.n * a.S * a.P;
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (long)gridDim.x * blockDim.x) {
        MapPiece pc;
        unsigned long long c = 0;
        if (map_piece(a, w, pc)) {
            c = a.ix_off[pc.key + 1] - a.ix_off[pc.key];
            if (a.max_occ > 0 && c > (unsigned long long)a.max_occ) {
                c = 0;
                atomicOr(flags + pc.read, MAP_F_SEED_CAPPED);
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
        MapPiece pc;
        map_piece(a, w, pc);
        const unsigned long long qlo = b < c0 ? c0 - b : 0ull, qhi = b + c > c1 ? c1 - b : c;
        const uint32_t first = a.ix_off[pc.key];
        for (unsigned long long q = qlo; q < qhi; q++) cand[b + q - c0] = map_candidate(a, pc, a.ix_pos[first + q]);
    }
}

/* thread per candidate: the window's best (d, end) and the read's atomicMin over the packed key (end local to sequence r) */
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
        uint32_t best_t = 0;
        const int best = map_best_end<W, uint32_t>(reads + r0, m, s, text, x.ws, x.we, 0u, e + 1, best_t);
        if (best <= e) atomicMin(keys + x.read, map_pack_key(best, s, r, best_t - (uint32_t)seq_off[r]));
    }
}

/* ---- all hits (asm_map_reads_all): a window reports each maximal interval of ends with D_w <= e as a run record ----
 * a slot in the run buffer for each active lane: one atomicAdd per wave (lanes of a wave close intervals at the same column) */
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
    if (slot < cap) map_run_pack(read, s, lo, hi, dmin, jmin, rkey[slot], rval[slot]);
}

/* thread per candidate: the window's run records appended to the run buffer instead of its best folded into an atomicMin */
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
        map_scan_runs<W>(reads + r0, m, s, text, x.ws, x.we, e, [&](uint32_t lo, uint32_t hi, int dmin, uint32_t jmin) {
            map_put_run(counter, cap, rkey, rval, x.read, s, lo, hi, dmin, jmin);
        });
    }
}

struct MapSelectArgs {
    const unsigned long long* rkey; /* the run records, sorted */
    const uint32_t* rval;
    unsigned long long nr;
    long n;                          /* reads */
    int e, strata, max_hits;
    const unsigned long long* seq_off;
    uint32_t n_seqs;
    const uint32_t* roff;
    uint32_t *n_hits, *d_best;       /* per read: loci with d <= min(e, d_best + strata); d_best (count pass), 0 when n_hits = 0 */
    const uint32_t* ibase;           /* per read: first item (emit pass) */
    const unsigned long long* dbase; /* per read: dirs offset of its first item (emit pass) */
    uint32_t* iread;                 /* per item */
    unsigned long long *ikey, *idirs; /* per item: its packed locus key (MAP_NO_KEY = unmapped) and its dirs offset */
};

/* thread per read: d_best and n_hits of its loci */
__global__ __launch_bounds__(256) void map_select_count_kernel(MapSelectArgs a) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        const MapRange g = map_read_runs(a.rkey, a.nr, i);
        int best = a.e + 1;
        map_walk_loci(a.rkey, a.rval, g.b, g.e, a.seq_off, a.n_seqs, [&](uint32_t, uint32_t, int d, uint32_t) { best = d < best ? d : best; });
        const int lim = best + a.strata < a.e ? best + a.strata : a.e;
        uint32_t cnt = 0;
        if (best <= a.e)
            map_walk_loci(a.rkey, a.rval, g.b, g.e, a.seq_off, a.n_seqs, [&](uint32_t, uint32_t, int d, uint32_t) { cnt += d <= lim; });
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
        const MapRange g = map_read_runs(a.rkey, a.nr, i);
        uint32_t k = 0;
        for (int lvl = (int)a.d_best[i]; lvl <= a.e && k < want; lvl++)
            map_walk_loci(a.rkey, a.rval, g.b, g.e, a.seq_off, a.n_seqs, [&](uint32_t s, uint32_t r, int d, uint32_t j) {
                if (d != lvl || k >= want) return;
                a.iread[q0 + k] = (uint32_t)i;
                a.ikey[q0 + k] = map_locus_key(a.seq_off, s, r, d, j);
                a.idirs[q0 + k] = db + (unsigned long long)k * (m + 1u);
                k++;
            });
    }
}

/* ---- paired-end reads (asm_map_pairs): the pairing picks one item per read, so the finish runs on the identity list ----
 * thread per read: its loci keys into lkey[lbase[i], ...) in walk order (n_hits of map_select_count_kernel with strata = e), the
 * first index of its s = 1 part into lsplit[i], and its smallest key (the best hit; MAP_NO_KEY without loci) into lbest[i] */
__global__ __launch_bounds__(256) void map_loci_emit_kernel(MapSelectArgs a, const uint32_t* __restrict__ lbase,
                                                            unsigned long long* __restrict__ lkey, uint32_t* __restrict__ lsplit,
                                                            unsigned long long* __restrict__ lbest) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        const MapRange g = map_read_runs(a.rkey, a.nr, i);
        uint32_t k = lbase[i], split = 0xffffffffu;
        unsigned long long best = MAP_NO_KEY;
        map_walk_loci(a.rkey, a.rval, g.b, g.e, a.seq_off, a.n_seqs, [&](uint32_t s, uint32_t r, int d, uint32_t j) {
            const unsigned long long key = map_locus_key(a.seq_off, s, r, d, j);
            if (s && split == 0xffffffffu) split = k;
            best = key < best ? key : best;
            lkey[k++] = key;
        });
        lsplit[i] = split == 0xffffffffu ? k : split;
        lbest[i] = best;
    }
}

/* thread per pair: the best concordant pair by pair order and n_concordant (the pairs with its d sum), else each mate's best hit
 * (its smallest key) and, with rescue on, each mapped mate as a rescue anchor */
__global__ __launch_bounds__(256) void map_pair_kernel(MapPairArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.np; p += (long)gridDim.x * blockDim.x) {
        const long A = p, B = a.np + p;
        const MapPairBest o = map_pair_best(a, p);
        a.n_conc[p] = o.cnt;
        if (o.cnt) {
            a.ikey[A] = o.kA, a.ikey[B] = o.kB, a.state[p] = (uint8_t)MAP_PAIR_CONCORDANT;
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

/* thread per (anchor, tile of MAP_RESCUE_TILE ends): the tile's smallest (D, j) is folded into rslot[partner] with a 64-bit
 * atomicMin.  Every anchor has ntile tiles; the anchor count is read on the device. */
template <int W>
__global__ __launch_bounds__(256) void map_rescue_kernel(MapPairArgs a, const char* __restrict__ reads, const char* __restrict__ text,
                                                         uint32_t ntile, unsigned long long* __restrict__ rslot) {
    const unsigned long long nt = (unsigned long long)*a.n_anchors * ntile;
    for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < nt;
         g += (unsigned long long)gridDim.x * blockDim.x) {
        uint32_t b;
        unsigned long long slot;
        if (map_rescue_tile<W>(a, reads, text, a.anchors[g / ntile], (uint32_t)(g % ntile), b, slot)) atomicMin(rslot + b, slot);
    }
}

/* thread per pair in MAP_PAIR_RESCUE: the rescued mate's item key is written, or the pair falls back to MAP_PAIR_NONE */
__global__ __launch_bounds__(256) void map_rescue_pick_kernel(MapPairArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.np; p += (long)gridDim.x * blockDim.x) {
        if (a.state[p] != MAP_PAIR_RESCUE) continue;
        unsigned long long key;
        const long who = map_rescue_pick(a, p, key);
        if (who >= 0) a.ikey[who] = key;
        a.state[p] = (uint8_t)(who < 0 ? MAP_PAIR_NONE : who == p ? MAP_PAIR_RESCUED1 : MAP_PAIR_RESCUED2);
    }
}

/* ---- secondary pairs (asm_map_pairs_all) ---- */
struct MapPairAllArgs {
    MapPairArgs pa;                   /* the pairing's loci lists, item keys and states */
    int strata, max_pairs;
    uint32_t *n_pairs, *sums;         /* per pair: eligible pairs (uncapped, saturating); bit s set when one has d sum s (s <= 30) */
    unsigned long long* nitem;        /* np + 1: secondary items per pair, 2 (min(n_pairs, max_pairs) - 1) */
    unsigned long long* ndirs;        /* np + 1: their dirs words, (m_A + 1) + (m_B + 1) per secondary pair */
    const unsigned long long *ibase, *dbase; /* np: exclusive scans of nitem and of ndirs */
    uint32_t* iread;                  /* per secondary item: its read */
    unsigned long long *ikey, *idirs; /* per secondary item: its locus key and its dirs offset */
};

/* thread per pair: n_pairs, the d sums that occur among the eligible pairs and the secondary items' sizes (0 unless CONCORDANT;
 * sum_best is the d sum of the pair map_pair_kernel reported) */
__global__ __launch_bounds__(256) void map_pair_count_kernel(MapPairAllArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.pa.np; p += (long)gridDim.x * blockDim.x) {
        uint32_t cnt = 0, mask = 0;
        unsigned long long ni = 0, nd = 0;
        if (a.pa.state[p] == MAP_PAIR_CONCORDANT) {
            const long A = p, B = a.pa.np + p;
            map_pair_count(a.pa, p, MAP_KEY_D(a.pa.ikey[A]) + MAP_KEY_D(a.pa.ikey[B]) + a.strata, cnt, mask);
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
        map_pair_ranked(a.pa, p, a.sums[p], want, [&](uint32_t k, unsigned long long kA, unsigned long long kB) {
            if (!k) return;
            a.iread[q] = (uint32_t)A, a.ikey[q] = kA, a.idirs[q] = dw;
            a.iread[q + 1] = (uint32_t)B, a.ikey[q + 1] = kB, a.idirs[q + 1] = dw + mA + 1u;
            q += 2, dw += mA + mB + 2u;
        });
    }
}

/* ---- mapping quality under MAP_MAPQ_GAP (the rules: asm_map_core.h) ---- */
struct MapMapqArgs {
    const unsigned long long* rkey; /* the run records, sorted */
    const uint32_t* rval;
    unsigned long long nr;
    long n;                          /* reads */
    int e;
    const unsigned long long* seq_off;
    uint32_t n_seqs;
    const uint32_t* flags;           /* per read */
    uint8_t *rq, *rd1;               /* per read: Q_read and d1 (e + 1: no locus) */
    unsigned long long* best;        /* per read: its best hit's key (the best-hit calls); NULL: not wanted */
    const uint32_t* ibase;           /* all hits: first item of every read (n + 1); NULL: no items */
    const unsigned long long* ikey;  /* all hits: per item, its locus key */
    uint8_t* mapq;                   /* all hits: per item */
};

/* thread per read: its run records (contiguous after the sort) folded into (d1, n1, d2); Q_read, d1 and, where wanted, the best
 * hit's key and the MAPQ of the read's items */
__global__ __launch_bounds__(256) void map_mapq_kernel(MapMapqArgs a) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        const MapRange g = map_read_runs(a.rkey, a.nr, i);
        const MapMapqRead x = map_mapq_read(a.rkey, a.rval, g.b, g.e, a.seq_off, a.n_seqs, a.e);
        const uint32_t q = map_mapq_read_q(x, a.flags[i]);
        a.rq[i] = (uint8_t)q, a.rd1[i] = (uint8_t)x.d1;
        if (a.best) a.best[i] = x.best;
        if (a.ibase)
            for (uint32_t it = a.ibase[i]; it < a.ibase[i + 1]; it++) a.mapq[it] = (uint8_t)map_mapq_locus(a.ikey[it], x.d1, q);
    }
}

struct MapPairMapqArgs {
    MapPairArgs pa;          /* the pairing's loci lists, item keys and final states */
    int e;
    const uint32_t* flags;   /* per read */
    const uint8_t *rq, *rd1; /* per read (map_mapq_kernel) */
    uint8_t* mapq;           /* per read: the MAPQ of its record in the pair's answer */
    uint8_t *pq, *ps1;       /* per pair: Q_pair and S1 (CONCORDANT pairs; else 0), for the secondary pairs */
    /* map_pair_item_mapq_kernel: the secondary items, two per pair (mate 1, mate 2) */
    long ni;
    const uint32_t* iread;
    const unsigned long long* ikey;
    uint8_t* imapq;
};

/* thread per pair: its concordant combinations folded into (S1, N1, S2), then both records' MAPQ by the pair's state */
__global__ __launch_bounds__(256) void map_pair_mapq_kernel(MapPairMapqArgs a) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.pa.np; p += (long)gridDim.x * blockDim.x) {
        const long A = p, B = a.pa.np + p;
        const uint32_t st = a.pa.state[p];
        const unsigned long long kA = a.pa.ikey[A], kB = a.pa.ikey[B];
        uint32_t q_pair = 0u, qA, qB;
        int S1 = 0;
        if (st == MAP_PAIR_CONCORDANT) {
            const MapMapqPair x = map_mapq_pair(a.pa, p);
            q_pair = map_mapq_pair_q(x, MAP_KEY_D(kA), MAP_KEY_D(kB), a.e, a.flags[A] | a.flags[B]);
            S1 = x.S1;
        }
        map_mapq_pair_records(st, kA, kB, a.rq[A], a.rq[B], (int)a.rd1[A], (int)a.rd1[B], q_pair, qA, qB);
        a.mapq[A] = (uint8_t)qA, a.mapq[B] = (uint8_t)qB;
        a.pq[p] = (uint8_t)q_pair, a.ps1[p] = (uint8_t)S1;
    }
}

/* thread per secondary pair (items 2 t and 2 t + 1: its mates 1 and 2) */
__global__ __launch_bounds__(256) void map_pair_item_mapq_kernel(MapPairMapqArgs a) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; 2 * t < a.ni; t += (long)gridDim.x * blockDim.x) {
        const long A = (long)a.iread[2 * t], B = (long)a.iread[2 * t + 1], p = A;
        uint32_t qA, qB;
        map_mapq_secondary(a.ikey[2 * t], a.ikey[2 * t + 1], (int)a.ps1[p], a.rq[A], a.rq[B], (int)a.rd1[A], (int)a.rd1[B], a.pq[p], qA, qB);
        a.imapq[2 * t] = (uint8_t)qA, a.imapq[2 * t + 1] = (uint8_t)qB;
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
    uint64_t* dirs;                     /* (m + 1) words per item */
    MapHit* hits;                       /* per item */
    uint16_t* ops;                      /* [n items][cap] */
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
        uint32_t fl = a.flags[i];
        if (m < (uint32_t)(a.P * a.k)) fl |= MAP_F_TOO_SHORT;
        uint64_t* dirs = a.dirs + (ITEMS ? a.idirs[it] : (unsigned long long)(r0 + (uint32_t)i));
        a.hits[it] = map_finish_item<W>(a.reads + r0, m, a.keys[it], fl, a.text, a.seq_off, dirs, a.ops + it * a.cap, a.cap, a.nops[it]);
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

/* ---- the MD:Z tag (the rule and the 78-byte bound: asm_md.h) ---- */
static_assert(MD_MAX_EDITS == MAP_MAX_ERRORS && MAP_MAX_READ <= 999, "the bound on an MD tag rests on the mapper's limits");
struct MapMdArgs {
    const char* reads;               /* upper-cased, concatenated */
    const uint32_t* roff;
    long n;                          /* items */
    const uint32_t* iread;           /* per item, its read; NULL: item i is read i */
    const MapHit* hits;              /* per item */
    const uint16_t* ops;             /* [n][cap] */
    const uint8_t* nops;
    int cap;
    const char* text;
    const unsigned long long* seq_off;
    char* md;                        /* [n][MD_ROW_CAP] */
    uint8_t* md_len;                 /* per item; 0: unmapped, or more than cap operations (the line's CIGAR is '*') */
};

/* thread per finished item: the row is written straight into the item's slot (byte stores, at most 78 of them; no private copy),
 * then its length.  The sink is bounded by the row, and a row that does not consume its read and window exactly, which the finish
 * kernel never writes, gets length 0. */
__global__ __launch_bounds__(256) void map_md_kernel(MapMdArgs a) {
    const long it = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= a.n) return;
    const MapHit h = a.hits[it];
    const uint32_t nops = a.nops[it];
    uint32_t len = 0;
    if ((h.flags & MAP_F_MAPPED) && nops <= (uint32_t)a.cap) {
        const long i = a.iread ? (long)a.iread[it] : it;
        const uint32_t r0 = a.roff[i], m = a.roff[i + 1] - r0, s = h.strand;
        const char* q = a.reads + r0;
        MdRowSink o{a.md + (size_t)it * MD_ROW_CAP, (uint32_t)MD_ROW_CAP};
        const char* w = a.text + a.seq_off[h.seq_id] + h.pos;
        const bool ok = md_format(a.ops + (size_t)it * a.cap, nops, [&](uint32_t p) { return map_read_byte(q, m, s, p); }, m,
                                  [&](uint32_t p) { return w[p]; }, h.end - h.pos, o);
        if (ok && o.cur <= (uint32_t)MD_ROW_CAP) len = o.cur;
    }
    a.md_len[it] = (uint8_t)len;
}
