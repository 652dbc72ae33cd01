// Host build of the read mapper's per-thread core (csrc/asm_map_core.h), for the CPU test-suite (tests/test_map_core_host.py):
// plain g++, run under ASan + UBSan.  A serial mirror of the pipeline of csrc/asm_map.h and nothing else: what a kernel does per
// thread is a `for` loop here, what hipcub does (sort, scan) is std::stable_sort and a running sum, what an atomic does is std::min.
// Every buffer has exactly the size the device gives it (dirs: m + 1 words, a CIGAR row: cap entries), so that an index past its
// end is a sanitizer report.  The index is a sorted (key, position) vector and a bucket is an equal_range of it.
// Two small host-visible decisions are this file's own copy of the kernel's text, not shared code, so the tests pin the core under
// them and not these lines: the fall-back of map_pair_kernel (each mate's best hit, MAP_PAIR_RESCUE or MAP_PAIR_NONE, the anchor
// list) and the state map_rescue_pick_kernel writes after map_rescue_pick.
//
// Input argv[1] (little endian): u32 n_seqs, each {u32 len, bytes}; u32 n_cases, each {u32 k, e, both_strands, paired; i32
// min_insert, max_insert, rescue_errors; u32 cigar_cap, pair_cap, n_reads, each {u32 len, bytes}}.  A paired case holds the mates 1
// of its n_reads / 2 pairs, then the mates 2.  The width W of a case is that of its longest read, as map_with_width picks it.
// Output argv[2], per case: per read {i32 seq_id, u32 pos, end, i32 dist, u32 strand, flags, nops, u16 ops[min(nops, cap)]} (the
// best hit; in a paired case the pairing's item), then per read {u32 n, each u64 locus key in (s, r, j) order}, then, paired, per
// pair {u32 state, n_concordant, u64 item key of A and of B, u32 n_pairs, u32 listed = min(n_pairs, pair_cap), each u64 kA, kB}.
// With a third argument `--mapq` (tests/test_mapq_host.py) every case goes on with the mapping-quality folds (map_mapq_kernel,
// map_pair_mapq_kernel): per read {u32 d1, n1, d2, Q_read}, then, paired, per pair {i32 S1, u32 N1, i32 S2, u32 Q_pair, MAPQ of
// the record of A and of B}.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/asm_map_core.h"

typedef unsigned long long u64;

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static void put(FILE* f, const void* p, size_t n) { if (n) fwrite(p, 1, n, f); }
static void put32(FILE* f, uint32_t v) { put(f, &v, 4); }

static bool get_strings(FILE* f, std::string& cat, std::vector<uint32_t>* off32, std::vector<u64>* off64) { /* upper-cased (map_upper_kernel) */
    uint32_t n = 0;
    if (!get(f, &n, 4)) return false;
    for (uint32_t i = 0; i <= n; i++) {
        if (off32) off32->push_back((uint32_t)cat.size());
        if (off64) off64->push_back(cat.size());
        uint32_t len = 0;
        if (i == n) break;
        if (!get(f, &len, 4)) return false;
        std::string s(len, '\0');
        if (!get(f, &s[0], len)) return false;
        for (char& c : s) c = (c >= 'a' && c <= 'z') ? (char)(c - 32) : c;
        cat += s;
    }
    return true;
}

struct Case {
    uint32_t k, e, both, paired;
    int32_t min_insert, max_insert, rescue;
    uint32_t cap, pair_cap;
};

typedef std::vector<std::pair<uint32_t, uint32_t>> Index; /* (key, position), sorted by key */

/* the index: map_kmer_key_kernel, then the radix sort (stable: positions ascend inside a bucket) */
static Index build_index(const std::string& text, const std::vector<u64>& seq_off, uint32_t k) {
    Index ix;
    for (u64 t = 0; t < text.size(); t++) {
        uint32_t key;
        const uint32_t r = map_seq_of(seq_off.data(), (uint32_t)seq_off.size() - 1, t);
        if (t + k <= seq_off[r + 1] && map_kmer_key([&](uint32_t q) { return (uint8_t)text[t + q]; }, k, k, key)) ix.push_back({key, (uint32_t)t});
    }
    std::stable_sort(ix.begin(), ix.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    return ix;
}

template <int W>
static void run_case(const std::string& text, const std::vector<u64>& seq_off, const Index& ix, const Case& c, const std::string& reads,
                     const std::vector<uint32_t>& roff, FILE* out, bool mapq) {
    const long n = (long)roff.size() - 1;
    const uint32_t n_seqs = (uint32_t)seq_off.size() - 1;
    /* seeding and both verifications: map_seed_count / emit, map_verify_kernel (atomicMin), map_verify_all_kernel (run buffer) */
    const MapSeedArgs sa = {reads.data(), roff.data(), n,       c.both ? 2 : 1, (int)c.e + 1, (int)c.k, (int)c.e, 0,
                            text.data(),  nullptr,     nullptr, seq_off.data(), n_seqs};
    std::vector<u64> keys(n, MAP_NO_KEY);
    std::vector<std::pair<u64, uint32_t>> runs;
    for (long w = 0; w < n * sa.S * sa.P; w++) {
        MapPiece pc;
        if (!map_piece(sa, w, pc)) continue;
        auto lo = std::lower_bound(ix.begin(), ix.end(), std::make_pair(pc.key, 0u));
        for (; lo != ix.end() && lo->first == pc.key; ++lo) {
            const MapCand x = map_candidate(sa, pc, lo->second);
            if (x.read == MAP_BAD_CAND) continue;
            const char* q = reads.data() + pc.r0;
            uint32_t best_t = 0;
            const int best = map_best_end<W, uint32_t>(q, pc.m, pc.s, text.data(), x.ws, x.we, 0u, (int)c.e + 1, best_t);
            if (best <= (int)c.e)
                keys[x.read] = std::min(keys[x.read], map_pack_key(best, pc.s, x.rs >> 1, best_t - (uint32_t)seq_off[x.rs >> 1]));
            map_scan_runs<W>(q, pc.m, pc.s, text.data(), x.ws, x.we, (int)c.e, [&](uint32_t rlo, uint32_t rhi, int dmin, uint32_t jmin) {
                runs.push_back({0, 0});
                map_run_pack(x.read, pc.s, rlo, rhi, dmin, jmin, runs.back().first, runs.back().second);
            });
        }
    }
    std::stable_sort(runs.begin(), runs.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    std::vector<u64> rkey(runs.size());
    std::vector<uint32_t> rval(runs.size());
    for (size_t t = 0; t < runs.size(); t++) rkey[t] = runs[t].first, rval[t] = runs[t].second;
    /* loci lists: map_loci_emit_kernel */
    std::vector<uint32_t> lbase(n + 1, 0), lsplit(n);
    std::vector<u64> lkey, lbest(n, MAP_NO_KEY);
    for (long i = 0; i < n; i++) {
        const MapRange g = map_read_runs(rkey.data(), rkey.size(), i);
        uint32_t split = 0xffffffffu;
        map_walk_loci(rkey.data(), rval.data(), g.b, g.e, seq_off.data(), n_seqs, [&](uint32_t s, uint32_t r, int d, uint32_t j) {
            const u64 key = map_locus_key(seq_off.data(), s, r, d, j);
            if (s && split == 0xffffffffu) split = (uint32_t)lkey.size();
            lbest[i] = std::min(lbest[i], key);
            lkey.push_back(key);
        });
        lbase[i + 1] = (uint32_t)lkey.size();
        lsplit[i] = split == 0xffffffffu ? lbase[i + 1] : split;
    }
    /* pairing: map_pair_kernel, map_rescue_kernel (atomicMin per partner), map_rescue_pick_kernel */
    const long np = c.paired ? n / 2 : 0;
    std::vector<u64> ikey(keys), rslot(n, ~0ull);
    std::vector<uint32_t> n_conc(np, 0), anchors;
    std::vector<uint8_t> state(np, 0);
    MapPairArgs pa = {np, roff.data(), lbase.data(), lsplit.data(), lbest.data(), lkey.data(), c.min_insert, c.max_insert, c.rescue,
                      ikey.data(), n_conc.data(), state.data(), nullptr, nullptr, rslot.data(), seq_off.data()};
    for (long p = 0; p < np; p++) {
        const long A = p, B = np + p;
        const MapPairBest o = map_pair_best(pa, p);
        n_conc[p] = o.cnt;
        if (o.cnt) {
            ikey[A] = o.kA, ikey[B] = o.kB, state[p] = (uint8_t)MAP_PAIR_CONCORDANT;
            continue;
        }
        ikey[A] = lbest[A], ikey[B] = lbest[B];
        const bool resc = c.rescue >= 0 && (lbest[A] != MAP_NO_KEY || lbest[B] != MAP_NO_KEY);
        state[p] = (uint8_t)(resc ? MAP_PAIR_RESCUE : MAP_PAIR_NONE);
        if (resc && lbest[A] != MAP_NO_KEY) anchors.push_back((uint32_t)A);
        if (resc && lbest[B] != MAP_NO_KEY) anchors.push_back((uint32_t)B);
    }
    const uint32_t ntile = (uint32_t)((c.max_insert - c.min_insert + MAP_RESCUE_TILE) / MAP_RESCUE_TILE);
    for (u64 g = 0; c.paired && g < (u64)anchors.size() * ntile; g++) {
        uint32_t b;
        u64 slot;
        if (map_rescue_tile<W>(pa, reads.data(), text.data(), anchors[g / ntile], (uint32_t)(g % ntile), b, slot))
            rslot[b] = std::min(rslot[b], slot);
    }
    for (long p = 0; p < np; p++) {
        if (state[p] != MAP_PAIR_RESCUE) continue;
        u64 key;
        const long who = map_rescue_pick(pa, p, key);
        if (who >= 0) ikey[who] = key;
        state[p] = (uint8_t)(who < 0 ? MAP_PAIR_NONE : who == p ? MAP_PAIR_RESCUED1 : MAP_PAIR_RESCUED2);
    }
    /* finish: map_finish_kernel on the identity list */
    for (long i = 0; i < n; i++) {
        const uint32_t m = roff[i + 1] - roff[i];
        std::vector<uint64_t> dirs(m + 1);
        std::vector<uint16_t> ops(c.cap);
        uint8_t nops;
        const MapHit h = map_finish_item<W>(reads.data() + roff[i], m, ikey[i], m < (c.e + 1) * c.k ? MAP_F_TOO_SHORT : 0u, text.data(),
                                            seq_off.data(), dirs.data(), ops.data(), (int)c.cap, nops);
        const uint32_t rec[7] = {(uint32_t)h.seq_id, h.pos, h.end, (uint32_t)(int32_t)h.dist, h.strand, h.flags, nops};
        put(out, rec, sizeof rec);
        put(out, ops.data(), 2 * std::min<size_t>(nops, c.cap));
    }
    for (long i = 0; i < n; i++) {
        put32(out, lbase[i + 1] - lbase[i]);
        put(out, lkey.data() + lbase[i], 8 * (size_t)(lbase[i + 1] - lbase[i]));
    }
    /* secondary pairs: map_pair_count_kernel, map_pair_emit_kernel (here rank 0 is listed too) */
    for (long p = 0; p < np; p++) {
        uint32_t cnt = 0, mask = 0;
        std::vector<u64> list;
        if (state[p] == MAP_PAIR_CONCORDANT) {
            map_pair_count(pa, p, 2 * (int)c.e, cnt, mask); /* every concordant combination of loci within e */
            map_pair_ranked(pa, p, mask, std::min(cnt, c.pair_cap), [&](uint32_t, u64 kA, u64 kB) { list.push_back(kA), list.push_back(kB); });
        }
        put32(out, state[p]), put32(out, n_conc[p]);
        put(out, &ikey[p], 8), put(out, &ikey[np + p], 8);
        put32(out, cnt), put32(out, (uint32_t)(list.size() / 2));
        put(out, list.data(), 8 * list.size());
    }
    if (!mapq) return;
    /* mapping quality: map_mapq_kernel per read, map_pair_mapq_kernel per pair (no bucket cap here, so no read is SEED_CAPPED) */
    std::vector<uint32_t> rq(n);
    std::vector<int> rd1(n);
    for (long i = 0; i < n; i++) {
        const MapRange g = map_read_runs(rkey.data(), rkey.size(), i);
        const MapMapqRead x = map_mapq_read(rkey.data(), rval.data(), g.b, g.e, seq_off.data(), n_seqs, (int)c.e);
        rq[i] = map_mapq_read_q(x, 0u), rd1[i] = x.d1;
        if (x.best != lbest[i]) rq[i] = 0xffffffffu; /* the fold's best key is the loci list's */
        put32(out, (uint32_t)x.d1), put32(out, x.n1), put32(out, (uint32_t)x.d2), put32(out, rq[i]);
    }
    for (long p = 0; p < np; p++) {
        const long A = p, B = np + p;
        MapMapqPair x = {-1, -1, 0u};
        uint32_t q_pair = 0, qA, qB;
        if (state[p] == MAP_PAIR_CONCORDANT) {
            x = map_mapq_pair(pa, p);
            q_pair = map_mapq_pair_q(x, MAP_KEY_D(ikey[A]), MAP_KEY_D(ikey[B]), (int)c.e, 0u);
        }
        map_mapq_pair_records(state[p], ikey[A], ikey[B], rq[A], rq[B], rd1[A], rd1[B], q_pair, qA, qB);
        put32(out, (uint32_t)x.S1), put32(out, x.N1), put32(out, (uint32_t)x.S2), put32(out, q_pair), put32(out, qA), put32(out, qB);
    }
}

int main(int argc, char** argv) {
    const bool mapq = argc == 4 && strcmp(argv[3], "--mapq") == 0;
    if (argc != 3 && !mapq) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::string text;
    std::vector<u64> seq_off;
    uint32_t ncases = 0;
    std::map<uint32_t, Index> index; /* per k */
    if (!get_strings(in, text, nullptr, &seq_off) || !get(in, &ncases, 4)) return 3;
    for (uint32_t t = 0; t < ncases; t++) {
        Case c;
        std::string reads;
        std::vector<uint32_t> roff;
        if (!get(in, &c, sizeof c) || !get_strings(in, reads, &roff, nullptr)) return 3;
        uint32_t maxm = 0;
        for (size_t i = 0; i + 1 < roff.size(); i++) maxm = std::max(maxm, roff[i + 1] - roff[i]);
        if (maxm > MAP_MAX_READ || c.e > MAP_MAX_ERRORS) return 3;
        const int nw = (int)(maxm + 63) / 64;
        if (!index.count(c.k)) index[c.k] = build_index(text, seq_off, c.k);
        const Index& ix = index[c.k];
        if (nw <= 1) run_case<1>(text, seq_off, ix, c, reads, roff, out, mapq);
        else if (nw <= 2) run_case<2>(text, seq_off, ix, c, reads, roff, out, mapq);
        else if (nw <= 4) run_case<4>(text, seq_off, ix, c, reads, roff, out, mapq);
        else run_case<8>(text, seq_off, ix, c, reads, roff, out, mapq);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
