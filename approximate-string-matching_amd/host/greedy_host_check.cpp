// Host build of the general Greedy step (csrc/asm_greedy_lane.h on csrc/asm_bits.h) for the CPU test-suite.  The functions the
// thin kernels call are driven serially, pair by pair, in the three shapes of the five kernels:
//   shape 0 (a)  one loop over all lanes, serial arg-max (greedy_beats), serial fold: greedy_wide_kernel's replays, and the structure of
//                greedy_persist_kernel (which spells its step out and is not executed here)
//   shape 1 (b)  per-lane values computed independently, arg-max as maxima over the key words and the tie key inside each 64 lanes and
//                the two-wave meet, the wave kernel's early-outs, candidate mask, ordered fold over the mask; lane vectors on four
//                words and the scan with fall-backs where the band fits one wave: greedy_wave2_kernel, and the structure of
//                greedy_wave_kernel (which, like the persist kernel, spells its step out and is not executed here)
//   shape 2 (c)  the band cut into T slices of LPT lanes, select-form refresh, per-slice best, keys with 127 - lane, the fold by lowest
//                remaining lane: greedy_group_kernel
// each through the real CigarSink, so that tests/test_greedy_lane_host.py can diff cost and CIGAR with the oracle without a GPU.  Built as
// a library for the tests and, with GREEDY_HOST_CHECK_MAIN, as a stand-alone program, which the same tests build under ASan + UBSan.
// Test support only: nothing in the product links this file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../csrc/asm_greedy_lane.h"

namespace {
constexpr int MAX_STEPS = 4 * 128; /* hurdle_matrix.h:358-361 */

struct Pair {
    uint4 a0, a1, b0, b1; /* the planes as the kernels load them */
    V128 A0, A1, B0, B1;
    uint32_t ln;
    // views: A[128], B[128] as the conversion sees them (bit_convert.cpp:340-355: exactly 'C','G','T' set bits)
    void load(const unsigned char* view, uint32_t lens) {
        uint32_t w[4][4] = {};
        for (int s = 0; s < 2; s++)
            for (int q = 0; q < 128; q++) {
                const unsigned char c = view[s * 128 + q];
                const int code = c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0;
                if (code & 1) w[2 * s][q >> 5] |= 1u << (q & 31);
                if (code & 2) w[2 * s + 1][q >> 5] |= 1u << (q & 31);
            }
        a0 = make_uint4(w[0][0], w[0][1], w[0][2], w[0][3]), a1 = make_uint4(w[1][0], w[1][1], w[1][2], w[1][3]);
        b0 = make_uint4(w[2][0], w[2][1], w[2][2], w[2][3]), b1 = make_uint4(w[3][0], w[3][1], w[3][2], w[3][3]);
        A0 = v_from_uint4(a0), A1 = v_from_uint4(a1), B0 = v_from_uint4(b0), B1 = v_from_uint4(b1);
        ln = lens;
    }
    V128 lane_vector(int lane) const { return greedy_lane_vector(A0, A1, B0, B1, lane); }
};

struct Run {
    GreedyArgs args;
    GreedyCosts pen;
    CigarSink cig;
    int k;
};

// ---- shape (a): thread per pair / workgroup per pair with serial replays ----
int shape_serial(const Pair& P, const Run& R, long pair) {
    const int k = R.k, nl = 2 * k + 1;
    const GreedyCosts pen = R.pen;
    std::vector<V128> lo(nl), lf(nl);
    std::vector<int> sp(nl, -1), len(nl, 0), nsw(nl, 128), dst(nl), sw(nl), nh(nl);
    int m, nn, dest_lane;
    greedy_lengths(P.ln, m, nn, dest_lane);
    for (int j = 0; j < nl; j++) {
        lo[j] = P.lane_vector(j - k);
        lf[j] = v_flip_short_hurdles1(lo[j]);
        dst[j] = lane_destination(m, nn, j - k);
    }
    const V128 dest_vec = P.lane_vector(dest_lane);
    int cur_lane = 0, cur_col = 0, cost = 0, guard = 0, ncig = 0;
    for (;;) {
        bool reaching = false;
        for (int j = 0; j < nl; j++) {
            const int lane = j - k;
            const int start_col = greedy_start_col(cur_lane, cur_col, lane);
            if (sp[j] < start_col) {
                int fz, nx;
                v_highway_from(lf[j], start_col, fz, nx);
                if (greedy_refresh(greedy_highway_at(start_col, fz, nx, dst[j]), cur_lane, lane, sp[j], len[j], nsw[j])) reaching = true;
            }
            sw[j] = greedy_switch_cost(pen.semi && guard == 0, cur_lane, lane, pen.o, pen.e);
            nh[j] = greedy_hurdles(lo[j], start_col, sp[j], len[j]);
        }
        double best_h = -__builtin_inf();
        int best_leap = 0, bj = k; /* the reference's default best lane is lane 0 */
        for (int j = 0; j < nl; j++) {
            double heur;
            int leap;
            greedy_score(R.args, pen, reaching, j - k, dest_lane, dst[j], sp[j], len[j], nsw[j], sw[j], nh[j], heur, leap);
            if (greedy_beats(heur, leap, best_h, best_leap)) best_h = heur, best_leap = leap, bj = j;
        }
        if (len[bj] <= 0 || ++guard > MAX_STEPS) break;
        const int best = bj - k, best_sp = sp[bj], best_cost = pen.x * nh[bj] + sw[bj];
        const int best_from_sp = v_ones_from(lo[bj], best_sp);
        int small_total = best_cost, small_inter = best_cost, cj = bj;
        for (int j = 0; j < nl; j++)
            if (greedy_cand_reachable(j - k, best, fwd_col(j - k, best), sp[j], best_sp)) {
                const int inter = greedy_cand_inter(sw[j], nh[j]);
                const int total = greedy_cand_total(pen, j - k, best, fwd_col(j - k, best), sp[j], len[j], inter, lo[bj], best_sp, best_from_sp);
                if (greedy_fold_accept(total, inter, small_total, small_inter)) cj = j;
            }
        if (greedy_commit(R.cig, true, pair, ncig, m, nn, cj - k, sp[cj] + len[cj], sw[cj] + pen.x * nh[cj], cur_lane, cur_col, cost)) break;
    }
    greedy_final_hop(pen, R.cig, true, pair, ncig, m, nn, dest_lane, [&]() { return dest_vec; }, cur_lane, cur_col, cost);
    if (R.cig.on()) R.cig.finish(pair, ncig);
    return cost;
}

// ---- shape (b): thread = band lane, one or two waves ----
int shape_wave(const Pair& P, const Run& R, long pair) {
    const int k = R.k, nl = 2 * k + 1, waves = (nl + 63) / 64, nt = 64 * waves;
    const GreedyCosts pen = R.pen;
    const bool one_wave = waves == 1; /* greedy_wave_kernel: lane vectors on words, scan with fall-backs, early-outs */
    std::vector<V128> lo(nt), lf(nt), nlf(nt);
    std::vector<unsigned> fb_lf(nt), fb_nlf(nt), khi(nt), klo(nt);
    std::vector<int> sp(nt, -1), len(nt, 0), nsw(nt, 128), dst(nt), sw(nt), nh(nt), leap(nt), inter(nt), total(nt);
    std::vector<char> cand(nt), may(nt);
    int m, nn, dest_lane;
    greedy_lengths(P.ln, m, nn, dest_lane);
    for (int t = 0; t < nt; t++) {
        const bool active = t < nl;
        const int lane = t - k;
        if (one_wave) {
            const bool neg = lane < 0;
            greedy_lane_words(P.a0, P.a1, P.b0, P.b1, neg, (uint32_t)(active ? (neg ? -lane : lane) : 0), lo[t], lf[t]);
        } else {
            lo[t] = P.lane_vector(lane);
            lf[t] = v_flip_short_hurdles1(lo[t]);
        }
        nlf[t] = v_not(lf[t]);
        fb_lf[t] = v_upper_fallback(lf[t]), fb_nlf[t] = v_upper_fallback(nlf[t]);
        dst[t] = lane_destination(m, nn, lane);
    }
    int cur_lane = 0, cur_col = 0, cost = 0, ncig = 0;
    for (int guard = 0; guard < MAX_STEPS; guard++) {
        bool reaching = false;
        for (int t = 0; t < nt; t++) {
            const int lane = t - k;
            sw[t] = nh[t] = 0;
            if (t >= nl) continue;
            const int start_col = greedy_start_col(cur_lane, cur_col, lane);
            if (sp[t] < start_col) {
                int fz, nx;
                if (one_wave)
                    v_highway_from_fb(lf[t], nlf[t], fb_lf[t], fb_nlf[t], start_col, fz, nx);
                else
                    v_highway_from(lf[t], start_col, fz, nx);
                if (greedy_refresh(greedy_highway_at(start_col, fz, nx, dst[t]), cur_lane, lane, sp[t], len[t], nsw[t])) reaching = true;
            }
            sw[t] = greedy_switch_cost(pen.semi && guard == 0, cur_lane, lane, pen.o, pen.e);
            nh[t] = greedy_hurdles(lo[t], start_col, sp[t], len[t]);
        }
        for (int t = 0; t < nt; t++) { /* every thread scores, band lane or not; the keys of the others are 0 */
            double heur;
            greedy_score(R.args, pen, reaching, t - k, dest_lane, dst[t], sp[t], len[t], nsw[t], sw[t], nh[t], heur, leap[t]);
            greedy_score_key_words(heur, khi[t], klo[t]);
            if (t >= nl) khi[t] = 0u;
        }
        // each wave's winner by three maxima, then the meet of the waves (ties: the lower lane)
        int bt = -1;
        unsigned long long bkey = 0;
        for (int w = 0; w < waves; w++) {
            unsigned mhi = 0, mlo = 0, m3 = 0;
            for (int t = 64 * w; t < 64 * w + 64; t++) mhi = khi[t] > mhi ? khi[t] : mhi;
            for (int t = 64 * w; t < 64 * w + 64; t++) cand[t] = t < nl && khi[t] == mhi;
            for (int t = 64 * w; t < 64 * w + 64; t++) mlo = cand[t] && klo[t] > mlo ? klo[t] : mlo;
            for (int t = 64 * w; t < 64 * w + 64; t++) cand[t] = cand[t] && klo[t] == mlo;
            for (int t = 64 * w; t < 64 * w + 64; t++) {
                const unsigned k3 = cand[t] ? greedy_tie_key<6>(leap[t], t & 63) : 0u;
                m3 = k3 > m3 ? k3 : m3;
            }
            const int wt = 64 * w + greedy_tie_key_slot<6>(m3);
            const unsigned long long key = wt < nl ? ((unsigned long long)khi[wt] << 32) | klo[wt] : 0ull;
            if (bt < 0 || key > bkey || (key == bkey && leap[wt] > leap[bt])) bt = wt, bkey = key;
        }
        const int best = bt - k, best_sp = sp[bt], best_cost = sw[bt] + pen.x * nh[bt];
        if (len[bt] <= 0) break;
        int ct = bt;
        // the wave kernel's early-outs: nobody can be accepted when the best lane costs nothing; no tail counts when no lane passes the
        // tests that need nothing of the best lane's vector
        if (best_cost > 0 || pen.o <= 0 || (pen.semi && guard == 0)) {
            bool any = false;
            for (int t = 0; t < nt; t++) {
                may[t] = t < nl && greedy_cand_reachable(t - k, best, fwd_col(t - k, best), sp[t], best_sp) && greedy_cand_inter(sw[t], nh[t]) <= best_cost;
                any = any || may[t];
            }
            if (any) {
                const V128 best_vec = lo[bt];
                const int best_from_sp = v_ones_from(best_vec, best_sp);
                int small_total = best_cost, small_inter = best_cost;
                for (int t = 0; t < nt; t++) {
                    inter[t] = total[t] = 0x3fffffff;
                    if (may[t]) {
                        inter[t] = greedy_cand_inter(sw[t], nh[t]);
                        total[t] = greedy_cand_total(pen, t - k, best, fwd_col(t - k, best), sp[t], len[t], inter[t], best_vec, best_sp, best_from_sp);
                    }
                }
                for (int t = 0; t < nt; t++) /* the candidate mask, folded in lane order */
                    if (total[t] <= best_cost && inter[t] <= best_cost && greedy_fold_accept(total[t], inter[t], small_total, small_inter)) ct = t;
            }
        }
        if (greedy_commit(R.cig, true, pair, ncig, m, nn, ct - k, sp[ct] + len[ct], sw[ct] + pen.x * nh[ct], cur_lane, cur_col, cost)) break;
    }
    const auto dest_vec = [&]() { /* out of the lane that holds it, or rebuilt when the destination lies outside the band */
        const int dt = dest_lane + k;
        return dt >= 0 && dt < nl ? lo[dt] : P.lane_vector(dest_lane);
    };
    greedy_final_hop(pen, R.cig, true, pair, ncig, m, nn, dest_lane, dest_vec, cur_lane, cur_col, cost);
    if (R.cig.on()) R.cig.finish(pair, ncig);
    return cost;
}

// ---- shape (c): T threads per pair, LPT consecutive lanes each ----
int shape_group(const Pair& P, const Run& R, int T, int LPT, long pair) {
    const int k = R.k, nl = 2 * k + 1, ns = T * LPT;
    const GreedyCosts pen = R.pen;
    std::vector<V128> lo(ns);
    std::vector<int> sp(ns, -1), len(ns, 0), nsw(ns, 128), sw(ns), nh(ns), ti(ns);
    std::vector<int> bq(T), bleap(T);
    std::vector<unsigned long long> bkey(T);
    std::vector<unsigned> cmask(T);
    int m, nn, dest_lane;
    greedy_lengths(P.ln, m, nn, dest_lane);
    for (int j = 0; j < ns; j++) lo[j] = P.lane_vector(j - k); /* slots beyond the band compute on what the shift leaves */
    int cur_lane = 0, cur_col = 0, cost = 0, ncig = 0;
    bool done = false;
    for (int guard = 0; guard < MAX_STEPS && !done; guard++) {
        bool reaching = false;
        const bool first_free = pen.semi && guard == 0;
        for (int j = 0; j < ns; j++) { /* pass 1, select form */
            const int lane = j - k;
            const int start_col = greedy_start_col(cur_lane, cur_col, lane);
            const bool stale = sp[j] < start_col;
            int fz, nx;
            v_highway_from(v_flip_short_hurdles1(lo[j]), start_col, fz, nx);
            const GreedyHighway h = greedy_highway_at(start_col, fz, nx, lane_destination(m, nn, lane));
            sp[j] = stale ? h.sp : sp[j];
            len[j] = stale ? h.len : len[j];
            nsw[j] = stale ? greedy_lane_distance(lane, cur_lane) : nsw[j];
            reaching = reaching || (stale && h.reach && j < nl);
            sw[j] = greedy_switch_cost(first_free, cur_lane, lane, pen.o, pen.e);
            nh[j] = greedy_hurdles(lo[j], start_col, sp[j], len[j]);
        }
        for (int r = 0; r < T; r++) { /* pass 2: the slice's own best lane */
            double bheur = -__builtin_inf();
            bleap[r] = -(1 << 20), bq[r] = -1;
            for (int q = 0; q < LPT; q++) {
                const int j = r * LPT + q;
                double heur;
                int leap;
                greedy_score(R.args, pen, reaching, j - k, dest_lane, lane_destination(m, nn, j - k), sp[j], len[j], nsw[j], sw[j], nh[j], heur, leap);
                if (j < nl && (bq[r] < 0 || greedy_beats(heur, leap, bheur, bleap[r]))) bheur = heur, bleap[r] = leap, bq[r] = q;
            }
            bkey[r] = bq[r] >= 0 ? greedy_score_key(bheur) : 0ull;
            bq[r] = bq[r] < 0 ? 0 : bq[r];
        }
        unsigned mhi = 0, mlo = 0, m3 = 0;
        for (int r = 0; r < T; r++) mhi = (unsigned)(bkey[r] >> 32) > mhi ? (unsigned)(bkey[r] >> 32) : mhi;
        for (int r = 0; r < T; r++)
            if ((unsigned)(bkey[r] >> 32) == mhi && (unsigned)bkey[r] > mlo) mlo = (unsigned)bkey[r];
        for (int r = 0; r < T; r++) {
            const bool cand = (unsigned)(bkey[r] >> 32) == mhi && (unsigned)bkey[r] == mlo && bkey[r] != 0ull;
            const unsigned k3 = cand ? greedy_tie_key<7>(bleap[r], r * LPT + bq[r]) : 0u;
            m3 = k3 > m3 ? k3 : m3;
        }
        const int bj = greedy_tie_key_slot<7>(m3), best = bj - k, owner = bj / LPT;
        const int oj = owner * LPT + bq[owner]; /* the owner's best lane IS the winner */
        const int best_sp = sp[oj], best_len = len[oj], best_cost = sw[oj] + pen.x * nh[oj];
        if (best_len <= 0) break;
        const V128 best_vec = lo[oj];
        const int best_from_sp = v_ones_from(best_vec, best_sp);
        for (int r = 0; r < T; r++) {
            cmask[r] = 0u;
            for (int q = 0; q < LPT; q++) {
                const int j = r * LPT + q, lane = j - k;
                const int fb = fwd_col(lane, best);
                const int inter = greedy_cand_inter(sw[j], nh[j]);
                const int total = greedy_cand_total(pen, lane, best, fb, sp[j], len[j], inter, best_vec, best_sp, best_from_sp);
                const bool can = j < nl && greedy_cand_reachable(lane, best, fb, sp[j], best_sp) && total <= best_cost && inter <= best_cost;
                ti[j] = (int)(((unsigned)total << 16) | ((unsigned)inter & 0xffffu));
                cmask[r] |= can ? 1u << q : 0u;
            }
        }
        int small_total = best_cost, small_inter = best_cost, ch = bj;
        for (;;) { /* the lowest remaining candidate lane of the group, until none is left */
            unsigned top = 0;
            for (int r = 0; r < T; r++) {
                const unsigned mine = cmask[r] ? (unsigned)(127 - (r * LPT + __builtin_ctz(cmask[r]))) : 0u;
                top = mine > top ? mine : top;
            }
            if (top == 0u) break;
            const int cj = 127 - (int)top;
            if (greedy_fold_accept(ti[cj] >> 16, ti[cj] & 0xffff, small_total, small_inter)) ch = cj;
            cmask[cj / LPT] &= cmask[cj / LPT] - 1u;
        }
        done = greedy_commit(R.cig, true, pair, ncig, m, nn, ch - k, sp[ch] + len[ch], sw[ch] + pen.x * nh[ch], cur_lane, cur_col, cost);
    }
    greedy_final_hop(pen, R.cig, true, pair, ncig, m, nn, dest_lane, [&]() { return P.lane_vector(dest_lane); }, cur_lane, cur_col, cost);
    if (R.cig.on()) R.cig.finish(pair, ncig);
    return cost;
}
}  // namespace

// views: n x (A[128], B[128]) as the conversion sees them; lens: m | n << 16; shape 0 / 1 / 2 as above ((T, LPT) for shape 2 only);
// ops: n rows of cap entries (count << 3 | op), nops: entries produced per pair.  0, or a negative number for arguments out of range.
extern "C" int greedy_host_batch(long n, const unsigned char* views, const uint32_t* lens, int shape, int T, int LPT, int k, int x, int o, int e,
                                 int semi, const double* probs, int32_t* costs, uint16_t* ops, int cap, uint8_t* nops) {
    if (k < 1 || k > 50 || shape < 0 || shape > 2) return -1;
    if (shape == 2 && !((T == 2 || T == 4 || T == 8 || T == 16) && LPT >= 1 && LPT <= 8 && T * LPT >= 2 * k + 1)) return -2;
    Run R;
    R.args = GreedyArgs{x, o, e, semi, log(probs[0] / 0.25), log(probs[1] / 0.25), log(probs[2] / 2 / 0.25)}; /* hurdle_matrix.h:536-538 */
    R.pen = GreedyCosts{x, o, e, semi != 0};
    R.cig = CigarSink{ops, nops, cap};
    R.k = k;
    for (long i = 0; i < n; i++) {
        Pair P;
        P.load(views + i * 256, lens[i]);
        costs[i] = shape == 0 ? shape_serial(P, R, i) : shape == 1 ? shape_wave(P, R, i) : shape_group(P, R, T, LPT, i);
    }
    return 0;
}

// The wave kernel's lane vectors on four words against greedy_lane_vector and v_flip_short_hurdles1, every lane -31..31 of every pair:
// the number of vectors that differ
extern "C" long greedy_host_lane_words(long n, const unsigned char* views) {
    long bad = 0;
    for (long i = 0; i < n; i++) {
        Pair P;
        P.load(views + i * 256, 0u);
        for (int lane = -31; lane <= 31; lane++) {
            V128 lo, lf;
            greedy_lane_words(P.a0, P.a1, P.b0, P.b1, lane < 0, (uint32_t)(lane < 0 ? -lane : lane), lo, lf);
            const V128 want = P.lane_vector(lane), want_f = v_flip_short_hurdles1(want);
            bad += !(lo.lo == want.lo && lo.hi == want.hi && lf.lo == want_f.lo && lf.hi == want_f.hi);
        }
    }
    return bad;
}

#ifdef GREEDY_HOST_CHECK_MAIN
// Stand-alone form (the one a sanitizer build takes): greedy_host_check BATCH k x o e semi T LPT [cap].  BATCH holds int32 n, uint32 lens[n]
// and the n x 256 view bytes, read into arrays of exactly that size; the CIGAR rows are n x cap entries on the heap, exactly (cap: 255
// unless given), so a store past a full row is a sanitizer report.  Prints per pair the cost and the CIGAR of each shape (shape (c) only
// where T * LPT covers the band; a truncated row as its stored entries and "+<entries missing>"), then the count of greedy_host_lane_words.
int main(int argc, char** argv) {
    if (argc != 9 && argc != 10) return fprintf(stderr, "usage: %s batch k x o e semi T LPT [cap]\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || fread(&n, sizeof n, 1, f) != 1 || n < 0) return fprintf(stderr, "%s: cannot read\n", argv[1]), 2;
    std::vector<uint32_t> lens((size_t)n);
    std::vector<unsigned char> views((size_t)n * 256);
    if (fread(lens.data(), 4, lens.size(), f) != lens.size() || fread(views.data(), 1, views.size(), f) != views.size()) return 2;
    fclose(f);
    const int k = atoi(argv[2]), x = atoi(argv[3]), o = atoi(argv[4]), e = atoi(argv[5]), semi = atoi(argv[6]), T = atoi(argv[7]), LPT = atoi(argv[8]);
    const double probs[3] = {0.80, 0.20 / 3, 0.40 / 3};
    const int cap = argc == 10 ? atoi(argv[9]) : 255, shapes = T * LPT >= 2 * k + 1 ? 3 : 2;
    if (cap < 1) return fprintf(stderr, "cap must be at least 1\n"), 2;
    std::vector<std::string> lines((size_t)n);
    for (int shape = 0; shape < shapes; shape++) {
        std::vector<int32_t> costs((size_t)n);
        std::vector<uint16_t> ops((size_t)n * cap);
        std::vector<uint8_t> nops((size_t)n);
        if (greedy_host_batch(n, views.data(), lens.data(), shape, T, LPT, k, x, o, e, semi, probs, costs.data(), ops.data(), cap, nops.data())) return 3;
        for (int32_t i = 0; i < n; i++) {
            std::string& s = lines[i];
            s += (shape ? " " : "") + std::to_string(costs[i]) + " ";
            if (nops[i] == 0) s += "*";
            for (int q = 0; q < nops[i] && q < cap; q++) s += std::to_string(ops[(size_t)i * cap + q] >> 3) + "MID"[ops[(size_t)i * cap + q] & 7];
            if (nops[i] > cap) s += "+" + std::to_string(nops[i] - cap); /* a truncated row: its stored entries, then how many are missing */
        }
    }
    for (int32_t i = 0; i < n; i++) printf("%s\n", lines[i].c_str());
    printf("lane words differing: %ld\n", greedy_host_lane_words(n, views.data()));
    return 0;
}
#endif
