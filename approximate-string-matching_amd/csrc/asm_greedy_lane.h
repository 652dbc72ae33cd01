// The step of the general ("FP64") Greedy hurdle-matrix aligner, rule by rule: what greedy_wave2_kernel (asm_wave.h),
// greedy_group_kernel (asm_group.h) and greedy_wide_kernel (asm_wide.h) run per band lane.  Those kernels differ in how band lanes map to
// threads and in how a pair's threads agree (serial replays from LDS, DPP reductions over a wave or inside T lanes, LDS and barriers);
// everything else is here.  greedy_persist_kernel (asm_kernels.h) and greedy_wave_kernel (asm_wave.h) call those of these functions that
// leave their instruction streams unchanged and hold the rest of the same step written out: see the notes at those kernels.
//
// Follows hurdle_matrix<int_128bit>: _construct_hurdles (hurdle_matrix.h:441-455), _update_highway_list (:285-362),
// _choose_best_highway (:368-401), _step (:407-434), run (:568-597).  The per-lane cache {starting_point, length, num_switches}
// persists across steps exactly as highway_info does (:26-44, reset :106-119).
//
// Small force-inlined functions over scalars and V128, so that a kernel which keeps its lanes in registers keeps them there.
// Builds for the host as well: host/greedy_host_check.cpp drives these functions serially in the three shapes the kernels use them in
// and tests/test_greedy_lane_host.py diffs the result with the oracle.
#pragma once
#include <stdint.h>

#include "asm_bits.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#include <string.h>
#endif

struct GreedyArgs {
    int x, o, e;
    int semi; /* SEMI_GLOBAL (hurdle_matrix.h:313-316,335-338,577-580): no switch cost into the first highway, into the
                 destination lane, or for the final hop */
    double sig_match, sig_mismatch, sig_indel; /* hurdle_matrix.h:536-538, computed on the host with libm */
};

// the penalties as a kernel holds them (compile-time constants in the UNIT instantiations)
struct GreedyCosts {
    int x, o, e;
    bool semi;
};

// hurdle_matrix.h:328-330.  With the default probabilities mismatch_sig == indel_sig bit for bit, so lanes that
// trade a hurdle for a lane switch tie up to rounding, and the rounding sequence decides the arg-max.  The
// reference built with its own flags (-O3 -march=native: GCC contracts a*b+c on FMA hardware) evaluates
// fma(indel, nsw, fma(mismatch, nh, match*len)); the same three roundings are issued here explicitly (the host build is compiled with
// -ffp-contract=off, so its plain multiply stays one).
ASM_HD double greedy_significance(const GreedyArgs& a, int len, int nh, int nsw) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fma_rn(a.sig_indel, (double)nsw, __fma_rn(a.sig_mismatch, (double)nh, __dmul_rn(a.sig_match, (double)len)));
#else
    return fma(a.sig_indel, (double)nsw, fma(a.sig_mismatch, (double)nh, a.sig_match * (double)len));
#endif
}

ASM_HD unsigned long long greedy_double_bits(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned long long)__double_as_longlong(v);
#else
    unsigned long long b;
    memcpy(&b, &v, sizeof b);
    return b;
#endif
}

// ---- _construct_hurdles (hurdle_matrix.h:441-455): lane < 0 compares A[i + |lane|] with B[i], lane >= 0 B[i + lane] with A[i] ----
ASM_HD V128 greedy_lane_vector(V128 A0, V128 A1, V128 B0, V128 B1, int lane) {
    const int s = lane < 0 ? -lane : lane;
    V128 m0, m1;
    if (lane < 0) {
        m0 = v_xor(v_toward0(A0, s), B0);
        m1 = v_xor(v_toward0(A1, s), B1);
    } else {
        m0 = v_xor(v_toward0(B0, s), A0);
        m1 = v_xor(v_toward0(B1, s), A1);
    }
    return v_or(m0, m1);
}

// The same vector and its flipped form (flip_short_hurdles(1), utils.h:200-216) on four 32-bit words, for a lane at most 31 positions
// off the main diagonal (sh = |lane| <= 31, neg = lane < 0): the 128-bit shift is four v_alignbit_b32, the flip's two shifts by one
// eight more.  = greedy_lane_vector and v_flip_short_hurdles1 of it.
ASM_HD uint4 w_toward0_small(uint4 v, uint32_t s /* 0..31 */) { /* utils.h:143-153 on four words, shift below 32 */
    return make_uint4(asm_alignbit(v.y, v.x, s), asm_alignbit(v.z, v.y, s), asm_alignbit(v.w, v.z, s), v.w >> s);
}
ASM_HD void greedy_lane_words(uint4 a0, uint4 a1, uint4 b0, uint4 b1, bool neg, uint32_t sh, V128& lo, V128& lf) {
    const uint4 xs0 = w_toward0_small(neg ? a0 : b0, sh), xs1 = w_toward0_small(neg ? a1 : b1, sh);
    const uint4 y0 = neg ? b0 : a0, y1 = neg ? b1 : a1;
    const uint4 mw = make_uint4((xs0.x ^ y0.x) | (xs1.x ^ y1.x), (xs0.y ^ y0.y) | (xs1.y ^ y1.y), (xs0.z ^ y0.z) | (xs1.z ^ y1.z),
                                (xs0.w ^ y0.w) | (xs1.w ^ y1.w));
    /* flip_short_hurdles(1): a hurdle survives only next to another one */
    const uint4 dn = w_toward0_small(mw, 1u);
    const uint4 up = make_uint4(mw.x << 1, asm_alignbit(mw.y, mw.x, 31u), asm_alignbit(mw.z, mw.y, 31u), asm_alignbit(mw.w, mw.z, 31u));
    lo = v_from_uint4(mw);
    lf = v_from_uint4(make_uint4(mw.x & (dn.x | up.x), mw.y & (dn.y | up.y), mw.z & (dn.z | up.z), mw.w & (dn.w | up.w)));
}

// the strings as the aligner sees them (cut at 128, hurdle_matrix.h:626-627) and the lane the alignment ends in (:649)
ASM_HD void greedy_lengths(uint32_t ln /* m | n << 16 */, int& m, int& nn, int& dest_lane) {
    m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
    m = m > 128 ? 128 : m;
    nn = nn > 128 ? 128 : nn;
    dest_lane = nn - m;
}

// ---- _update_highway_list (hurdle_matrix.h:285-362) ----
ASM_HD int greedy_start_col(int cur_lane, int cur_col, int lane) { return cur_col + fwd_col(cur_lane, lane); }
ASM_HD int greedy_lane_distance(int a, int b) {
    const int d = a - b;
    return d < 0 ? -d : d;
}

// The highway a scan from start_col found (fz zeros skipped, then nx ones: v_highway_from on the lane's flipped vector), cut where the
// lane ends (dst = lane_destination): its start, its length, and whether it reaches the destination (:299-312)
struct GreedyHighway {
    int sp, len;
    bool reach;
};
ASM_HD GreedyHighway greedy_highway_at(int start_col, int fz, int nx, int dst) {
    GreedyHighway h;
    h.sp = start_col + fz;
    h.len = nx;
    h.reach = false;
    if (start_col + fz + nx > dst) {
        const int c = dst - (start_col + fz);
        h.len = c > 0 ? c : 0;
        h.reach = true;
    }
    return h;
}
// ... written into a lane's cache, which is stale when it starts before start_col (the caller's test: a branch, or selects)
ASM_HD bool greedy_refresh(GreedyHighway h, int cur_lane, int lane, int& sp, int& len, int& nsw) {
    nsw = greedy_lane_distance(lane, cur_lane);
    sp = h.sp;
    len = h.len;
    return h.reach;
}

// cost of switching into `lane` (free for SEMI_GLOBAL's first step, :313-316) and the hurdles from start_col to the highway's end
ASM_HD int greedy_switch_cost(bool first_free, int cur_lane, int lane, int o, int e) { return first_free ? 0 : lane_penalty(cur_lane, lane, o, e); }
ASM_HD int greedy_hurdles(V128 lo, int start_col, int sp, int len) { return v_pop_between(lo, start_col, sp + len); }

// a lane's score (:328-343): the significance of its highway, or, once some lane reaches its destination, the integer cost of ending there
ASM_HD void greedy_score(const GreedyArgs& args, GreedyCosts c, bool reaching, int lane, int dest_lane, int dst, int sp, int len, int nsw,
                         int sw, int nh, double& heur, int& leap) {
    heur = greedy_significance(args, len, nh, nsw);
    leap = -sw;
    if (reaching) {
        const int fsw = c.semi ? 0 : lane_penalty(lane, dest_lane, c.o, c.e);
        heur = (double)(-sw - c.x * nh - fsw - c.x * (dst - sp - len));
        leap -= fsw;
    }
}

// arg-max rule (:345-351): larger score, then larger leap; scanning lanes in ascending order, the lower lane keeps an exact tie.
// The scan starts from (-inf, 0, lane 0): -numeric_limits<int>::infinity() == 0 (:287)
ASM_HD bool greedy_beats(double heur, int leap, double best_heur, int best_leap) {
    return heur > best_heur || (heur == best_heur && leap > best_leap);
}

// The same order as a maximum over integers: an order-preserving 64-bit key of the score (-0.0 -> +0.0 so that equal values have equal
// keys; key = hb < 0 ? ~hb : hb | 2^63) in two words — the lower one only matters where the upper ones tie —, then a third word of
// leap and the lane slot counted downwards, so that the lowest slot wins an exact tie.  A key of 0 is below every score's.
ASM_HD void greedy_score_key_words(double heur, unsigned& khi, unsigned& klo) {
    heur = heur + 0.0;
    const unsigned long long hb = greedy_double_bits(heur);
    const unsigned hhi = (unsigned)(hb >> 32);
    const unsigned sgn = (unsigned)((int)hhi >> 31); /* all ones for a negative score */
    khi = (hhi ^ sgn) | (~sgn & 0x80000000u);
    klo = (unsigned)hb ^ sgn;
}
ASM_HD unsigned long long greedy_score_key(double heur) {
    unsigned khi, klo;
    greedy_score_key_words(heur, khi, klo);
    return ((unsigned long long)khi << 32) | klo;
}
template <int SLOT_BITS>
ASM_HD unsigned greedy_tie_key(int leap, int slot) {
    return (((unsigned)(leap + 32768)) << SLOT_BITS) | (unsigned)(((1 << SLOT_BITS) - 1) - slot);
}
template <int SLOT_BITS>
ASM_HD int greedy_tie_key_slot(unsigned key) {
    return ((1 << SLOT_BITS) - 1) - (int)(key & (unsigned)((1 << SLOT_BITS) - 1));
}

// ---- _choose_best_highway (:368-401): a lane that reaches the best lane's highway more cheaply than the best lane does ----
// (fb = fwd_col(lane, best): the columns a switch from the lane into the best lane skips)
// the part that needs nothing of the best lane's vector (:376-377): another lane, whose highway does not start behind the best one's
ASM_HD bool greedy_cand_reachable(int lane, int best, int fb, int sp, int best_sp) { return lane != best && !(sp + fb > best_sp); }
// inter: cost up to the end of the lane's highway — the range _update_highway_list counted, hurdles not multiplied by x (:388);
// total: inter, the switch into the best lane and the best lane's hurdles from there to its highway (best_from_sp = v_ones_from(best_vec, best_sp))
ASM_HD int greedy_cand_inter(int sw, int nh) { return sw + nh; }
ASM_HD int greedy_cand_total(GreedyCosts c, int lane, int best, int fb, int sp, int len, int inter, V128 best_vec, int best_sp, int best_from_sp) {
    const int tail = c.x * v_pop_between_pre(best_vec, fb + sp + len, best_sp, best_from_sp);
    return inter + lane_penalty(lane, best, c.o, c.e) + (tail > 0 ? tail : 0);
}
// The ordered fold (:382-399): lanes in ascending order, one is accepted only if it is no worse than the last accepted one in both
// total and intermediate cost (<=: later lanes win ties).  The thresholds start at the best lane's cost and only go down.
ASM_HD bool greedy_fold_accept(int total, int inter, int& small_total, int& small_inter) {
    if (total <= small_total && inter <= small_inter) {
        small_total = total, small_inter = inter;
        return true;
    }
    return false;
}

// ---- _step commit (:411-433): take the chosen lane's highway; true when the lane's end is reached ----
ASM_HD bool greedy_commit(const CigarSink& cig, bool writer, long pair, int& ncig, int m, int nn, int ch, int ch_end, int ch_cost,
                          int& cur_lane, int& cur_col, int& cost) {
    cost += ch_cost;
    if (cig.on() && writer) cig.step(pair, ncig, cur_lane, ch, ch_end - greedy_start_col(cur_lane, cur_col, ch));
    cur_lane = ch;
    cur_col = ch_end;
    return cur_col >= lane_destination(m, nn, ch);
}

// ---- final hop (:575-590): from where the steps ended to the end of the destination lane.  The caller says how it gets that lane's
// vector (dest_vec() -> V128, asked only when a hop is needed): kept, read from the lane that holds it, or rebuilt — the lane may lie
// outside the band: undefined in the reference, built like a band lane ----
template <class DestVec>
ASM_HD void greedy_final_hop(GreedyCosts c, const CigarSink& cig, bool writer, long pair, int& ncig, int m, int nn, int dest_lane,
                             DestVec dest_vec, int cur_lane, int cur_col, int& cost) {
    const int dest_col = lane_destination(m, nn, dest_lane);
    if (cur_lane != dest_lane || cur_col < dest_col) {
        const int sw_f = c.semi ? 0 : lane_penalty(cur_lane, dest_lane, c.o, c.e);
        const int distance = v_pop_between(dest_vec(), cur_col + fwd_col(cur_lane, dest_lane), dest_col);
        const int hc = c.x * distance;
        cost += sw_f + (hc > 0 ? hc : 0);
        if (cig.on() && writer) cig.step(pair, ncig, cur_lane, dest_lane, distance);
    }
}
