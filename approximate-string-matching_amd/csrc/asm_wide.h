// General-parameter kernels: wide bands (k up to 50/63), arbitrary penalties, and the affine-gap NW.
//
// For a wide band the 2k+1 lanes no longer fit one thread's registers, so the mapping flips: ONE WORKGROUP
// PER READ PAIR, thread = band lane (the "wavefront per pair" shape: 61 lanes at k = 30 fill a 64-wide wave),
// neighbours exchange their furthest-reach values through a small LDS ring, and `__syncthreads_or` doubles
// as the per-generation barrier and the "some lane reached the end" vote.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "asm_bits.h"
#include "asm_kernels.h"
#include "asm_launch.h"

#define ASM_WIDE_RING 16

// --------------------------------------------------------------------------------------------------------
// LEAP, any k <= 63, any penalties 1 <= ext <= o, x >= 1 (<= 15), len <= 64*W64.  LV::run, LV_BAG.cpp:127-245.
// --------------------------------------------------------------------------------------------------------
template <int W64>
__global__ __launch_bounds__(ASM_WIDE_THREADS) void leap_wide_kernel(const uint4* __restrict__ planes,
                                                                     const uint32_t* __restrict__ lens, long n,
                                                                     int w4, int k, int x, int o, int ext,
                                                                     int mode /* ASM_LEAP_* (LV::init's ED_modes) */, OutMap out) {
    // LOCAL and SEMI_FREE_BEGIN give every lane a start at generation 0, at the lane's distance from the main one (LV_BAG.cpp:
    // 102-104); LOCAL and SEMI_FREE_END accept any lane that reaches the end, without converge_ED's lane term and threshold (:220-238)
    const bool all_start = mode == 1 || mode == 2, converge_rule = mode == 0 || mode == 2;
    __shared__ int s_end[ASM_WIDE_RING][ASM_WIDE_THREADS + 2];
    __shared__ int s_ip[ASM_WIDE_RING][ASM_WIDE_THREADS + 2];
    __shared__ int s_dp[ASM_WIDE_RING][ASM_WIDE_THREADS + 2];
    const int t = threadIdx.x;
    const int nl = 2 * k + 1;
    const bool active = t < nl;
    const int d = t - k; /* lane l = t + 1, mid = k + 1 */
    const int diff = d < 0 ? -d : d;
    for (long i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t ln = lens[i];
        const int m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
        const int len = m > nn ? m : nn;
        VW<W64> A0, A1, B0, B1;
        load_planes<W64>(planes, n, w4, i, A0, A1, B0, B1);
        const VW<W64> VA = vw_low_ones<W64>(m), VB = vw_low_ones<W64>(nn);
        VW<W64> mask;
        if (active) {
            mask = leap_lane_mask<W64>(A0, A1, B0, B1, VA, VB, d);
        } else {
#pragma unroll
            for (int q = 0; q < W64; q++) mask.w[q] = ~0ull;
        }
        // ring slots hold generations e mod RING; slot index t+1 leaves the two sentinel lanes at -2
        for (int g = 0; g < ASM_WIDE_RING; g++) {
            s_end[g][t + 1] = -2, s_ip[g][t + 1] = -2, s_dp[g][t + 1] = -2;
            if (t < 2) {
                const int edge = t == 0 ? 0 : ASM_WIDE_THREADS + 1;
                s_end[g][edge] = -2, s_ip[g][edge] = -2, s_dp[g][edge] = -2;
            }
        }
        int pass0 = 0;
        if (active && (d == 0 || all_start)) { /* e = 0, LV_BAG.cpp:131-147: start[l][0] = |l - mid| */
            const int from0 = diff > len ? len : diff; /* as a start of any later generation (count_ID_length, :9-23) */
            int r0 = vw_next_one<W64>(mask, from0);
            r0 = r0 > len ? len : r0;
            const int e0 = diff > len ? diff : r0;
            s_end[0][t + 1] = e0;
            pass0 = (e0 == len);
        }
        int result = -1;
        if (__syncthreads_or(pass0)) {
            result = 0;
        } else {
            for (int e = 1; e <= ASM_LEAP_AF_THRESHOLD; e++) {
                int pass = 0;
                int enew = -2, inew = -2, dnew = -2;
                if (active) {
                    const int top = d >= 0 ? 1 : 0, bot = d <= 0 ? 1 : 0;
                    const int so = (e - o) & (ASM_WIDE_RING - 1), se = (e - ext) & (ASM_WIDE_RING - 1),
                              sx = (e - x) & (ASM_WIDE_RING - 1);
                    /* lanes t-1 / t+1; beyond the band (sentinels and inactive threads) everything is -2, and so is a read the
                     * reference guards: the ring is 16 deep whatever the penalties (lv_affine_step) */
                    const int e_up = (e >= o && t > 0) ? s_end[so][t] : -2;
                    const int i_up = (e >= ext && t > 0) ? s_ip[se][t] : -2;
                    const int e_dn = (e >= o && t + 1 < nl) ? s_end[so][t + 2] : -2;
                    const int d_dn = (e >= ext && t + 1 < nl) ? s_dp[se][t + 2] : -2;
                    const int own = (e >= x) ? s_end[sx][t + 1] : -2;
                    const LvStep s = lv_affine_step(e_up, i_up, e_dn, d_dn, own, top, bot);
                    const int st = s.st;
                    inew = s.inew, dnew = s.dnew;
                    if (st >= 0) {
                        const int from = st > len ? len : st;
                        int r = vw_next_one<W64>(mask, from);
                        r = r > len ? len : r;
                        enew = st > len ? st : r;
                        if (enew == len && (!converge_rule || e + affine_gap(diff, o, ext) <= ASM_LEAP_AF_THRESHOLD)) pass = 1;
                    }
                }
                const int sw = e & (ASM_WIDE_RING - 1);
                s_end[sw][t + 1] = enew, s_ip[sw][t + 1] = inew, s_dp[sw][t + 1] = dnew;
                if (__syncthreads_or(pass)) {
                    result = e;
                    break;
                }
            }
        }
        if (t == 0) out.put(i, result);
        __syncthreads(); /* ring is re-initialised by the next pair */
    }
}


// --------------------------------------------------------------------------------------------------------
// Greedy, any k <= 50: workgroup per pair, thread = lane.  The step's rules are asm_greedy_lane.h's; the two
// lane loops of _update_highway_list become per-thread work plus a workgroup arg-max, and both the arg-max and the
// order-dependent fold of _choose_best_highway are replayed in lane order from LDS by every thread.
// --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASM_WIDE_THREADS) void greedy_wide_kernel(const uint4* __restrict__ planes,
                                                                       const uint32_t* __restrict__ lens, long n,
                                                                       int w4, int k, GreedyArgs args,
                                                                       OutMap out, CigarSink cig) {
    __shared__ double s_heur[ASM_WIDE_THREADS];
    __shared__ int s_leap[ASM_WIDE_THREADS];
    __shared__ int s_sp[ASM_WIDE_THREADS], s_len[ASM_WIDE_THREADS], s_cost[ASM_WIDE_THREADS];
    __shared__ int s_inter[ASM_WIDE_THREADS], s_total[ASM_WIDE_THREADS];
    __shared__ u64 s_vec[2];
    const int t = threadIdx.x;
    const int nl = 2 * k + 1;
    const bool active = t < nl;
    const int lane = t - k;
    const GreedyCosts pen = {args.x, args.o, args.e, args.semi != 0};
    for (long i = blockIdx.x; i < n; i += gridDim.x) {
        const V128 A0 = v_from_uint4(planes[((long)0 * w4) * n + i]);
        const V128 A1 = v_from_uint4(planes[((long)1 * w4) * n + i]);
        const V128 B0 = v_from_uint4(planes[((long)2 * w4) * n + i]);
        const V128 B1 = v_from_uint4(planes[((long)3 * w4) * n + i]);
        int m, nn, dest_lane;
        greedy_lengths(lens[i], m, nn, dest_lane);
        const V128 lo_ = greedy_lane_vector(A0, A1, B0, B1, lane);
        const V128 lf_ = v_flip_short_hurdles1(lo_);
        int sp = -1, len = 0, nsw = 128;
        const int dst = lane_destination(m, nn, lane);
        int cur_lane = 0, cur_col = 0, cost = 0, ncig = 0;
        const long pair = out.index(i);
        for (int guard = 0; guard < 4 * 128; guard++) {
            int reach = 0, sw = 0, nh = 0;
            if (active) {
                const int start_col = greedy_start_col(cur_lane, cur_col, lane);
                if (sp < start_col) {
                    int fz, nx;
                    v_highway_from(lf_, start_col, fz, nx);
                    reach = greedy_refresh(greedy_highway_at(start_col, fz, nx, dst), cur_lane, lane, sp, len, nsw) ? 1 : 0;
                }
                sw = greedy_switch_cost(pen.semi && guard == 0, cur_lane, lane, pen.o, pen.e);
                nh = greedy_hurdles(lo_, start_col, sp, len);
            }
            const int reaching = __syncthreads_or(reach);
            const int hc = pen.x * nh;
            if (active) {
                double heur;
                int leap;
                greedy_score(args, pen, reaching != 0, lane, dest_lane, dst, sp, len, nsw, sw, nh, heur, leap);
                s_heur[t] = heur, s_leap[t] = leap;
                s_sp[t] = sp, s_len[t] = len, s_cost[t] = sw + hc;
            }
            __syncthreads();
            // arg-max in lane order, replayed by every thread from LDS (broadcast reads)
            double best_h = -__builtin_inf();
            int best_leap = 0, bt = k; /* reference default best lane 0 <-> thread k */
            for (int j = 0; j < nl; j++) {
                const double hj = s_heur[j];
                const int lj = s_leap[j];
                if (greedy_beats(hj, lj, best_h, best_leap)) best_h = hj, best_leap = lj, bt = j;
            }
            const int best = bt - k, best_sp = s_sp[bt], best_len = s_len[bt], best_cost = s_cost[bt];
            if (best_len <= 0) break; /* uniform across the workgroup */
            if (t == bt) s_vec[0] = lo_.lo, s_vec[1] = lo_.hi;
            __syncthreads();
            const V128 best_vec = v_make(s_vec[0], s_vec[1]);
            const int best_from_sp = v_ones_from(best_vec, best_sp);
            int inter = 0x3fffffff, total = 0x3fffffff;
            const int fb = fwd_col(lane, best);
            if (active && greedy_cand_reachable(lane, best, fb, sp, best_sp)) {
                inter = greedy_cand_inter(sw, nh);
                total = greedy_cand_total(pen, lane, best, fb, sp, len, inter, best_vec, best_sp, best_from_sp);
            }
            s_inter[t] = inter, s_total[t] = total;
            __syncthreads();
            int small_inter = best_cost, small_total = best_cost, ct = bt;
            for (int j = 0; j < nl; j++) {
                if (greedy_fold_accept(s_total[j], s_inter[j], small_total, small_inter)) ct = j; /* the best lane's own slot holds no candidate */
            }
            const bool done = greedy_commit(cig, t == 0, pair, ncig, m, nn, ct - k, s_sp[ct] + s_len[ct], s_cost[ct], cur_lane, cur_col, cost);
            __syncthreads(); /* LDS arrays are rewritten by the next step */
            if (done) break;
        }
        if (t == 0) {
            greedy_final_hop(pen, cig, true, pair, ncig, m, nn, dest_lane, [&]() { return greedy_lane_vector(A0, A1, B0, B1, dest_lane); }, cur_lane,
                             cur_col, cost);
            if (cig.on()) cig.finish(pair, ncig);
            out.put(i, cost);
        }
        __syncthreads();
    }
}


// --------------------------------------------------------------------------------------------------------
// NW with affine gaps (Gotoh), arbitrary penalties: gotoh_sweep (asm_affine.h), score only, one thread per pair; the block
// boundary column in LDS [row][thread].
// --------------------------------------------------------------------------------------------------------
template <int W64, int MAXROWS>
__global__ __launch_bounds__(64) void nw_affine_kernel(const uint4* __restrict__ planes,
                                                       const uint32_t* __restrict__ lens, long n, int w4, int x,
                                                       int o, int e, OutMap out, const uint32_t* __restrict__ todo,
                                                       const uint32_t* __restrict__ todo_count) {
    __shared__ uint32_t s_bound[MAXROWS + 1][64];
    const int t = threadIdx.x;
    long i = (long)blockIdx.x * 64 + t;
    if (todo) { /* second pass of launch_nw_wfa: only the listed bucket slots */
        if (i >= (long)*todo_count) return;
        i = (long)todo[i];
    }
    if (i >= n) return;
    const uint32_t ln = lens[i];
    const int m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
    VW<W64> A0, A1, B0, B1;
    load_planes<W64>(planes, n, w4, i, A0, A1, B0, B1);
    NoCellSink sink;
    const int result = gotoh_sweep<W64>(A0, A1, B0, B1, m, nn, x, o, e, &s_bound[0][t], 64, sink);
    out.put(i, result);
}

