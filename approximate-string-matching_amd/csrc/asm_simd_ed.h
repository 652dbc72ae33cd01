// What one thread of the filter kernels (asm_filter.h) decides for its pair: bit-parallel LEAP (SIMD_ED, Levenshtein and affine
// mode) and the SHD pre-filter of GASMA/benchmark/LEAP_SIMD — the filtering stage in front of the aligners (SURVEY.md §8 f-3;
// driver LEAP_SIMD/main.cpp:95-101,186-195) — on the batch's 2-bit planes.  Vectors are W64 64-bit words (2: length <= 128,
// 4: <= 256 = _MAX_LENGTH_).  The kernels keep their thread shapes, LDS carving, fences and wave mechanics; every rule is here.
//
// Reference behaviour kept on purpose (oracle/asm_oracle_filter.c S1-S4):
//  S1  the reference's 256-bit shifts move each 128-bit half on its own (shift.cpp:33-61);
//  S2  SIMD_ED's verdict state (final_ED, final lane, converge_ED) flows from pair to pair: a pair yields one *event* and, in
//      sequential mode, two last-setter scans resolve the chain in batch order (simd_setter_key .. simd_verdict_sequential);
//  S3  the mask-array SHD inside SIMD_ED amends nothing and masks the main lane with bits 0..254 (SHD.cpp:324-372);
//  S4  a lane that starts at or beyond the end reaches the end (SIMD_ED.cpp:57-60).
//
// The header compiles for the host as well (LU_HD): host/filter_host_check.cpp drives every function here serially in the kernels'
// shapes against the oracle and the reference's recorded results (tests/test_filter_host.py).
#pragma once
#include "asm_affine.h"
#include "asm_limits.h"

#define ASM_SHD_MAX_ERROR 16   /* MAX_ERROR_AVX (LEAP_SIMD/mask.h:21): rows of the reference's begin-mask table */

// events of one pair (S2)
#define EV_REJECTED (-1)  /* SHD said no: verdict fail, state untouched                                             */
#define EV_NOT_REACHED (-2) /* no lane reached the end within T generations: verdict = the carried state's             */
#define EV_EXACT (-3)     /* the main lane reached the end at e = 0: passes, sets (final_ED, lane) = (0, 0) only;
                             EV_EXACT - d: the same on a lane d off the main one (ED_modes LOCAL / SEMI_FREE_BEGIN)          */
/* >= 0: reached at generation fe on a lane fd away from the main one: fe | fd << 8                                     */
LU_HD int simd_ev_reached(int e, int dist) { return e | (dist << 8); }
LU_HD int simd_ev_exact(int dist) { return EV_EXACT - dist; }

// init_levenshtein's / init_affine's ED_modes (ASM_LEAP_*): LOCAL (1) and SEMI_FREE_BEGIN (2) keep every lane live from generation
// 0, starting at its distance from the main lane (SIMD_ED.cpp:246-266,476-478,497-516); GLOBAL and SEMI_FREE_END let lane l join at
// generation |l - mid|.  LOCAL and SEMI_FREE_END (3): any lane that reaches the end passes and get_ED() is final_ED (:589-610,748-753)
LU_HD bool simd_all_start(int mode) { return mode == 1 || mode == 2; }
LU_HD bool simd_converge_rule(int mode) { return mode == 0 || mode == 2; }
LU_HD int simd_lane_dist(int j, int mid) { return j < mid ? mid - j : j - mid; }

// bits move away from index 0 by s in [0, 63], each 128-bit half separately when W64 = 4 (S1)
template <int W64>
LU_HD VW<W64> avx_away0(const VW<W64>& v, int s) {
    VW<W64> r;
#pragma unroll
    for (int q = 0; q < W64; q++) {
        const u64 lo = (q & 1) ? v.w[q - 1] : 0ull; /* nothing crosses an even word boundary */
        r.w[q] = (v.w[q] << s) | (s ? (lo >> (64 - s)) : 0ull);
    }
    return r;
}

// hamming mask of lane d = l - mid in [-T, T] (SIMD_ED::calculate_masks, SIMD_ED.cpp:180-212): d < 0 shifts the reference,
// d > 0 the read
template <int W64>
LU_HD VW<W64> simd_lane_mask(const VW<W64>& A0, const VW<W64>& A1, const VW<W64>& B0, const VW<W64>& B1, int d) {
    VW<W64> r;
    const int s = d < 0 ? -d : d;
    if (d < 0) {
        const VW<W64> b0 = avx_away0<W64>(B0, s), b1 = avx_away0<W64>(B1, s);
#pragma unroll
        for (int q = 0; q < W64; q++) r.w[q] = (A0.w[q] ^ b0.w[q]) | (A1.w[q] ^ b1.w[q]);
    } else {
        const VW<W64> a0 = avx_away0<W64>(A0, s), a1 = avx_away0<W64>(A1, s);
#pragma unroll
        for (int q = 0; q < W64; q++) r.w[q] = (a0.w[q] ^ B0.w[q]) | (a1.w[q] ^ B1.w[q]);
    }
    return r;
}

// end position of the run of matches that starts at st (start + count_ID_length_avx, SIMD_ED.cpp:10-61): the next set bit
// of the lane mask, capped at len.  The reference shifts the mask down by st half by half (S1), so for st < 128 the bits
// 128 .. 127+st never arrive and read as matches.
template <int W64>
LU_HD int simd_extend(const VW<W64>& mask, int st, int len) {
    if (st >= len) return len; /* S4: st + (len - st) */
    VW<W64> v = mask;
    if (W64 == 4 && st < 128) {
        v.w[2] &= st >= 64 ? 0ull : (~0ull << st);
        if (st > 64) v.w[3] &= ~0ull << (st - 64);
    }
    const int r = vw_next_one<W64>(v, st);
    return r < len ? r : len;
}

// popcount_SHD_avx (popcount.cpp:44-76,78-110): a table lookup per nibble that is the number of runs of ones in the nibble,
// except that 0110 counts 2
template <int W64>
LU_HD int shd_popcount(const VW<W64>& v) {
    int s = 0;
#pragma unroll
    for (int q = 0; q < W64; q++) {
        const u64 w = v.w[q];
        const u64 x = w ^ 0x6666666666666666ull; /* a nibble of x is zero where w's is 0110 */
        const u64 is6 = ~(x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ull;
        s += __builtin_popcountll(w & ~((w << 1) & 0xeeeeeeeeeeeeeeeeull)) + __builtin_popcountll(is6);
    }
    return s;
}

template <int W64>
LU_HD VW<W64> vw_from(int cnt) { /* bits cnt.. set: MASK_AVX_BEG row cnt-1 (mask.cpp:149-166) */
    VW<W64> r = vw_low_ones<W64>(cnt);
#pragma unroll
    for (int q = 0; q < W64; q++) r.w[q] = ~r.w[q];
    return r;
}

// ---- load and clip ----------------------------------------------------------------------------------------------------------------
// main.cpp:131-132: the read's length, at most `cap` = _MAX_LENGTH_ (or the kernel's width); strncpy(A/B, ., length) — what lies
// beyond is never compared, but it is cleared so that shifts bring in zeros only.  The reference string ends at its own length (a
// sequential-mode batch keeps Greedy's stale tail bits beyond it).
struct SimdClip {
    int len, ref; /* positions kept of the read's planes and of the reference's */
};
LU_HD SimdClip simd_clip(uint32_t ln, int cap) {
    const int m = (int)(ln & 0xffffu), nn_ref = (int)(ln >> 16);
    SimdClip c;
    c.len = m > cap ? cap : m;
    c.ref = nn_ref < c.len ? nn_ref : c.len;
    return c;
}

template <int W64>
struct SimdPair {
    VW<W64> A0, A1, B0, B1; /* read planes 0/1, reference planes 0/1, clipped */
    int len;
};
template <int W64>
LU_HD SimdPair<W64> simd_load_pair(const lu_quad* __restrict__ planes, const uint32_t* __restrict__ lens, long n, int w4, long i) {
    SimdPair<W64> p;
    const SimdClip c = simd_clip(lens[i], 64 * W64);
    p.len = c.len;
    load_planes<W64>(planes, n, w4, i, p.A0, p.A1, p.B0, p.B1);
    const VW<W64> lm = vw_low_ones<W64>(c.len), lb = vw_low_ones<W64>(c.ref);
#pragma unroll
    for (int q = 0; q < W64; q++) p.A0.w[q] &= lm.w[q], p.A1.w[q] &= lm.w[q], p.B0.w[q] &= lb.w[q], p.B1.w[q] &= lb.w[q];
    return p;
}
template <int W64>
LU_HD VW<W64> simd_lane_mask(const SimdPair<W64>& p, int d) {
    /* four objects of their own: which pair of planes is shifted depends on d, and a choice between two members of one struct
     * keeps the struct in memory (40 bytes of scratch in simd_ed_kernel<0, 2>) */
    const VW<W64> A0 = p.A0, A1 = p.A1, B0 = p.B0, B1 = p.B1;
    return simd_lane_mask<W64>(A0, A1, B0, B1, d);
}

// ---- the mask-array SHD (S3) ------------------------------------------------------------------------------------------------------
// bit_vec_filter_avx(hamming_masks + first, buffer_length, T) (SHD.cpp:324-372): the 2T+1 lane masks mask_of(0 .. 2T), each cut by
// the begin mask of its distance from the centre one (bits 0..254 for the centre itself), ANDed together.  NLC > 0: 2T+1 at compile
// time, for a caller whose masks sit in a register array; NLC = 0: T at run time.
template <int W64, int NLC, class MaskOf>
LU_HD bool simd_shd_rejects(const SimdPair<W64>& p, int T, MaskOf mask_of) {
    VW<W64> diff = vw_low_ones<W64>(p.len);
    const auto lane = [&](int j) {
        const int s = simd_lane_dist(j, T);
        const VW<W64> tm = s ? vw_from<W64>(s) : vw_low_ones<W64>(255);
        const VW<W64> h = mask_of(j);
#pragma unroll
        for (int q = 0; q < W64; q++) diff.w[q] &= h.w[q] & tm.w[q];
    };
    if constexpr (NLC > 0) {
#pragma unroll
        for (int j = 0; j < NLC; j++) lane(j);
    } else {
        for (int j = 0; j <= 2 * T; j++) lane(j);
    }
    return shd_popcount<W64>(diff) > T;
}

// ---- SIMD_ED::run_levenshtein for one pair (SIMD_ED.cpp:269-352) -> event ---------------------------------------------------------------
// where lane j of 0..2T starts in generation e (SIMD_ED.cpp:318-323): behind its own end of generation e-1, or where the lane above
// or below hands over; -2 = never written (:236-241)
LU_HD int simd_lev_start(int up, int own, int dn, int j, int T) {
    int st = own + 1;
    const int u = up + (j >= T ? 1 : 0), d = dn + (j <= T ? 1 : 0);
    st = u > st ? u : st;
    st = d > st ? d : st;
    return st;
}
LU_HD bool simd_lev_live(int j, int T, int e) { return simd_lane_dist(j, T) <= e; } /* cur_ED[l] == e: lane j has joined */
// one live lane of generation e >= 1: its new end; the first lane to reach the end (ascending j: the lowest wins, :334-340) sets ev
template <int W64>
LU_HD int simd_lev_lane(const VW<W64>& mask, int up, int own, int dn, int j, int T, int e, int len, int& ev) {
    const int en = simd_extend<W64>(mask, simd_lev_start(up, own, dn, j, T), len);
    if (en == len && ev == EV_NOT_REACHED) ev = simd_ev_reached(e, simd_lane_dist(j, T));
    return en;
}

// Two columns for the previous generation's ends, one loop each (docs/design/kernels.md says why they stay two):
// T = TT at compile time, ED_GLOBAL / SEMI_FREE_END: all lane masks hm[0 .. 2TT] and the column in registers, every lane visited
// in every generation under simd_lev_live so that all indices are constants
template <int TT, int W64>
LU_HD int simd_lev_events_reg(const SimdPair<W64>& p, const VW<W64>* hm) {
    constexpr int NLC = 2 * TT + 1;
    int ev = EV_NOT_REACHED;
    int prev[NLC + 2]; /* end[.][e-1] with the two guard lanes */
#pragma unroll
    for (int j = 0; j < NLC + 2; j++) prev[j] = -2;
    prev[TT + 1] = simd_extend<W64>(hm[TT], 0, p.len);
    if (prev[TT + 1] == p.len) ev = simd_ev_exact(0); /* SIMD_ED.cpp:291-296 */
    for (int e = 1; e <= TT && ev == EV_NOT_REACHED; e++) {
        int cur[NLC + 2];
        cur[0] = cur[NLC + 1] = -2;
#pragma unroll
        for (int j = 0; j < NLC; j++)
            cur[j + 1] = simd_lev_live(j, TT, e) ? simd_lev_lane<W64>(hm[j], prev[j], prev[j + 1], prev[j + 2], j, TT, e, p.len, ev) : -2;
#pragma unroll
        for (int j = 0; j < NLC + 2; j++) prev[j] = cur[j];
    }
    return ev;
}
// T at run time, every ED_mode: lane masks rebuilt per use, the column end(g, l) — generation parity g, lanes 1 .. 2T+1 between two
// guard rows — in memory of the caller's (the kernel: a thread-private LDS column), only the live lanes visited
template <int STRIDE>
struct SimdEndColumn {
    short* col;
    int rows; /* 2T + 3 */
    LU_HD short& operator()(int g, int l) const { return col[(g * rows + l) * STRIDE]; }
};
template <int W64, class Col>
LU_HD int simd_lev_events_col(const SimdPair<W64>& p, int T, bool all_start, const Col& end) {
    int ev = EV_NOT_REACHED;
    for (int l = 0; l < 2 * T + 3; l++) end(0, l) = -2, end(1, l) = -2;
    const int first = all_start ? 0 : T, last = all_start ? 2 * T : T;
    for (int j = first; j <= last && ev == EV_NOT_REACHED; j++) { /* cur_ED == 0, ascending */
        const int dist = simd_lane_dist(j, T);
        const int e0 = simd_extend<W64>(simd_lane_mask<W64>(p, j - T), dist, p.len);
        end(0, j + 1) = (short)e0;
        if (e0 == p.len) ev = simd_ev_exact(dist);
    }
    for (int e = 1; e <= T && ev == EV_NOT_REACHED; e++) {
        const int gp = (e - 1) & 1, gc = e & 1;
        for (int j = all_start ? 0 : T - e; j <= (all_start ? 2 * T : T + e) && ev == EV_NOT_REACHED; j++) /* simd_lev_live, ascending */
            end(gc, j + 1) = (short)simd_lev_lane<W64>(simd_lane_mask<W64>(p, j - T), end(gp, j), end(gp, j + 1), end(gp, j + 2), j, T, e,
                                                       p.len, ev);
    }
    return ev;
}

// ---- SIMD_ED in affine mode (init_affine / run_affine, SIMD_ED.cpp:435-616), CLEAN: every pair from init_affine's tables ---------------
// lv_affine_step (asm_affine.h) over SIMD_ED's own lane masks with the read's length as the target.  Result: get_ED() =
// converge_ED, the smallest e + gap(lane distance) <= af_t over the lanes that reach the end in the first generation in which one
// does; SIMD_AF_NONE — reset_affine's value — for a pair that reaches the end at e = 0 (run_affine returns before converge_ED is
// written); in LOCAL / SEMI_FREE_END final_ED, without a threshold.
#define SIMD_AF_NONE 1000000
struct SimdAffine {
    int T, af_t, x, o, ext, mode; /* gap threshold (lanes 1 .. 2T+1 around mid = T+1, guard rows 0 and 2T+2: SIMD_ED.cpp:452-453) */
    LU_HD int mid() const { return T + 1; }
    LU_HD int exact() const { return simd_converge_rule(mode) ? SIMD_AF_NONE : 0; } /* converge_ED is never written; final_ED = 0 */
};
// the rings of one pair: element [slot][lane row][column], `stride` columns (threads of the workgroup, or pairs of it)
template <typename EnT>
struct SimdAffineRings {
    EnT *en, *ip, *dp; /* this pair's column of `end` [gm], I [gi], D [gi] */
    LvRings rg;
    int slot, stride; /* elements per slot: (2T + 3) * stride */
};
// e = 0: the main lane (ED_GLOBAL, SEMI_FREE_END) or every lane at its distance (:474-477,497-516); a thread takes the lanes
// first + lane0, first + lane0 + step, ...  Returns whether one of them reached the end.  extend(d, st): where lane d's run of
// matches from st ends.
template <typename EnT, class Extend>
LU_HD bool simd_affine_seed(const SimdAffineRings<EnT>& r, const SimdAffine& a, int len, int lane0, int step, Extend extend) {
    const bool all_start = simd_all_start(a.mode);
    const int mid = a.mid(), last = all_start ? 2 * a.T + 1 : mid;
    bool exact = false;
    for (int l = (all_start ? 1 : mid) + lane0; l <= last; l += step) {
        const int e0 = extend(l - mid, simd_lane_dist(l, mid));
        r.en[l * r.stride] = (EnT)(e0 + 2);
        if (e0 == len) exact = true;
    }
    return exact;
}
// generation e >= 1 over the lanes a gap of this cost can have reached, dealt as in simd_affine_seed; returns the generation's
// converge_ED (final_ED in LOCAL / SEMI_FREE_END), SIMD_AF_NONE when no lane of this thread passed
template <typename EnT, class Extend>
LU_HD int simd_affine_generation(const SimdAffineRings<EnT>& r, const SimdAffine& a, int len, int e, int lane0, int step, Extend extend) {
    const bool converge_rule = simd_converge_rule(a.mode);
    const int mid = a.mid(), S = r.stride;
    int dmax = e < a.o ? 0 : (e - a.o) / a.ext + 1;
    dmax = (dmax > a.T || simd_all_start(a.mode)) ? a.T : dmax; /* (every lane is live from the start in LOCAL / SEMI_FREE_BEGIN) */
    const LvRingView<EnT> g(r.en, r.ip, r.dp, r.rg, r.slot, e, a.x, a.o, a.ext);
    int conv = SIMD_AF_NONE;
    for (int l = mid - dmax + lane0; l <= mid + dmax; l += step) {
        const int top = l >= mid ? 1 : 0, bot = l <= mid ? 1 : 0;
        const int e_up = (int)g.en_o[(l - 1) * S] - 2, i_up = (int)g.ip_e[(l - 1) * S] - 2;
        const int e_dn = (int)g.en_o[(l + 1) * S] - 2, d_dn = (int)g.dp_e[(l + 1) * S] - 2;
        const int own = (int)g.en_x[l * S] - 2;
        const LvStep s = lv_affine_step(e_up, i_up, e_dn, d_dn, own, top, bot); /* SIMD_ED.cpp:533-558 */
        int enew = -2;
        if (s.st >= 0) {
            enew = extend(l - mid, s.st); /* :579-581 */
            if (enew == len) { /* :589-603; :604-608: final_ED, no threshold */
                const int tc = converge_rule ? e + affine_gap(simd_lane_dist(l, mid), a.o, a.ext) : e;
                if ((!converge_rule || tc <= a.af_t) && tc < conv) conv = tc;
            }
        }
        g.en_w[l * S] = (EnT)(enew + 2), g.ip_w[l * S] = (EnT)(s.inew + 2), g.dp_w[l * S] = (EnT)(s.dnew + 2);
    }
    return conv; /* != SIMD_AF_NONE: ED_pass, the generation loop ends (:609-610) */
}

// ---- four threads per pair: the planes in dwords --------------------------------------------------------------------------------------
// A pair's four planes pair-major, SIMD_QUAD_PD dwords each: the 128 positions between two zero dwords, so that the window of a
// shifted operand can start up to 32 positions before the string (avx_away0 fills with zeros) and run past its end.
#define SIMD_QUAD_PW LEAP_QUAD_PAIR_DWORDS(SIMD_QUAD_PD)
// one plane of the batch into that layout, `keep` positions of it (simd_clip: len for a read plane, ref for a reference plane)
LU_HD void simd_quad_stage(uint32_t* dst, const lu_quad& v, int keep) {
    const uint32_t d4[4] = {v.x, v.y, v.z, v.w};
    dst[0] = 0u, dst[5] = 0u;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int kb = keep - 32 * w;
        dst[1 + w] = kb >= 32 ? d4[w] : (kb <= 0 ? 0u : (d4[w] & ((1u << kb) - 1u)));
    }
}
LU_HD uint32_t simd_quad_window(const uint32_t* plane, int pos) { /* pos is already offset by the leading zero dword */
    const int q = pos >> 5;
    return lu_alignbit(plane[q + 1], plane[q], (uint32_t)(pos & 31));
}
// simd_extend(simd_lane_mask(d), st, len) on those planes: d < 0 shifts the reference away from 0, d > 0 the read
LU_HD int simd_quad_extend(const uint32_t* pl, int d, int st, int len) {
    if (st >= len) return len;
    const int s = d < 0 ? -d : d;
    int apos = st + 32 - (d > 0 ? s : 0), bpos = st + 32 - (d < 0 ? s : 0), p = st;
    for (;;) {
        const uint32_t diff = (simd_quad_window(pl, apos) ^ simd_quad_window(pl + 2 * SIMD_QUAD_PD, bpos)) |
                              (simd_quad_window(pl + SIMD_QUAD_PD, apos) ^ simd_quad_window(pl + 3 * SIMD_QUAD_PD, bpos));
        if (diff) {
            p += __builtin_ctz(diff);
            break;
        }
        p += 32, apos += 32, bpos += 32;
        if (p >= len) break;
    }
    return p < len ? p : len;
}

// ---- verdicts (S2) ----------------------------------------------------------------------------------------------------------------
// clean mode: every pair judged alone — never reached: fail; exact: 0; reached: final_ED + lane distance if <= T
LU_HD int simd_verdict_clean(int ev, int T) {
    if (ev <= EV_EXACT) return 0;
    if (ev < 0) return -1;
    const int conv = (ev & 0xff) + (ev >> 8);
    return conv <= T ? conv : -1;
}
// ED_modes LOCAL and SEMI_FREE_END: a pair passes exactly when a lane reached the end, and get_ED() is final_ED
// (SIMD_ED.cpp:348-351 does not apply, :748-753) — no state of an earlier pair is read
LU_HD int simd_verdict_final(int ev) { return ev <= EV_EXACT ? 0 : (ev >= 0 ? (ev & 0xff) : -1); }
// sequential mode, step 1: key of the (final_ED, lane) chain — pairs that set it carry fe | fd << 8 (exact: final_ED = 0 on a lane
// EV_EXACT - ev off the main one), the others -1
LU_HD int simd_setter_key(int ev) { return ev <= EV_EXACT ? ((EV_EXACT - ev) << 8) : (ev >= 0 ? ev : -1); }
// step 2 (state_after: the last-setter scan of the setter keys at this pair): converge_ED is rewritten by pairs that run to the end of
// run_levenshtein (reached or not) from the state in force; exact and rejected pairs leave it alone
LU_HD int simd_converge_key(int ev, int state_after, int init_fe, int init_fd) {
    if (!(ev >= 0 || ev == EV_NOT_REACHED)) return -1;
    return state_after >= 0 ? (state_after & 0xff) + (state_after >> 8) : init_fe + init_fd;
}
// step 3 (conv_before / conv_own: the last-setter scan of the converge keys at the pair before, -1 for the first pair, and at this
// one): an exact pair passes and get_ED() is the converge_ED left by the pairs before it
LU_HD int simd_verdict_sequential(int ev, int conv_before, int conv_own, int T, int init_conv) {
    if (ev <= EV_EXACT) return conv_before >= 0 ? conv_before : init_conv;
    if (ev == EV_REJECTED) return -1;
    return conv_own <= T ? conv_own : -1;
}
struct LastSetter { /* scan operator: the most recent non-negative key */
    LU_HD int32_t operator()(int32_t a, int32_t b) const { return b >= 0 ? b : a; }
};

// ---- SHD on the planes: bit_vec_filter_avx(read0, read1, ref0, ref1, length, max_error) (SHD.cpp:241-322) ---------------------------------
// the four in-byte windows of flip_false_zero (SHD.cpp:95-122): in bits i..i+3 of every byte, every zero between the lowest
// and the highest set bit is set (MASK_SRS, mask.cpp:427-432); the windows are applied one after the other
LU_HD u64 srs_round_word(u64 w) {
    const u64 NIB = 0x0f0f0f0f0f0f0f0full;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u64 nb = (w >> i) & NIB;
        const u64 below = nb | (nb << 1) | (nb << 2) | (nb << 3); /* a set bit at or below */
        const u64 above = nb | (nb >> 1) | (nb >> 2) | (nb >> 3); /* a set bit at or above */
        w |= (below & above & NIB) << i;
    }
    return w;
}

template <int W64>
LU_HD VW<W64> shd_flip_false_zero(VW<W64> v) { /* SHD.cpp:95-143 */
#pragma unroll
    for (int q = 0; q < W64; q++) v.w[q] = srs_round_word(v.w[q]);
    VW<W64> sv = avx_away0<W64>(v, 4); /* the windows that straddle a byte boundary */
#pragma unroll
    for (int q = 0; q < W64; q++) sv.w[q] = srs_round_word(sv.w[q]);
#pragma unroll
    for (int q = 0; q < W64; q++) { /* shift_left_avx(., 4): back towards index 0, half by half */
        const u64 hi = (q & 1) ? 0ull : sv.w[q + 1];
        v.w[q] |= (sv.w[q] >> 4) | (hi << 60);
    }
    return v;
}

template <int W64>
LU_HD bool shd_pass(const SimdPair<W64>& p, int max_error) {
    const VW<W64> lm = vw_low_ones<W64>(p.len);
    VW<W64> diff = shd_flip_false_zero<W64>(simd_lane_mask<W64>(p, 0));
    for (int j = 1; j <= max_error; j++) {
        const VW<W64> tm = vw_from<W64>(j);
#pragma unroll
        for (int sign = 1; sign >= -1; sign -= 2) { /* the read shifted by j against the reference, then the other way round */
            VW<W64> t = simd_lane_mask<W64>(p, sign * j);
#pragma unroll
            for (int q = 0; q < W64; q++) t.w[q] &= tm.w[q] & lm.w[q];
            t = shd_flip_false_zero<W64>(t);
#pragma unroll
            for (int q = 0; q < W64; q++) diff.w[q] &= t.w[q];
        }
    }
    return shd_popcount<W64>(diff) <= max_error;
}
