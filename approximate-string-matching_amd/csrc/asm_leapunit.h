// LEAP (banded affine Landau-Vishkin, "BAG") with unit penalties x = o = e = 1: what one thread of leap_unit_kernel and
// leap_unit_hint_kernel (asm_kernels.h) computes for its pair, with the word vectors (VW, vw_*) and the lane masks the other
// LEAP kernels share.
//
// Follows LV::run (LEAP_SIMD/LV_BAG.cpp:127-245) with init(k,200,ED_GLOBAL,1,1,1); the scalar character loop
// count_ID_length (:9-23) becomes a count-trailing-zeros on the lane's mismatch bit-vector.  Only generation e-1 is live
// (SURVEY.md L6), so one register per lane replaces the four [2k+3][201] tables.  W64 = number of 64-bit words per vector
// (2: len <= 128, 4: len <= 256).
//
// Two forms of the same function:
//   leap_unit_generic<K, W64>  every width; the form all widths ran before the one-granule form existed
//   leap_unit_w2<K>            W64 == 2 (one 128-base granule per string: the width the 100 bp workloads run), see below
// leap_unit_core<K, W64> picks between them; both return LV::run's final_ED, or -1.
//
// The header compiles for the host as well (LU_HD): host/leap_host_check.cpp runs both forms on the CPU against each other and
// against the oracle (tests/test_leap_unit_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LU_HD __host__ __device__ __forceinline__
typedef uint4 lu_quad;
#else
#define LU_HD inline
struct lu_quad {
    uint32_t x, y, z, w;
};
#endif

#ifndef ASM_LEAP_AF_THRESHOLD
#define ASM_LEAP_AF_THRESHOLD 200 /* benchmark_utils.h:289; include/asm_mi355x.h has the same */
#endif

typedef unsigned long long u64;

// ---- small primitives (device: one instruction each; host: the plain meaning) ------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
// v_ffbl_b32: index of the lowest set bit, 0xFFFFFFFF for an empty word
LU_HD unsigned lu_ffbl(unsigned x) {
    unsigned r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
LU_HD unsigned lu_add_sat(unsigned a, unsigned b) { return __builtin_elementwise_add_sat(a, b); }
LU_HD uint32_t lu_alignbit(uint32_t hi, uint32_t lo, uint32_t s) { return __builtin_amdgcn_alignbit(hi, lo, s); }
#else
LU_HD unsigned lu_ffbl(unsigned x) { return x ? (unsigned)__builtin_ctz(x) : 0xFFFFFFFFu; }
LU_HD unsigned lu_add_sat(unsigned a, unsigned b) { return a + b < a ? 0xFFFFFFFFu : a + b; }
LU_HD uint32_t lu_alignbit(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((u64)hi << 32) | (u64)lo) >> (s & 31u)); }
#endif
LU_HD unsigned lu_min(unsigned a, unsigned b) { return a < b ? a : b; }

template <int W64>
struct VW {
    u64 w[W64];
};

// first set bit at or after `from` in a W64-word vector, or W64*64 when none.  `from` in [0, W64*64].
// Only the word `from` falls into needs its low bits dropped (one 64-bit shift, taken mod 64 by the hardware); the words
// above it count from their own bit 0, the words below it not at all.
template <int W64>
LU_HD int vw_next_one(const VW<W64>& v, int from) {
    const int q = from >> 6;
    u64 x = v.w[W64 - 1];
#pragma unroll
    for (int qq = W64 - 2; qq >= 0; qq--) x = q == qq ? v.w[qq] : x;
    const u64 y = x >> (from & 63);
    int res = W64 * 64;
#pragma unroll
    for (int qq = W64 - 1; qq >= 1; qq--) /* descending: the lowest non-empty word above `from` wins */
        if (qq > q && v.w[qq]) res = qq * 64 + __builtin_ctzll(v.w[qq]);
    if (y) res = from + __builtin_ctzll(y);
    return from >= W64 * 64 ? W64 * 64 : res;
}

// The same scan for a caller that keeps, per vector, "first set bit in the words above word q" (W64 * 64 when none) for every q
// but the last: v_ffbl_b32 gives 0xFFFFFFFF for an empty word, and with saturating adds an empty shifted word turns into a candidate
// that loses the final min — no zero tests, no compare-and-select chain behind the shift (asm_bits.h, v_next_one_from_fb).
/* Up to three words per vector the fall-backs cost no registers the compiler was not already spending (it hoists the upper
 * words' ctz out of the generation loop either way: 59 and 90 VGPRs before and after at two and three words).  From four words
 * on they do — 120 -> 146 and 165 -> 209 VGPRs at four and six words, a wave per SIMD less — and the wider classes of C5 lost
 * what the shorter scan gained: those keep vw_next_one. */
#define VW_SCAN_FB(W64) ((W64) <= 3)
template <int W64>
struct VWAbove {
    unsigned fb[W64 > 1 ? W64 - 1 : 1];
};
template <int W64>
LU_HD VWAbove<W64> vw_above(const VW<W64>& v) {
    VWAbove<W64> r;
    unsigned run = W64 * 64u;
#pragma unroll
    for (int q = W64 - 2; q >= 0; q--) {
        run = v.w[q + 1] ? (unsigned)(q + 1) * 64u + (unsigned)__builtin_ctzll(v.w[q + 1]) : run;
        r.fb[q] = run;
    }
    return r;
}
template <int W64>
LU_HD int vw_next_one_fb(const VW<W64>& v, const VWAbove<W64>& ab, int from) { /* = vw_next_one(v, from) for from >= 0 */
    u64 x = v.w[W64 - 1];
    unsigned f = W64 * 64u;
#pragma unroll
    for (int q = W64 - 2; q >= 0; q--) { /* the nested tests leave the word `from` falls into, and what lies above it */
        const bool below = from < (q + 1) * 64;
        x = below ? v.w[q] : x;
        f = below ? ab.fb[q] : f;
    }
    const u64 y = x >> (from & 63);
    const unsigned c = lu_min(lu_ffbl((unsigned)y), lu_add_sat(lu_ffbl((unsigned)(y >> 32)), 32u));
    return (int)lu_min(lu_add_sat((unsigned)from, c), f);
}

// bit p of the result = bit (p - s) of v (bits move away from index 0), s in [0, 63]
template <int W64>
LU_HD VW<W64> vw_away0_small(const VW<W64>& v, int s) {
    VW<W64> r;
#pragma unroll
    for (int q = 0; q < W64; q++) {
        u64 lo = q > 0 ? v.w[q - 1] : 0ull;
        r.w[q] = (v.w[q] << s) | (s ? (lo >> (64 - s)) : 0ull);
    }
    return r;
}

template <int W64>
LU_HD VW<W64> vw_low_ones(int len) {
    VW<W64> r;
#pragma unroll
    for (int q = 0; q < W64; q++) {
        const int rel = len - q * 64;
        r.w[q] = rel <= 0 ? 0ull : (rel >= 64 ? ~0ull : ((1ull << rel) - 1ull));
    }
    return r;
}

template <int W64>
LU_HD void load_planes(const lu_quad* __restrict__ planes, long n, int w4, long i, VW<W64>& A0, VW<W64>& A1, VW<W64>& B0,
                       VW<W64>& B1) {
#pragma unroll
    for (int g = 0; g < (W64 + 1) / 2; g++) { /* an odd W64 takes only the low half of its last granule */
        lu_quad qa0 = {0u, 0u, 0u, 0u}, qa1 = qa0, qb0 = qa0, qb1 = qa0;
        if (g < w4) { /* a vector wider than the batch's granule count has empty upper words */
            qa0 = planes[((long)0 * w4 + g) * n + i];
            qa1 = planes[((long)1 * w4 + g) * n + i];
            qb0 = planes[((long)2 * w4 + g) * n + i];
            qb1 = planes[((long)3 * w4 + g) * n + i];
        }
        A0.w[2 * g] = (u64)qa0.x | ((u64)qa0.y << 32), A1.w[2 * g] = (u64)qa1.x | ((u64)qa1.y << 32);
        B0.w[2 * g] = (u64)qb0.x | ((u64)qb0.y << 32), B1.w[2 * g] = (u64)qb1.x | ((u64)qb1.y << 32);
        if (2 * g + 1 < W64) {
            A0.w[2 * g + 1] = (u64)qa0.z | ((u64)qa0.w << 32), A1.w[2 * g + 1] = (u64)qa1.z | ((u64)qa1.w << 32);
            B0.w[2 * g + 1] = (u64)qb0.z | ((u64)qb0.w << 32), B1.w[2 * g + 1] = (u64)qb1.z | ((u64)qb1.w << 32);
        }
    }
}

// Mismatch vector of LEAP lane d = l - mid (LV_BAG.cpp:13-18): position p = max(read idx, ref idx);
// d < 0 compares A[p-|d|] with B[p], d > 0 compares A[p] with B[p-d].  Positions where either string has
// run out (the NUL padding of LV::load_reads, LV_BAG.cpp:116-117) and all positions >= len are mismatches.
template <int W64>
LU_HD VW<W64> leap_lane_mask(const VW<W64>& A0, const VW<W64>& A1, const VW<W64>& B0, const VW<W64>& B1, const VW<W64>& VA,
                             const VW<W64>& VB, int d) {
    VW<W64> r;
    const int s = d < 0 ? -d : d;
    if (d < 0) {
        VW<W64> a0 = vw_away0_small<W64>(A0, s), a1 = vw_away0_small<W64>(A1, s), va = vw_away0_small<W64>(VA, s);
#pragma unroll
        for (int q = 0; q < W64; q++) r.w[q] = (a0.w[q] ^ B0.w[q]) | (a1.w[q] ^ B1.w[q]) | ~(va.w[q] & VB.w[q]);
    } else {
        VW<W64> b0 = vw_away0_small<W64>(B0, s), b1 = vw_away0_small<W64>(B1, s), vb = vw_away0_small<W64>(VB, s);
#pragma unroll
        for (int q = 0; q < W64; q++) r.w[q] = (A0.w[q] ^ b0.w[q]) | (A1.w[q] ^ b1.w[q]) | ~(VA.w[q] & vb.w[q]);
    }
    return r;
}

template <int K, int W64>
LU_HD int leap_unit_generic(const VW<W64>& A0, const VW<W64>& A1, const VW<W64>& B0, const VW<W64>& B1, int m, int nn) {
    constexpr int NL = 2 * K + 1;
    const int len = m > nn ? m : nn; /* benchmark_utils.h:162 */
    const VW<W64> VA = vw_low_ones<W64>(m), VB = vw_low_ones<W64>(nn);

    VW<W64> mask[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) mask[j] = leap_lane_mask<W64>(A0, A1, B0, B1, VA, VB, j - K);

    // Generation e-1 state per lane: `end` only (-2 = never reached, LV_BAG.cpp:95-101).  With o == ext (here 1 == 1) the
    // I and D tables carry no information of their own: I[l][e] is taken from end[l-1][e-o] when that is > I[l-1][e-ext],
    // else from I[l-1][e-ext] (LV_BAG.cpp:166-176) — the same generation e-1 on both sides — and end[.][g] >= I[.][g]
    // whenever I[.][g] >= 0, because a lane's start is max(end+1, I, D) (:186-201) and its end is never before its start.
    // So I[l][e] = end[l-1][e-1] + top if that end is >= 0, else -2; likewise D from lane l+1.  And since -2 + {0,1} and
    // -2 + 1 stay negative, start = max(end+1, end_up+top, end_dn+bot) needs no selects: it is negative exactly when all
    // three sources are -2.
    int en[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) en[j] = -2;
    VWAbove<W64> above[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) above[j] = vw_above<W64>(mask[j]);

    int result = -1;
    // e = 0: only the main diagonal is live in ED_GLOBAL (LV_BAG.cpp:102-104,131-147)
    {
        int e0 = vw_next_one<W64>(mask[K], 0);
        e0 = e0 > len ? len : e0;
        en[K] = e0;
        if (e0 == len) result = 0;
    }
    for (int e = 1; e <= ASM_LEAP_AF_THRESHOLD && result < 0; e++) {
        int en2[NL];
        bool pass = false;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int d = j - K;
            const int top = d >= 0 ? 1 : 0, bot = d <= 0 ? 1 : 0;
            const int e_up = j > 0 ? en[j - 1] : -2;
            const int e_dn = j < NL - 1 ? en[j + 1] : -2;
            int st = en[j] + 1;                        /* :186-187 */
            st = e_up + top > st ? e_up + top : st;    /* I_pos, :166-176,193-194 */
            st = e_dn + bot > st ? e_dn + bot : st;    /* D_pos, :179-182,200-201 */
            int enew = -2;
            if (st >= 0) {
                const int from = st > len ? len : st;
                /* count_ID_length (:9-23) as a saturating scan: first mismatch at or after `from`, capped at len; enew = max(t, st)
                 * is the reference's "a start beyond the end stays where it is" (t >= from = st whenever st <= len) */
                int t = VW_SCAN_FB(W64) ? vw_next_one_fb<W64>(mask[j], above[j], from) : vw_next_one<W64>(mask[j], from);
                t = t > len ? len : t;
                enew = t > st ? t : st;
                if (enew == len) { /* :220-238 */
                    const int diff = d < 0 ? -d : d;
                    const int conv = e + diff; /* o + (diff-1)*ext with o = ext = 1 */
                    if (conv <= ASM_LEAP_AF_THRESHOLD) pass = true;
                }
            }
            en2[j] = enew;
        }
#pragma unroll
        for (int j = 0; j < NL; j++) en[j] = en2[j];
        if (pass) result = e; /* final_ED (LV_BAG.cpp:228,356-358), not converge_ED */
    }
    return result;
}

// --------------------------------------------------------------------------------------------------------------------------
// One granule per string (W64 == 2).  The same masks, generations and result as leap_unit_generic<K, 2>, with the work the
// result does not need taken out:
//
// Lane masks, in dwords.  A 128-bit shift by the lane's constant |d| is one v_alignbit_b32 per dword.  Validity travels as the
// complements NVA = ~ones[0, m), NVB = ~ones[0, n): the shifted one is filled with ones from below, so the mask equals
// leap_lane_mask's bit for bit, and "(a0 ^ b0) | nv" is one three-input operation per dword.
//
// Generations 1..K run apart from the rest: in generation e only the lanes |d| <= e can have been reached (lane 0 in generation
// 0, one lane further out on either side per generation), every other lane has -2 on itself and on both neighbours and stays at
// -2.  Which lanes those are depends on e alone, the same for every thread.  After generation K every lane is live, and so is
// every start: the per-thread `st >= 0` test is gone with the dead lanes.
//
// No clamps in the lane step.  Every mask has all bits from the end of its lane's valid interval on set, that end is <= len,
// and an empty scan returns 128 = len when len is the full width: a scan from `from` <= len never returns more than len.  And
// st <= len + 1 (en <= len), where the scan from st and the scan from min(st, len) give the same max(t, st).  CHECK = true
// (host only: tests/test_leap_unit_host.py) evaluates both forms in every lane step and counts where they differ.
// --------------------------------------------------------------------------------------------------------------------------
struct LuDwords {
    uint32_t d[4];
};
LU_HD LuDwords lu_dwords(const VW<2>& v) {
    LuDwords r;
    r.d[0] = (uint32_t)v.w[0], r.d[1] = (uint32_t)(v.w[0] >> 32), r.d[2] = (uint32_t)v.w[1], r.d[3] = (uint32_t)(v.w[1] >> 32);
    return r;
}
// bit p of the result = bit (p - S) of v, the S bits that come in at the bottom taken from the top of `fill`; S in [1, 31]
template <int S>
LU_HD LuDwords lu_away0(const LuDwords& v, uint32_t fill) {
    static_assert(S >= 1 && S <= 31, "the shift of a lane is its distance from the main diagonal");
    LuDwords r;
    r.d[0] = lu_alignbit(v.d[0], fill, 32 - S);
#pragma unroll
    for (int q = 1; q < 4; q++) r.d[q] = lu_alignbit(v.d[q], v.d[q - 1], 32 - S);
    return r;
}
// ~ones[0, len) in dwords, len in [0, 128]
LU_HD LuDwords lu_high_ones(int len) {
    LuDwords r;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        int rel = len - 32 * q;
        rel = rel < 0 ? 0 : (rel > 32 ? 32 : rel);
        r.d[q] = (uint32_t)(0xFFFFFFFFull << rel); /* rel = 32 leaves nothing in the low dword */
    }
    return r;
}
LU_HD VW<2> lu_combine(const LuDwords& p0, const LuDwords& q0, const LuDwords& p1, const LuDwords& q1, const LuDwords& nv0,
                       const LuDwords& nv1) {
    uint32_t r[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t u = (p0.d[q] ^ q0.d[q]) | nv0.d[q];
        const uint32_t v = (p1.d[q] ^ q1.d[q]) | nv1.d[q];
        r[q] = u | v;
    }
    VW<2> o;
    o.w[0] = (u64)r[0] | ((u64)r[1] << 32), o.w[1] = (u64)r[2] | ((u64)r[3] << 32);
    return o;
}
template <int D>
LU_HD VW<2> leap_lane_mask_w2(const LuDwords& a0, const LuDwords& a1, const LuDwords& b0, const LuDwords& b1, const LuDwords& nva,
                              const LuDwords& nvb) {
    if constexpr (D < 0)
        return lu_combine(lu_away0<-D>(a0, 0u), b0, lu_away0<-D>(a1, 0u), b1, lu_away0<-D>(nva, 0xFFFFFFFFu), nvb);
    else if constexpr (D > 0)
        return lu_combine(a0, lu_away0<D>(b0, 0u), a1, lu_away0<D>(b1, 0u), nva, lu_away0<D>(nvb, 0xFFFFFFFFu));
    else
        return lu_combine(a0, b0, a1, b1, nva, nvb);
}

template <int K, int J>
struct LuMasks { /* mask[J..2K] by recursion: the lane's shift is a template argument */
    static LU_HD void fill(VW<2>* mask, const LuDwords& a0, const LuDwords& a1, const LuDwords& b0, const LuDwords& b1,
                           const LuDwords& nva, const LuDwords& nvb) {
        mask[J] = leap_lane_mask_w2<J - K>(a0, a1, b0, b1, nva, nvb);
        if constexpr (J < 2 * K) LuMasks<K, J + 1>::fill(mask, a0, a1, b0, b1, nva, nvb);
    }
};

// One lane of one generation: en_up1 / en_dn1 are the neighbours' ends with the lane's top / bot already added (-2 + {0, 1} for
// a neighbour outside the band or not reached: negative, never the maximum).  Returns the lane's new end.
template <bool CHECK>
LU_HD int lu_lane_step(const VW<2>& mask, const VWAbove<2>& above, int en_self, int en_up1, int en_dn1, int len, int* differ) {
    int st = en_self + 1;          /* :186-187 */
    st = en_up1 > st ? en_up1 : st; /* I_pos, :166-176,193-194 */
    st = en_dn1 > st ? en_dn1 : st; /* D_pos, :179-182,200-201 */
    const int t = vw_next_one_fb<2>(mask, above, st); /* count_ID_length (:9-23) */
    const int enew = t > st ? t : st; /* "a start beyond the end stays where it is" */
    if constexpr (CHECK) {
        const int from = st > len ? len : st;
        int tc = vw_next_one_fb<2>(mask, above, from);
        const bool capped = tc > len; /* statement 1: a scan from `from` <= len returns at most len */
        tc = capped ? len : tc;
        const int want = tc > st ? tc : st; /* statement 2: the scan from st gives the same end as the scan from min(st, len) */
        if (differ != nullptr && (capped || st > len + 1 || want != enew)) ++*differ;
    }
    return enew;
}

template <int K, bool CHECK = false>
LU_HD int leap_unit_w2(const VW<2>& A0, const VW<2>& A1, const VW<2>& B0, const VW<2>& B1, int m, int nn, int* differ = nullptr) {
    constexpr int NL = 2 * K + 1;
    const int len = m > nn ? m : nn; /* benchmark_utils.h:162 */
    VW<2> mask[NL];
    LuMasks<K, 0>::fill(mask, lu_dwords(A0), lu_dwords(A1), lu_dwords(B0), lu_dwords(B1), lu_high_ones(m), lu_high_ones(nn));
    VWAbove<2> above[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) above[j] = vw_above<2>(mask[j]);

    int en[NL]; /* generation e-1's end per lane, -2 = never reached: see leap_unit_generic */
#pragma unroll
    for (int j = 0; j < NL; j++) en[j] = -2;
    int result = -1;
    // e = 0: only the main diagonal is live in ED_GLOBAL (LV_BAG.cpp:102-104,131-147)
    {
        const int e0 = vw_next_one<2>(mask[K], 0);
        if constexpr (CHECK)
            if (differ != nullptr && e0 > len) ++*differ;
        en[K] = e0;
        if (e0 == len) result = 0;
    }
#define LU_GENERATION(E, REACH)                                                                              \
    {                                                                                                        \
        int en2[NL];                                                                                         \
        bool pass = false;                                                                                   \
        _Pragma("unroll") for (int j = 0; j < NL; j++) {                                                     \
            const int d = j - K, diff = d < 0 ? -d : d;                                                      \
            en2[j] = -2;                                                                                     \
            if (diff <= (REACH)) {                                                                           \
                const int up1 = (j > 0 ? en[j > 0 ? j - 1 : 0] : -2) + (d >= 0 ? 1 : 0);                     \
                const int dn1 = (j < NL - 1 ? en[j < NL - 1 ? j + 1 : j] : -2) + (d <= 0 ? 1 : 0);           \
                en2[j] = lu_lane_step<CHECK>(mask[j], above[j], en[j], up1, dn1, len, differ);               \
                if (en2[j] == len && (E) + diff <= ASM_LEAP_AF_THRESHOLD) pass = true; /* :220-238 */        \
            }                                                                                                \
        }                                                                                                    \
        _Pragma("unroll") for (int j = 0; j < NL; j++) en[j] = en2[j];                                       \
        if (pass) result = (E); /* final_ED (LV_BAG.cpp:228,356-358), not converge_ED */                     \
    }
    /* the first K generations stay one rolled loop whose lane tests (|d| <= e) are scalar branches: unrolled, its K copies of
     * the lane steps cost 70 VGPRs at K = 3 and with them the eighth wave per SIMD (62 as written) */
#pragma unroll 1
    for (int e = 1; e <= K && result < 0; e++) LU_GENERATION(e, e)
    for (int e = K + 1; e <= ASM_LEAP_AF_THRESHOLD && result < 0; e++) LU_GENERATION(e, K)
#undef LU_GENERATION
    return result;
}

template <int K, int W64>
LU_HD int leap_unit_core(const VW<W64>& A0, const VW<W64>& A1, const VW<W64>& B0, const VW<W64>& B1, int m, int nn) {
    if constexpr (W64 == 2)
        return leap_unit_w2<K>(A0, A1, B0, B1, m, nn);
    else
        return leap_unit_generic<K, W64>(A0, A1, B0, B1, m, nn);
}

template <int K, int W64>
LU_HD int leap_unit_pair(const lu_quad* __restrict__ planes, const uint32_t* __restrict__ lens, long n, int w4, long i) {
    const uint32_t ln = lens[i];
    VW<W64> A0, A1, B0, B1;
    load_planes<W64>(planes, n, w4, i, A0, A1, B0, B1);
    return leap_unit_core<K, W64>(A0, A1, B0, B1, (int)(ln & 0xffffu), (int)(ln >> 16));
}
