// The filter kernels: SIMD_ED (Levenshtein and affine mode) and the SHD pre-filter in front of the aligners.  What a thread decides
// for its pair is in asm_simd_ed.h, which also builds on the host; a kernel here computes its index, loads and clips the pair
// (simd_load_pair), calls into that core and writes one result.  Thread shapes, LDS carving, ring zeroing, fences and the quad
// reductions are the kernels' own.
#pragma once
#include "asm_kernels.h"
#include "asm_simd_ed.h"

// SIMD_ED::run_levenshtein -> event.  TT > 0: T = TT at compile time, all lane masks and the column of ends in registers
// (simd_lev_events_reg; ED_GLOBAL / SEMI_FREE_END only).  TT = 0: T at run time, lane masks rebuilt per use, the column in
// thread-private LDS [2][2T+3][threads] (simd_lev_events_col; every ed_mode).
template <int TT, int W64>
__global__ __launch_bounds__(SIMD_ED_THREADS) void simd_ed_kernel(const uint4* __restrict__ planes,
                                                                  const uint32_t* __restrict__ lens, long n, int w4, int t_rt,
                                                                  int shd_enable, int ed_mode /* ASM_LEAP_*; TT == 0 only */,
                                                                  OutMap events) {
    constexpr int NLC = TT > 0 ? 2 * TT + 1 : 1;
    extern __shared__ short s_end[];
    const int T = TT > 0 ? TT : t_rt;
    const long i = (long)blockIdx.x * SIMD_ED_THREADS + threadIdx.x;
    if (i >= n) return;
    const SimdPair<W64> p = simd_load_pair<W64>(planes, lens, n, w4, i);
    VW<W64> hm[NLC];
    if (TT > 0) {
#pragma unroll
        for (int j = 0; j < NLC; j++) hm[j] = simd_lane_mask<W64>(p, j - TT);
    }
    if (shd_enable) { /* bit_vec_filter_avx(hamming_masks + 1, buffer_length, ED_t), S3 */
        bool no;
        if constexpr (TT > 0)
            no = simd_shd_rejects<W64, NLC>(p, T, [&](int j) -> const VW<W64>& { return hm[j]; });
        else
            no = simd_shd_rejects<W64, 0>(p, T, [&](int j) { return simd_lane_mask<W64>(p, j - T); });
        if (no) {
            events.put(i, EV_REJECTED);
            return;
        }
    }
    if constexpr (TT > 0)
        events.put(i, simd_lev_events_reg<TT, W64>(p, hm));
    else
        events.put(i, simd_lev_events_col<W64>(p, T, simd_all_start(ed_mode), SimdEndColumn<SIMD_ED_THREADS>{s_end + threadIdx.x, 2 * T + 3}));
}

// SIMD_ED in affine mode, clean, one thread per pair: simd_affine_seed / simd_affine_generation over lane masks rebuilt per use;
// rings of LvRings::pow2 depths in thread-private LDS columns [slot][lane row][thread] of uint16.  -1 when the pair does not pass.
// blockDim.x threads (64, 32 or 16: whatever lets the rings fit the LDS).
template <int W64>
__global__ __launch_bounds__(64) void simd_ed_affine_kernel(const uint4* __restrict__ planes, const uint32_t* __restrict__ lens,
                                                            long n, int w4, int T, int af_t, int x, int o, int ext, int gm, int gi,
                                                            int mode /* ASM_LEAP_*: init_affine's ED_modes */, OutMap out) {
    extern __shared__ uint16_t s_afring[]; /* `end` [gm][rows][TH], I [gi][rows][TH], D [gi][rows][TH] */
    const int TH = (int)blockDim.x, t = threadIdx.x;
    const int rows = 2 * T + 3, slot = rows * TH;
    const LvRings rg{gm, gi};
    const SimdAffine a{T, af_t, x, o, ext, mode};
    const SimdAffineRings<uint16_t> r{s_afring + t, s_afring + t + gm * slot, s_afring + t + (gm + gi) * slot, rg, slot, TH};
    {
        const int words = (int)(rg.ring_bytes(rows, TH, sizeof(uint16_t)) / 4);
        uint32_t* const base = reinterpret_cast<uint32_t*>(s_afring);
        for (int w = t; w < words; w += TH) base[w] = 0u;
    }
    __syncthreads();
    const long i = (long)blockIdx.x * TH + t;
    if (i >= n) return;
    const SimdPair<W64> p = simd_load_pair<W64>(planes, lens, n, w4, i);
    const auto extend = [&](int d, int st) { return simd_extend<W64>(simd_lane_mask<W64>(p, d), st, p.len); };
    int result = simd_affine_seed(r, a, p.len, 0, 1, extend) ? a.exact() : -2; /* -2: still running */
    for (int e = 1; e <= af_t; e++) {
        if (__ballot(result == -2) == 0ull) break;
        if (result != -2) continue;
        const int conv = simd_affine_generation(r, a, p.len, e, 0, 1, extend);
        if (conv != SIMD_AF_NONE) result = conv;
    }
    out.put(i, result == -2 ? -1 : result);
}

// The same recurrence with FOUR THREADS PER PAIR, sixteen pairs per wave, for strings of at most 128 characters (one 128-bit
// half: none of the half-by-half shift effects of the 256-bit form) — the shape leap_quad_kernel gave LV::run (asm_wave.h):
// the live lanes of a generation are dealt round-robin to the quad (lane0 = q, step 4), rings [slot][lane row][pair] of bytes
// (end + 2 <= 130) and the pair's four planes in LDS (simd_quad_stage); a wave-scope fence between generations.  Against one
// thread per pair the LDS a wave needs shrinks by four (gap 30, (2,3,1): 8 KB per wave instead of 61), which is what bounds the
// occupancy there, and a wave waits for the slowest of 16 pairs instead of 64.
ASM_DEV int quad_min(int v) {
    int w = __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false); /* quad_perm [1,0,3,2] */
    v = w < v ? w : v;
    w = __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false); /* quad_perm [2,3,0,1] */
    return w < v ? w : v;
}

__global__ __launch_bounds__(64) void simd_ed_affine_quad_kernel(const uint4* __restrict__ planes, const uint32_t* __restrict__ lens,
                                                                 long n, int w4, int T, int af_t, int x, int o, int ext, int gm,
                                                                 int gi, int mode /* as simd_ed_affine_kernel */, OutMap out) {
    constexpr int P = 16, PD = SIMD_QUAD_PD, PW = SIMD_QUAD_PW;
    typedef uint8_t EnT;
    extern __shared__ uint32_t s_afq[];
    const int t = threadIdx.x, pr = t >> 2, q = t & 3;
    const int rows = 2 * T + 3, slot = rows * P;
    const LvRings rg{gm, gi};
    const SimdAffine a{T, af_t, x, o, ext, mode};
    uint32_t* const pl = s_afq + pr * PW;                             /* [P][4][PD] (+1) */
    EnT* const r_en = reinterpret_cast<EnT*>(s_afq + P * PW) + pr;   /* [gm][rows][P], then I and D [gi][rows][P] */
    const SimdAffineRings<EnT> r{r_en, r_en + gm * slot, r_en + (gm + gi) * slot, rg, slot, P};
    {
        const int ring_words = (int)(rg.ring_bytes(rows, P, sizeof(EnT)) / 4);
        uint32_t* const base = s_afq + P * PW;
        for (int w = t; w < ring_words; w += 64) base[w] = 0u;
    }
    const long i = (long)blockIdx.x * P + pr;
    const bool live = i < n;
    int len = 0;
    if (live) { /* thread q of the quad stages plane q: read plane 0/1, reference plane 0/1 */
        const SimdClip c = simd_clip(lens[i], 128);
        len = c.len;
        simd_quad_stage(pl + q * PD, planes[((long)q * w4) * n + i], q < 2 ? c.len : c.ref);
    }
    leap_quad_fence();
    const auto extend = [&](int d, int st) { return simd_quad_extend(pl, d, st, len); };
    int result = live ? -2 : 0; /* -2: still running */
    const int exact = quad_or(live && simd_affine_seed(r, a, len, q, 4, extend) ? 1 : 0);
    if (live && exact) result = a.exact();
    leap_quad_fence();
    for (int e = 1; e <= af_t; e++) {
        if (__ballot(result == -2) == 0ull) break;
        const int conv = quad_min(result == -2 ? simd_affine_generation(r, a, len, e, q, 4, extend) : SIMD_AF_NONE);
        if (conv != SIMD_AF_NONE && result == -2) result = conv;
        leap_quad_fence();
    }
    if (live && q == 0) out.put(i, result == -2 ? -1 : result);
}

// init_affine's SHD_enable / SHD_threshold (SIMD_ED.cpp:435,445-446): run_affine starts with bit_vec_filter_avx(hamming_masks + 1,
// buffer_length, SHD_threshold) (:489-492), the mask-array filter of simd_ed_kernel (S3) over the FIRST 2*SHD_threshold+1 lane
// masks — lanes -gap .. -gap + 2*SHD_threshold: centred on the main lane only when SHD_threshold equals the gap threshold.  A
// rejected pair does not pass and nothing else changes, so this runs as a second, cheap kernel behind the affine one and
// overwrites the verdicts of the pairs it rejects.
template <int W64>
__global__ __launch_bounds__(ASM_BLOCK) void simd_affine_shd_kernel(const uint4* __restrict__ planes, const uint32_t* __restrict__ lens,
                                                                    long n, int w4, int gap_t, int shd_t, OutMap out) {
    const long i = (long)blockIdx.x * ASM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const SimdPair<W64> p = simd_load_pair<W64>(planes, lens, n, w4, i);
    if (simd_shd_rejects<W64, 0>(p, shd_t, [&](int j) { return simd_lane_mask<W64>(p, j - gap_t); })) out.put(i, -1);
}

// events -> verdicts, in place: clean, and ED_modes LOCAL / SEMI_FREE_END
__global__ __launch_bounds__(ASM_BLOCK) void simd_ed_clean_kernel(int32_t* __restrict__ ev_to_ed, long n, int T) {
    const long i = (long)blockIdx.x * ASM_BLOCK + threadIdx.x;
    if (i < n) ev_to_ed[i] = simd_verdict_clean(ev_to_ed[i], T);
}
__global__ __launch_bounds__(ASM_BLOCK) void simd_ed_final_kernel(int32_t* __restrict__ ev_to_ed, long n) {
    const long i = (long)blockIdx.x * ASM_BLOCK + threadIdx.x;
    if (i < n) ev_to_ed[i] = simd_verdict_final(ev_to_ed[i]);
}
// sequential mode: setter keys; after their last-setter scan the converge keys; after theirs the verdicts
__global__ __launch_bounds__(ASM_BLOCK) void simd_ed_setter_kernel(const int32_t* __restrict__ ev, long n,
                                                                   int32_t* __restrict__ key) {
    const long i = (long)blockIdx.x * ASM_BLOCK + threadIdx.x;
    if (i < n) key[i] = simd_setter_key(ev[i]);
}
__global__ __launch_bounds__(ASM_BLOCK) void simd_ed_converge_kernel(const int32_t* __restrict__ ev,
                                                                     const int32_t* __restrict__ state_after, long n,
                                                                     int init_fe, int init_fd, int32_t* __restrict__ conv_key) {
    const long i = (long)blockIdx.x * ASM_BLOCK + threadIdx.x;
    if (i < n) conv_key[i] = simd_converge_key(ev[i], state_after[i], init_fe, init_fd);
}
__global__ __launch_bounds__(ASM_BLOCK) void simd_ed_verdict_kernel(int32_t* __restrict__ ev_to_ed,
                                                                    const int32_t* __restrict__ conv_after, long n, int T,
                                                                    int init_conv) {
    const long i = (long)blockIdx.x * ASM_BLOCK + threadIdx.x;
    if (i < n) ev_to_ed[i] = simd_verdict_sequential(ev_to_ed[i], i > 0 ? conv_after[i - 1] : -1, conv_after[i], T, init_conv);
}

// SHD on the planes: bit_vec_filter_avx(read0, read1, ref0, ref1, length, max_error) (SHD.cpp:241-322)
template <int W64>
__global__ __launch_bounds__(ASM_BLOCK) void shd_kernel(const uint4* __restrict__ planes, const uint32_t* __restrict__ lens,
                                                        long n, int w4, int max_error, OutMap out) {
    const long i = (long)blockIdx.x * ASM_BLOCK + threadIdx.x;
    if (i < n) out.put(i, shd_pass<W64>(simd_load_pair<W64>(planes, lens, n, w4, i), max_error) ? 1 : 0);
}
