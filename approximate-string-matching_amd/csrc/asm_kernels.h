// HIP kernels of the batched pair aligner for MI355X (gfx950, wave64).
//
// Data layout in HBM: a batch of n pairs is held as
//   planes : uint4[4][w4][n]   plane p in {A.bit0, A.bit1, B.bit0, B.bit1}, granule g = positions
//                              [128g, 128g+128), pair i at planes[(p*w4+g)*n + i]  (bit q of a granule <->
//                              character 128g+q; codes A=00 C=01 G=10 T=11, anything else 00 — the code of
//                              GASMA/bit_convert.cpp:340-355)
//   lens   : uint32[n]         m | n << 16
// so that thread i of a wave reads 16 contiguous bytes next to thread i+1's: every load instruction of a
// thread-per-pair kernel is one fully coalesced 1 KiB request.
//
// Work decomposition: ONE THREAD PER READ PAIR for the narrow band (k <= 7, the benchmark's k = 3): the
// 2k+1 lanes of the band live in registers, the lane loops are fully unrolled, no cross-lane traffic, and
// every VALU lane does useful work (a wave-per-pair mapping would idle 57 of 64 lanes at k = 3).  Wide bands
// (k up to 50) use the block-per-pair kernels further down (thread = band lane).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "asm_affine.h"
#include "asm_bits.h"
#include "asm_gen.h"
#include "asm_greedy_lane.h"
#include "asm_leapunit.h"
#include "asm_nwband.h"
#include "asm_pack.h"

#include "asm_limits.h" /* ASM_BLOCK and the other shapes the dispatch reads too */

// --------------------------------------------------------------------------------------------------------
// Pack: ASCII -> bit planes.  Device counterpart of sse3_convert2bit1 (GASMA/bit_convert.cpp:248-369), minus
// its in-place byte permutation (whose only observable effect, the stale tails of later pairs, is supplied
// through `tails` in sequential mode — see asm_tails.h).
//
// A workgroup owns 256 consecutive pairs.  Their ASCII is one contiguous byte range of the batch per side, and the
// conversion is a function of the byte alone, so it is done where the bytes land: thread t loads 16-byte vector v of
// the range (fully coalesced) and turns it into bits [16v, 16v+16) of two plane arrays in LDS, in buffer-position
// coordinates (bit q of plane dword j <-> byte 32j+q of the range).  After one barrier thread t cuts pair t's string
// out of those arrays with one funnel shift per output dword.  LDS holds 2 bits per byte; when the block's planes do
// not fit (long strings), each side is done in rounds of whole pairs that do.
// --------------------------------------------------------------------------------------------------------
#ifndef PACK_BLOCK
#define PACK_BLOCK 256 /* pairs (threads) per pack workgroup */
#endif
#define PACK_LDS_MAX (33 * 1024) /* plane bytes per workgroup: one side of 256 strings of ASM_MAX_LENGTH (32 784 B) fits */
#define PACK_UNROLL 8            /* 16-byte vectors a thread keeps in flight */

// Length buckets of a batch (mixed-length batches are grouped by the number of 128-position granules their longer
// string needs, so that every kernel launch works on pairs of one width class).  Bucket b holds the pairs at slots
// [start[b], start[b+1]) of the bucketed order; its planes are a uint4[4][w4[b]][size] block at plane_off[b].
struct PackBuckets {
    int nb;
    int w4[4];
    long start[5];
    long plane_off[4];
};

ASM_DEV uint32_t pack_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); } /* x is the same in every thread */

// Converts the vectors of the two ranges into plane arrays: A's plane 0 / plane 1 at u16 offsets 0 / 2*pdA, B's at 4*pdA /
// 4*pdA + 2*pdB (pd = dwords per plane array).  Loads are issued PACK_UNROLL at a time, both sides in one loop.  Everything but t is
// workgroup-uniform and the caller passes it from scalar registers.  The loop counts vectors with B's first one moved up to a
// multiple of 64, so a wave's 64 vectors are always on one side: which side, the source pointer, the plane offsets, the number of
// live threads and the loop itself are scalar work, and a thread is left with one add per address and one compare.
ASM_DEV void pack_convert_range(uint16_t* sp, const uint4* __restrict__ srcA, int nvA, int pdA, const uint4* __restrict__ srcB,
                                int nvB, int pdB, int t) {
    const int startB = (nvA + 63) & ~63, tot = startB + nvB;
    const int w0 = __builtin_amdgcn_readfirstlane(t); /* the wave's first thread */
    const int lane = t - w0;
    const uint32_t lane16 = 16u * (uint32_t)lane;
    uint16_t* const spl = sp + lane;
#pragma unroll 1
    for (int base = 0; base < tot; base += PACK_UNROLL * PACK_BLOCK) {
        uint4 r[PACK_UNROLL];
#pragma unroll
        for (int q = 0; q < PACK_UNROLL; q++) {
            const int wv = base + q * PACK_BLOCK + w0; /* the wave's first vector: a multiple of 64 */
            if (wv < tot) {
                const bool sideA = wv < startB;
                const uint4* src = sideA ? srcA + wv : srcB + (wv - startB);
                if (lane < (sideA ? nvA : tot) - wv) r[q] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(src) + lane16);
            }
        }
#pragma unroll
        for (int q = 0; q < PACK_UNROLL; q++) {
            const int wv = base + q * PACK_BLOCK + w0;
            if (wv < tot) {
                uint32_t p0, p1;
                pack_vec(r[q], p0, p1);
                const bool sideA = wv < startB;
                const int at = sideA ? wv : 4 * pdA + (wv - startB);
                if (lane < (sideA ? nvA : tot) - wv) {
                    spl[at] = (uint16_t)p0;
                    spl[at + 2 * (sideA ? pdA : pdB)] = (uint16_t)p1;
                }
            }
        }
        // every load of this turn has been used: said aloud, or the next turn's first address waits for loads it takes to be pending
        __builtin_amdgcn_s_waitcnt(0x0f70); /* vmcnt(0) */
    }
}

// One thread cuts its string (byte offset `off` into the converted range, `len` characters) out of the plane arrays
// P0 / P1 (pack_cut_begin, pack_cut_granule: asm_pack.h) and stores its granules.
template <int W4>
ASM_DEV void pack_extract(const uint32_t* P0, const uint32_t* P1, uint32_t off, int len, int w4, int s,
                          const uint4* __restrict__ tails, long n, long pair, uint4* __restrict__ bplanes, long bn, long local) {
    PackCut c = pack_cut_begin(P0, P1, off, len);
#pragma unroll
    for (int g = 0; g < W4; g++) {
        if (g < w4) {
            uint4 v0, v1;
            pack_cut_granule(P0, P1, c, len, g, v0, v1);
            if (tails != nullptr && g == 0) {
                const uint4 t0 = tails[(long)(2 * s) * n + pair], t1 = tails[(long)(2 * s + 1) * n + pair];
                v0.x |= t0.x, v0.y |= t0.y, v0.z |= t0.z, v0.w |= t0.w;
                v1.x |= t1.x, v1.y |= t1.y, v1.z |= t1.z, v1.w |= t1.w;
            }
            bplanes[((long)(2 * s) * w4 + g) * bn + local] = v0;
            bplanes[((long)(2 * s + 1) * w4 + g) * bn + local] = v1;
        }
    }
}

template <int W4>
__global__ __launch_bounds__(PACK_BLOCK) void pack_kernel(const char* __restrict__ reads,
                                                         const uint32_t* __restrict__ read_off,
                                                         const char* __restrict__ refs,
                                                         const uint32_t* __restrict__ ref_off,
                                                         const uint4* __restrict__ tails, /* [4][n] or null */
                                                         uint4* __restrict__ planes, uint32_t* __restrict__ lens,
                                                         long n, PackBuckets pb,
                                                         const uint32_t* __restrict__ pos /* pair -> slot, or null */,
                                                         uint32_t lds_dwords /* dynamic LDS (plane arrays), in dwords */) {
    // plane arrays sized by the host from the batch's longest string: short reads leave room for more resident workgroups
    extern __shared__ uint32_t s_pl[];
    __shared__ uint32_t s_off[2][PACK_BLOCK + 1];
    const int t = threadIdx.x;
    const long p0 = (long)blockIdx.x * PACK_BLOCK;
    const int np = (n - p0) < PACK_BLOCK ? (int)(n - p0) : PACK_BLOCK;
    uint16_t* const sp = reinterpret_cast<uint16_t*>(s_pl);
    // where this thread's pair lives in the bucketed layout
    const long slot = (t < np) ? (pos ? (long)pos[p0 + t] : p0 + t) : 0;
    int bk = 0;
#pragma unroll
    for (int q = 1; q < 4; q++)
        if (q < pb.nb && slot >= pb.start[q]) bk = q;
    const int w4 = pb.w4[bk];
    const long bn = pb.start[bk + 1] - pb.start[bk], local = slot - pb.start[bk];
    uint4* bplanes = planes + pb.plane_off[bk];

    // both offset tables up front: one global round trip instead of two
    s_off[0][t] = read_off[p0 + (t < np ? t : np)];
    s_off[1][t] = ref_off[p0 + (t < np ? t : np)];
    if (t == 0) s_off[0][PACK_BLOCK] = read_off[p0 + np], s_off[1][PACK_BLOCK] = ref_off[p0 + np];
    __syncthreads();
    const uint32_t oA0 = s_off[0][t], oA1 = s_off[0][t + 1], oB0 = s_off[1][t], oB1 = s_off[1][t + 1];
    // the block's ranges are the same in every thread: kept in scalar registers (pack_convert_range)
    const uint32_t baseA = pack_uniform(s_off[0][0] & ~15u), baseB = pack_uniform(s_off[1][0] & ~15u);
    const int nvA = (int)((pack_uniform(s_off[0][PACK_BLOCK]) - baseA + 15u) >> 4);
    const int nvB = (int)((pack_uniform(s_off[1][PACK_BLOCK]) - baseB + 15u) >> 4);
    const int pdA = pack_plane_dwords(nvA), pdB = pack_plane_dwords(nvB);
    if (t < np) lens[slot] = (oA1 - oA0) | ((oB1 - oB0) << 16);

    if (2 * (pdA + pdB) <= (int)lds_dwords) {
        // Fast path: both sides of the whole block in one pass, one barrier
        pack_convert_range(sp, reinterpret_cast<const uint4*>(reads + baseA), nvA, pdA,
                           reinterpret_cast<const uint4*>(refs + baseB), nvB, pdB, t);
        __syncthreads();
        if (t < np) {
            pack_extract<W4>(s_pl, s_pl + pdA, oA0 - baseA, (int)(oA1 - oA0), w4, 0, tails, n, p0 + t, bplanes, bn, local);
            pack_extract<W4>(s_pl + 2 * pdA, s_pl + 2 * pdA + pdB, oB0 - baseB, (int)(oB1 - oB0), w4, 1, tails, n, p0 + t,
                             bplanes, bn, local);
        }
        return;
    }
    // Rounds: one side at a time, whole pairs whose planes fit.  The host sizes the LDS for at least one string.
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const char* str = s ? refs : reads;
        const uint32_t o0 = s ? oB0 : oA0, o1 = s ? oB1 : oA1;
        const int len = (int)(o1 - o0);
        int ps = 0;
        while (ps < np) { /* uniform across the workgroup */
            __syncthreads();
            const uint32_t base = pack_uniform(s_off[s][ps] & ~15u);
            const int fits = (t >= ps && t < np && 2 * pack_plane_dwords((int)((o1 - base + 15u) >> 4)) <= (int)lds_dwords) ? 1 : 0;
            const int pe = ps + __syncthreads_count(fits); /* offsets are monotone: the fitting pairs are [ps, pe) */
            const int nv = (int)((pack_uniform(s_off[s][pe]) - base + 15u) >> 4), pd = pack_plane_dwords(nv);
            const uint4* src = reinterpret_cast<const uint4*>(str + base);
            pack_convert_range(sp, src, nv, pd, src, 0, pd, t); /* B empty (a null B pointer crashes ROCm 7.2's inliner) */
            __syncthreads();
            if (t >= ps && t < pe) pack_extract<W4>(s_pl, s_pl + pd, o0 - base, len, w4, s, tails, n, p0 + t, bplanes, bn, local);
            ps = pe;
        }
    }
}

// width class of every pair (granules of the longer string, minus one) and the class histogram
__global__ __launch_bounds__(ASM_BLOCK) void classify_kernel(const uint32_t* __restrict__ read_off,
                                                             const uint32_t* __restrict__ ref_off, long n,
                                                             uint8_t* __restrict__ cls, uint32_t* __restrict__ idx,
                                                             unsigned int* __restrict__ counts /* [4] */) {
    __shared__ unsigned int s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint32_t m = read_off[i + 1] - read_off[i], nn = ref_off[i + 1] - ref_off[i];
        uint32_t L = m > nn ? m : nn;
        L = L < 1u ? 1u : L;
        uint32_t c = (L + 127u) / 128u - 1u;
        c = c > 3u ? 3u : c;
        cls[i] = (uint8_t)c;
        idx[i] = (uint32_t)i;
        atomicAdd(&s_cnt[c], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(ASM_BLOCK) void invert_order_kernel(const uint32_t* __restrict__ order, long n,
                                                                 uint32_t* __restrict__ pos) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) pos[order[j]] = (uint32_t)j;
}

// --------------------------------------------------------------------------------------------------------
// Greedy hurdle-matrix aligner (hurdle_matrix<int_128bit>), general form: GreedyArgs and every rule of its step are in
// asm_greedy_lane.h (host-buildable: host/greedy_host_check.cpp); the kernels in asm_wave.h, asm_group.h and asm_wide.h hold the
// mapping of band lanes to threads and the reductions.  The k <= 3 straight-line form is asm_greedy3.h.
// greedy_persist_kernel below takes GreedyArgs, the significance, the lane vectors, the start column, the switch cost and the hurdle count
// from that header and holds the rest of the step written out:
// its 32 instantiations sit at the edge of the register file (K = 8-10 are held at two waves per SIMD by launch bounds), and on the
// shared functions the unit-penalty instantiations allocate more registers and K = 10 spills (table in profiles/greedy_lane_ab.txt).
// Shape (a) of host/greedy_host_check.cpp has the same serial structure but does not execute this kernel's text: a change to a rule is
// made here as well as in the header.

// A V128 held by another lane of the wave, word by word through the caller's 32-bit fetch (v_readlane, ds_bpermute)
template <class Fetch32>
ASM_DEV V128 v_fetch_lane(V128 v, Fetch32 fetch) {
    return v_make((u64)(unsigned)fetch((int)(unsigned)v.lo) | ((u64)(unsigned)fetch((int)(v.lo >> 32)) << 32),
                  (u64)(unsigned)fetch((int)(unsigned)v.hi) | ((u64)(unsigned)fetch((int)(v.hi >> 32)) << 32));
}
// --------------------------------------------------------------------------------------------------------

// Wave-local work queue for the persistent kernels: every wave owns a contiguous slice [q_next, q_end) of the batch
// (static split over the resident waves: ~n/3000 pairs each, so slices are balanced to a few percent) and its lanes pull
// the next pair with wave-level bit tricks only — no memory atomics (a single global queue head saturates at ~88
// dequeues/us on this chip, far below the refill rate of these kernels).
// Measured dead end (C2, 10^6 pairs, 3072 waves, ~120 us): drawing chunks of pairs from counters in device memory instead —
// one counter, or eight per-XCD-group counters 128 B or 8 KB apart, with a static first chunk and stealing between groups —
// costs ~7 ns of kernel time per draw whatever the layout (chunks of 16 / 64 / 256 pairs: 0.56 / 0.19 / 0.13 ms against 0.12):
// the kernel hands out 8 pairs per nanosecond, and a wave stalls for two memory-side round trips per draw.  The wave-per-pair
// kernels, where a chunk of 16 pairs lasts a wave ~100 us, do use such a queue (PairQueue, asm_wave.h).
struct WaveQueue {
    long next, end;
    ASM_DEV void init(long n) {
        const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
        next = n * wave / nwaves;
        end = n * (wave + 1) / nwaves;
    }
    // lanes with need=true receive consecutive indices; returns -1 when the slice is used up
    ASM_DEV long pull(bool need) {
        const unsigned long long mask = __ballot(need);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        const long cnt = (long)__popcll(mask);
        const long avail = end - next;
        const long idx = (need && rank < avail) ? next + rank : -1;
        next += cnt < avail ? cnt : avail;
        return idx;
    }
};

// --------------------------------------------------------------------------------------------------------
// Persistent, lane-refilling thread-per-pair Greedy kernel.  Pairs need 1..7 steps each (mean ~2 at err 0.10); with one
// pair per thread a wave runs as long as its slowest pair and the other lanes idle.  Here a wave keeps all 64
// lanes busy: whenever a lane's pair terminates it writes the result and pulls the next pair index from a global
// wave-local queue (WaveQueue above), so every pass of the step body works on 64 live pairs.  The grid is sized to
// what is resident (CUs x occupancy), not to n.
// --------------------------------------------------------------------------------------------------------
// K = 8, 9 (and 10 with unit penalties) fit 256 registers without scratch when asked to; left alone the allocator spreads into
// the AGPR half and the kernel runs at one wave per SIMD instead of two.
#ifndef GREEDY_PERSIST_MIN_WAVES
#define GREEDY_PERSIST_MIN_WAVES(K, UNIT) (((K) == 8 || (K) == 9 || ((K) == 10 && (UNIT))) ? 2 : 1)
#endif
template <int K, bool UNIT> /* UNIT: x = o = e = 1 known at compile time (the benchmark's penalties): the multiplies fold away */
__global__ __launch_bounds__(ASM_BLOCK, GREEDY_PERSIST_MIN_WAVES(K, UNIT)) void greedy_persist_kernel(const uint4* __restrict__ planes,
                                                                   const uint32_t* __restrict__ lens, long n, int w4,
                                                                   GreedyArgs args, OutMap out,
                                                                   CigarSink cig, int refill_min) {
    constexpr int NL = 2 * K + 1;
#ifndef ASM_PERSIST_KEEP_LF
#define ASM_PERSIST_KEEP_LF 5 /* largest K whose flipped lane vectors stay in registers; above it they are rebuilt per look-up */
#endif
    constexpr bool KEEP_LF = K <= ASM_PERSIST_KEEP_LF;
    constexpr int NLF = KEEP_LF ? NL : 1;
    const int x = UNIT ? 1 : args.x, o = UNIT ? 1 : args.o, e = UNIT ? 1 : args.e;
    const bool semi = UNIT ? false : args.semi != 0; /* the UNIT instantiation is GLOBAL only */
    V128 lo_[NL], lf_[NLF];
    int sp[NL], len[NL], nsw[NL], dst[NL], sw[NL], nh[NL];
    V128 dest_vec = v_make(0, 0);
    int m = 0, nn = 0, dest_lane = 0, cur_lane = 0, cur_col = 0, cost = 0, guard = 0, ncig = 0;
    long idx = -1, pair = 0;
    bool active = false, finished = true, exhausted = false;
    WaveQueue wq;
    wq.init(n);
#pragma unroll
    for (int j = 0; j < NL; j++) {
        lo_[j] = v_make(0, 0);
        if (KEEP_LF) lf_[j] = v_make(0, 0);
        sp[j] = -1, len[j] = 0, nsw[j] = 128, dst[j] = 0, sw[j] = nh[j] = 0;
    }
#ifdef GREEDY_DIAG
    unsigned long long dg_refill = 0, dg_step = 0, dg_iters = 0, dg_refills = 0, dg_lanes = 0, dg_t0 = __builtin_amdgcn_s_memtime();
#endif
    for (;;) {
#ifdef GREEDY_DIAG
        const unsigned long long dg_a = __builtin_amdgcn_s_memtime();
#endif
        const bool need = finished && !exhausted;
        // Refill lazily: the setup below costs about as much as a step, so wait until `refill_min` lanes are idle
        // (or nothing else is left to do) before paying for it.
        const unsigned long long need_mask = __ballot(need);
        if (need_mask != 0ull && (__popcll(need_mask) >= refill_min || __ballot(active && !finished) == 0ull)) {
            if (need && active) {
                // ---- final hop (hurdle_matrix.h:575-590) ----
                const int dest_col = lane_destination(m, nn, dest_lane);
                if (cur_lane != dest_lane || cur_col < dest_col) {
                    const int sw_f = semi ? 0 : lane_penalty(cur_lane, dest_lane, o, e);
                    const int distance = v_pop_between(dest_vec, cur_col + fwd_col(cur_lane, dest_lane), dest_col);
                    const int hc = x * distance;
                    cost += sw_f + (hc > 0 ? hc : 0);
                    if (cig.on()) cig.step(pair, ncig, cur_lane, dest_lane, distance);
                }
                if (cig.on()) cig.finish(pair, ncig);
                out.put(idx, cost);
            }
            const long got = wq.pull(need);
            if (need) {
                idx = got;
                active = got >= 0;
                exhausted = !active;
            }
            if (need && active) {
                const V128 A0 = v_from_uint4(planes[((long)0 * w4) * n + idx]);
                const V128 A1 = v_from_uint4(planes[((long)1 * w4) * n + idx]);
                const V128 B0 = v_from_uint4(planes[((long)2 * w4) * n + idx]);
                const V128 B1 = v_from_uint4(planes[((long)3 * w4) * n + idx]);
                const uint32_t ln = lens[idx];
                m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
                m = m > 128 ? 128 : m; /* hurdle_matrix.h:626-627 */
                nn = nn > 128 ? 128 : nn;
                dest_lane = nn - m; /* hurdle_matrix.h:649 */
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int lane = j - K;
                    lo_[j] = greedy_lane_vector(A0, A1, B0, B1, lane);
                    if (KEEP_LF) lf_[j] = v_flip_short_hurdles1(lo_[j]);
                    sp[j] = -1; /* hurdle_matrix.h:106-119 */
                    len[j] = 0;
                    nsw[j] = 128;
                    dst[j] = lane_destination(m, nn, lane);
                }
                dest_vec = greedy_lane_vector(A0, A1, B0, B1, dest_lane); /* may lie outside the band (G13) */
                cur_lane = 0, cur_col = 0, cost = 0, guard = 0, ncig = 0;
                pair = out.index(idx);
                finished = false;
            }
        }
#ifdef GREEDY_DIAG
        const unsigned long long dg_b = __builtin_amdgcn_s_memtime();
        dg_refill += dg_b - dg_a;
        dg_iters++;
        dg_lanes += __popcll(__ballot(active && !finished));
#endif
        if (__ballot(active && !finished) == 0ull) break; /* wave-uniform: every lane has drained the queue */
        if (active && !finished) {
            // ---- _update_highway_list ----
            bool reaching = false;
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int lane = j - K;
                const int start_col = greedy_start_col(cur_lane, cur_col, lane);
                if (sp[j] < start_col) {
                    int d = lane - cur_lane;
                    nsw[j] = d < 0 ? -d : d;
                    int fz, nx;
                    v_highway_from(KEEP_LF ? lf_[j] : v_flip_short_hurdles1(lo_[j]), start_col, fz, nx);
                    sp[j] = start_col + fz;
                    len[j] = nx;
                    if (start_col + fz + nx > dst[j]) {
                        const int c = dst[j] - (start_col + fz);
                        len[j] = c > 0 ? c : 0;
                        reaching = true;
                    }
                }
                sw[j] = greedy_switch_cost(semi && guard == 0, cur_lane, lane, o, e);
                nh[j] = greedy_hurdles(lo_[j], start_col, sp[j], len[j]);
            }
            double best_h = -__builtin_inf();
            int best_leap = 0; /* -numeric_limits<int>::infinity() == 0 (hurdle_matrix.h:287) */
            int best = 0, best_sp = sp[K], best_len = len[K], best_cost = x * nh[K] + sw[K];
            V128 best_vec = lo_[K];
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int lane = j - K;
                const int hc = x * nh[j];
                double heur = greedy_significance(args, len[j], nh[j], nsw[j]);
                int leap = -sw[j];
                if (reaching) {
                    const int fsw = semi ? 0 : lane_penalty(lane, dest_lane, o, e);
                    heur = (double)(-sw[j] - hc - fsw - x * (dst[j] - sp[j] - len[j]));
                    leap -= fsw;
                }
                if (heur > best_h || (heur == best_h && leap > best_leap)) {
                    best_h = heur, best_leap = leap, best = lane;
                    best_sp = sp[j], best_len = len[j], best_cost = hc + sw[j], best_vec = lo_[j];
                }
            }
            if (best_len <= 0 || ++guard > 4 * 128) { /* hurdle_matrix.h:358-361 */
                finished = true;
            } else {
                // ---- _choose_best_highway ----
                const int best_from_sp = v_ones_from(best_vec, best_sp);
                int small_inter = best_cost, small_total = best_cost;
                int ch = best, ch_sp = best_sp, ch_len = best_len, ch_cost = best_cost;
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int lane = j - K;
                    if (lane != best && !(sp[j] + fwd_col(lane, best) > best_sp)) {
                        const int endp = sp[j] + len[j];
                        const int inter = sw[j] + nh[j]; /* the same range loop 1 counted: [cur_col + fwd, sp + len) */
                        const int tail = x * v_pop_between_pre(best_vec, fwd_col(lane, best) + endp, best_sp, best_from_sp);
                        const int total = inter + lane_penalty(lane, best, o, e) + (tail > 0 ? tail : 0);
                        if (total <= small_total && inter <= small_inter) {
                            small_total = total, small_inter = inter;
                            ch = lane, ch_sp = sp[j], ch_len = len[j], ch_cost = sw[j] + x * nh[j];
                        }
                    }
                }
                // ---- _step commit (hurdle_matrix.h:411-433) ----
                cost += ch_cost;
                if (cig.on()) cig.step(pair, ncig, cur_lane, ch, ch_sp + ch_len - (cur_col + fwd_col(cur_lane, ch)));
                cur_lane = ch;
                cur_col = ch_sp + ch_len;
                if (cur_col >= lane_destination(m, nn, ch)) finished = true;
            }
        }
#ifdef GREEDY_DIAG
        dg_step += __builtin_amdgcn_s_memtime() - dg_b;
#endif
    }
#ifdef GREEDY_DIAG
    if ((threadIdx.x & 63) == 0 && cig.nops != nullptr && cig.ops == nullptr) { /* diag build: cig.nops doubles as the debug buffer */
        unsigned long long* dbg = reinterpret_cast<unsigned long long*>(cig.nops) + 8 * (((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
        dbg[0] = dg_refill, dbg[1] = dg_step, dbg[2] = dg_iters, dbg[3] = dg_lanes, dbg[4] = __builtin_amdgcn_s_memtime() - dg_t0;
    }
#endif
}

// --------------------------------------------------------------------------------------------------------
// LEAP (banded affine Landau-Vishkin, "BAG"), unit penalties x = o = e = 1, lanes in registers, one thread
// per pair: leap_unit_pair, with the word vectors VW / vw_* and leap_lane_mask that the other LEAP kernels
// below share, is in asm_leapunit.h (host-buildable: host/leap_host_check.cpp).
// --------------------------------------------------------------------------------------------------------

template <int K, int W64>
__global__ __launch_bounds__(ASM_BLOCK) void leap_unit_kernel(const uint4* __restrict__ planes,
                                                              const uint32_t* __restrict__ lens, long n, int w4,
                                                              OutMap out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out.put(i, leap_unit_pair<K, W64>(planes, lens, n, w4, i));
}

// Work-sorted form.  A pair needs final_ED + 1 generations, and a wave runs as long as its slowest pair: with pairs in
// input order a wave of 64 runs ~16 generations for a mean of ~8.  When a per-pair work estimate is at hand — the NW
// penalty of the same pair, computed one kernel earlier in `_run_benchmark`, is within one generation of LEAP's count
// for ~98 % of pairs — each workgroup counting-sorts its 256 pairs by that hint in LDS and thread t takes the pair of
// rank t, so each of the four waves works on one quartile of the workgroup's pairs, i.e. on 64 pairs that need
// (nearly) the same number of generations.  The hint only changes the schedule, never a result.
template <int K, int W64>
__global__ __launch_bounds__(ASM_BLOCK) void leap_unit_hint_kernel(const uint4* __restrict__ planes,
                                                                   const uint32_t* __restrict__ lens, long n, int w4,
                                                                   OutMap out, const int32_t* __restrict__ hint) {
    __shared__ uint16_t s_sorted[LEAP_HINT_PAIRS];
    __shared__ int s_bin[64];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * LEAP_HINT_PAIRS;
    const int cnt = (n - base) < LEAP_HINT_PAIRS ? (int)(n - base) : LEAP_HINT_PAIRS;
    if (t < 64) s_bin[t] = 0;
    __syncthreads();
    int key[LEAP_HINT_PAIRS / ASM_BLOCK];
#pragma unroll
    for (int q = 0; q < LEAP_HINT_PAIRS / ASM_BLOCK; q++) {
        const int local = t + q * ASM_BLOCK;
        key[q] = -1;
        if (local < cnt) {
            int h = hint[out.index(base + local)];
            h = h < 0 ? 63 : (h > 63 ? 63 : h);
            key[q] = h;
            atomicAdd(&s_bin[h], 1);
        }
    }
    __syncthreads();
    if (t < 64) { /* exclusive scan of 64 bins in the first wave: bin t ends up with the count of all bins below it */
        const int c = s_bin[t];
        int run = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(run, off, 64);
            run += t >= off ? up : 0;
        }
        s_bin[t] = run - c;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LEAP_HINT_PAIRS / ASM_BLOCK; q++) {
        if (key[q] >= 0) {
            const int slot = atomicAdd(&s_bin[key[q]], 1);
            s_sorted[slot] = (uint16_t)(t + q * ASM_BLOCK);
        }
    }
    __syncthreads();
    for (int q = 0; q < LEAP_HINT_PAIRS / ASM_BLOCK; q++) {
        const int p = t + q * ASM_BLOCK;
        if (p < cnt) {
            const long i = base + s_sorted[p];
            out.put(i, leap_unit_pair<K, W64>(planes, lens, n, w4, i));
        }
    }
}

// --------------------------------------------------------------------------------------------------------
// LEAP with general penalties (x, o, ext), narrow band, one thread per pair: lv_affine_step over rings of LvRings::pow2 depths
// (asm_affine.h), per thread, in dynamic LDS laid out [ring][slot][lane][thread]: thread-private columns, so no barriers and no
// bank conflicts; slot offsets are wave-uniform (scalar).
// --------------------------------------------------------------------------------------------------------

template <int K, int W64, typename EnT> /* EnT: ring element, values stored + 2 (0 = never reached) */
__global__ __launch_bounds__(LEAP_GEN_THREADS) void leap_general_kernel(const uint4* __restrict__ planes,
                                                                        const uint32_t* __restrict__ lens, long n, int w4,
                                                                        int x, int o, int ext, int gm, int gi, OutMap out) {
    constexpr int NL = 2 * K + 1, T = LEAP_GEN_THREADS, SLOT = NL * T;
    extern __shared__ uint32_t s_ring32[];
    const int t = threadIdx.x;
    EnT* const r_en = reinterpret_cast<EnT*>(s_ring32) + t;
    EnT* const r_ip = r_en + gm * SLOT;
    EnT* const r_dp = r_ip + gi * SLOT;
    const long i = (long)blockIdx.x * T + t;
    if (i >= n) return;
    const uint32_t ln = lens[i];
    const int m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
    const int len = m > nn ? m : nn; /* benchmark_utils.h:162 */
    VW<W64> A0, A1, B0, B1;
    load_planes<W64>(planes, n, w4, i, A0, A1, B0, B1);
    const VW<W64> VA = vw_low_ones<W64>(m), VB = vw_low_ones<W64>(nn);
    VW<W64> mask[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) mask[j] = leap_lane_mask<W64>(A0, A1, B0, B1, VA, VB, j - K);
    VWAbove<W64> above[NL]; /* the saturating scan's fall-backs (vw_next_one_fb) */
#pragma unroll
    for (int j = 0; j < NL; j++) above[j] = vw_above<W64>(mask[j]);

    int result = -1;
    // e = 0: only the main diagonal is live (LV_BAG.cpp:102-104,131-147)
#pragma unroll
    for (int j = 0; j < NL; j++) { /* every slot starts as "never reached" (which stands in for the reference's guards: lv_affine_step, asm_affine.h) */
        for (int q = 0; q < gm; q++) r_en[q * SLOT + j * T] = (EnT)0;
        for (int q = 0; q < gi; q++) r_ip[q * SLOT + j * T] = (EnT)0, r_dp[q * SLOT + j * T] = (EnT)0;
    }
    {
        int e0 = vw_next_one<W64>(mask[K], 0);
        e0 = e0 > len ? len : e0;
        r_en[K * T] = (EnT)(e0 + 2);
        if (e0 == len) result = 0;
    }
    for (int e = 1; e <= ASM_LEAP_AF_THRESHOLD && result < 0; e++) {
        const LvRingView<EnT> g(r_en, r_ip, r_dp, LvRings{gm, gi}, SLOT, e, x, o, ext);
        bool pass = false;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int d = j - K;
            const int top = d >= 0 ? 1 : 0, bot = d <= 0 ? 1 : 0;
            const int e_up = j > 0 ? (int)g.en_o[(j > 0 ? j - 1 : 0) * T] - 2 : -2;
            const int i_up = j > 0 ? (int)g.ip_e[(j > 0 ? j - 1 : 0) * T] - 2 : -2;
            const int e_dn = j < NL - 1 ? (int)g.en_o[(j < NL - 1 ? j + 1 : j) * T] - 2 : -2;
            const int d_dn = j < NL - 1 ? (int)g.dp_e[(j < NL - 1 ? j + 1 : j) * T] - 2 : -2;
            const int own = (int)g.en_x[j * T] - 2;
            const auto [inew, dnew, st] = lv_affine_step(e_up, i_up, e_dn, d_dn, own, top, bot);
            int enew = -2;
            if (st >= 0) {
                const int from = st > len ? len : st;
                int r = VW_SCAN_FB(W64) ? vw_next_one_fb<W64>(mask[j], above[j], from) : vw_next_one<W64>(mask[j], from); /* count_ID_length, :9-23 */
                r = r > len ? len : r;
                enew = r > st ? r : st; /* st beyond the end stays st (r >= from = st otherwise) */
                if (enew == len) { /* :220-238 */
                    if (e + affine_gap(d < 0 ? -d : d, o, ext) <= ASM_LEAP_AF_THRESHOLD) pass = true;
                }
            }
            g.en_w[j * T] = (EnT)(enew + 2), g.ip_w[j * T] = (EnT)(inew + 2), g.dp_w[j * T] = (EnT)(dnew + 2);
        }
        if (pass) result = e; /* final_ED (LV_BAG.cpp:228,356-358) */
    }
    out.put(i, result);
}

// --------------------------------------------------------------------------------------------------------
// NW with affine gaps as a banded wavefront (furthest-reaching offsets per diagonal and score), one thread per pair —
// the same LDS rings as leap_general_kernel, at LvRings::exact depths (slot = score mod depth, in scalar counters).
// Diagonal d = j - i (i: read characters consumed, j: reference characters),
// lanes d in [-K, K].  M[s][d] = furthest i with cost s ending in a match/mismatch state; I consumes the reference
// (d-1 -> d, i unchanged), D consumes the read (d+1 -> d, i+1).  gap(L) = o + (L-1)*e, mismatch x — the model of
// nw_affine_kernel and of the oracle (benchmark_utils.h:139-142,288).  The answer is the first s whose M on diagonal
// n-m reaches i = m.
// Exactness of the band: a path that leaves it touches a diagonal |D| = K+1, which costs at least gap(K+1) to reach
// and gap(K+1-|n-m|) to come back from: bound = 2o + (2K - |n-m|)e.  A banded result s <= bound is therefore the global
// optimum; pairs that do not finish by then (or with |n-m| > K) are appended to `todo` for the full-matrix kernel.
// --------------------------------------------------------------------------------------------------------
// append `value` to list[*count ...) in the threads where `flag` holds: one atomic per wave
ASM_DEV void wave_append(uint32_t* __restrict__ list, uint32_t* __restrict__ count, bool flag, uint32_t value) {
    const u64 bal = __ballot(flag);
    if (bal) {
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        const int leader = __builtin_ctzll(bal);
        uint32_t base = 0;
        if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(count, (uint32_t)__builtin_popcountll(bal));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
        if (flag) list[base + rank] = value;
    }
}
// EnT: bytes when every position + 2 fits (values are stored + 2, 0 = never reached), else shorts.  LISTED: the pairs come from
// `in_list[0 .. *in_count)` (the previous pass's todo list) instead of 0..n.
template <int K, int W64, typename EnT, bool LISTED>
__global__ __launch_bounds__(LEAP_GEN_THREADS) void nw_wfa_kernel(const uint4* __restrict__ planes,
                                                                  const uint32_t* __restrict__ lens, long n, int w4, int x,
                                                                  int o, int ext, int gm, int gi, OutMap out,
                                                                  const uint32_t* __restrict__ in_list, const uint32_t* __restrict__ in_count,
                                                                  uint32_t* __restrict__ todo, uint32_t* __restrict__ todo_count) {
    constexpr int NL = 2 * K + 1, T = LEAP_GEN_THREADS, SLOT = NL * T;
    extern __shared__ uint32_t s_ring32[];
    EnT* const s_ring = reinterpret_cast<EnT*>(s_ring32);
    const int t = threadIdx.x;
    EnT* const r_m = s_ring + t;
    EnT* const r_i = r_m + gm * SLOT;
    EnT* const r_d = r_i + gi * SLOT;
    const long slot_id = (long)blockIdx.x * T + t;
    long i = slot_id;
    bool have = slot_id < n;
    if constexpr (LISTED) {
        have = slot_id < (long)*in_count;
        i = have ? (long)in_list[slot_id] : 0;
    }
    int result = 0;
    bool unresolved = false;
    if (have) {
        const uint32_t ln = lens[i];
        const int m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
        const int df = nn - m, adf = df < 0 ? -df : df;
        if (adf > K) {
            unresolved = true;
        } else {
            VW<W64> A0, A1, B0, B1;
            load_planes<W64>(planes, n, w4, i, A0, A1, B0, B1);
            // mismatch-or-outside vector per diagonal, indexed by i: bit p = (A[p] != B[p+d]) or p >= min(m, n-d) or p+d < 0
            VW<W64> mask[NL];
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int d = j - K, sft = d < 0 ? -d : d;
                const int lim = m < nn - d ? m : nn - d;
                const VW<W64> valid = vw_low_ones<W64>(lim);
                if (d >= 0) { /* bit p of b = B[p+d]: towards index 0 */
#pragma unroll
                    for (int q = 0; q < W64; q++) {
                        const u64 h0 = q + 1 < W64 ? B0.w[q + 1] : 0ull, h1 = q + 1 < W64 ? B1.w[q + 1] : 0ull;
                        const u64 b0 = (B0.w[q] >> sft) | (sft ? (h0 << (64 - sft)) : 0ull);
                        const u64 b1 = (B1.w[q] >> sft) | (sft ? (h1 << (64 - sft)) : 0ull);
                        mask[j].w[q] = (A0.w[q] ^ b0) | (A1.w[q] ^ b1) | ~valid.w[q];
                    }
                } else {
                    const VW<W64> b0 = vw_away0_small<W64>(B0, sft), b1 = vw_away0_small<W64>(B1, sft);
                    const VW<W64> low = vw_low_ones<W64>(sft);
#pragma unroll
                    for (int q = 0; q < W64; q++) mask[j].w[q] = (A0.w[q] ^ b0.w[q]) | (A1.w[q] ^ b1.w[q]) | ~valid.w[q] | low.w[q];
                }
            }
            const int bound = 2 * o + (2 * K - adf) * ext;
            result = -1;
            // every ring slot starts as "never reached": score s only sweeps the diagonals a gap of that cost can reach,
            // |d| <= (s - o) / ext + 1 (a bound that never shrinks), and their neighbours are read before they are ever written
            for (int q = 0; q < gm; q++)
#pragma unroll
                for (int j = 0; j < NL; j++) r_m[q * SLOT + j * T] = (EnT)0;
            for (int q = 0; q < gi; q++)
#pragma unroll
                for (int j = 0; j < NL; j++) r_i[q * SLOT + j * T] = (EnT)0, r_d[q * SLOT + j * T] = (EnT)0;
            {
                const int e0 = vw_next_one<W64>(mask[K], 0); /* <= min(m, n) */
                r_m[K * T] = (EnT)(e0 + 2);
                if (df == 0 && e0 >= m) result = 0;
            }
            // ring slots by score: scalar counters instead of a modulo (s, s-o, s-x, s-ext advance together)
            int sl_w = 0, sl_o = gm - o % gm, sl_x = gm - x % gm; /* slot of s, s-o, s-x in the M ring at s = 0 */
            int sj_w = 0, sj_e = gi - ext % gi;                    /* slot of s, s-ext in the I/D rings */
            sl_o = sl_o == gm ? 0 : sl_o, sl_x = sl_x == gm ? 0 : sl_x, sj_e = sj_e == gi ? 0 : sj_e;
            using LdsEl = __attribute__((address_space(3))) EnT;
            const uint32_t a_m = (uint32_t)(uintptr_t)(LdsEl*)r_m, a_i = (uint32_t)(uintptr_t)(LdsEl*)r_i, a_d = (uint32_t)(uintptr_t)(LdsEl*)r_d;
            const int m2 = m + 2;
            for (int s = 1; s <= bound && result < 0; s++) {
                sl_w = sl_w + 1 == gm ? 0 : sl_w + 1, sl_o = sl_o + 1 == gm ? 0 : sl_o + 1, sl_x = sl_x + 1 == gm ? 0 : sl_x + 1;
                sj_w = sj_w + 1 == gi ? 0 : sj_w + 1, sj_e = sj_e + 1 == gi ? 0 : sj_e + 1;
                // The seven slot addresses of this score, each pinned in a VGPR: a DS instruction takes one VGPR and an
                // immediate, and left alone the compiler re-adds the (scalar) slot offset in front of every access.
                uint32_t p_mo = a_m + (uint32_t)(sl_o * SLOT * (int)sizeof(EnT)), p_mx = a_m + (uint32_t)(sl_x * SLOT * (int)sizeof(EnT));
                uint32_t p_ie = a_i + (uint32_t)(sj_e * SLOT * (int)sizeof(EnT)), p_de = a_d + (uint32_t)(sj_e * SLOT * (int)sizeof(EnT));
                uint32_t p_mw = a_m + (uint32_t)(sl_w * SLOT * (int)sizeof(EnT)), p_iw = a_i + (uint32_t)(sj_w * SLOT * (int)sizeof(EnT));
                uint32_t p_dw = a_d + (uint32_t)(sj_w * SLOT * (int)sizeof(EnT));
                asm volatile("" : "+v"(p_mo), "+v"(p_mx), "+v"(p_ie), "+v"(p_de), "+v"(p_mw), "+v"(p_iw), "+v"(p_dw));
                const LdsEl* const m_o = (const LdsEl*)(uintptr_t)p_mo;
                const LdsEl* const m_x = (const LdsEl*)(uintptr_t)p_mx;
                const LdsEl* const i_e = (const LdsEl*)(uintptr_t)p_ie;
                const LdsEl* const d_e = (const LdsEl*)(uintptr_t)p_de;
                LdsEl* const m_w = (LdsEl*)(uintptr_t)p_mw;
                LdsEl* const i_w = (LdsEl*)(uintptr_t)p_iw;
                LdsEl* const d_w = (LdsEl*)(uintptr_t)p_dw;
                // No "s >= o" style guards on the reads: for s < o the slot of s - o is the slot of a score that has not been
                // written yet (ring depth > o), which still holds the initial "never reached"; likewise s - x and s - ext.
                // Unguarded, the five reads of a lane issue back to back instead of one scalar branch and one wait each.
                const int dmax = s < o ? 0 : (s - o) / ext + 1; /* wave-uniform: every thread is at the same score */
                int done = 0;
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int d = j - K;
                    if ((d < 0 ? -d : d) > dmax) continue;
                    // all values in the stored form u = position + 2 (0 = never reached, valid from 2)
                    const int m_lo = j > 0 ? (int)m_o[(j > 0 ? j - 1 : 0) * T] : 0;
                    const int i_lo = j > 0 ? (int)i_e[(j > 0 ? j - 1 : 0) * T] : 0;
                    const int m_hi = j < NL - 1 ? (int)m_o[(j < NL - 1 ? j + 1 : j) * T] : 0;
                    const int d_hi = j < NL - 1 ? (int)d_e[(j < NL - 1 ? j + 1 : j) * T] : 0;
                    const int own = (int)m_x[j * T];
                    int inew = m_lo > i_lo ? m_lo : i_lo;      /* reference character consumed: i stays, j = i + d */
                    inew = (inew >= 2 && inew + (d - 2) <= nn) ? inew : 0;
                    int dnew = m_hi > d_hi ? m_hi : d_hi;      /* read character consumed: i + 1 */
                    dnew = (dnew >= 2 && dnew < m2) ? dnew + 1 : 0;
                    int st = (own >= 2 && own < m2 && own + (d - 1) <= nn) ? own + 1 : 0;
                    st = inew > st ? inew : st;
                    st = dnew > st ? dnew : st;
                    int mnew = 0;
                    if (st >= 2) mnew = vw_next_one<W64>(mask[j], st - 2) + 2;
                    if (d == df && mnew >= m2) done = 1;
                    m_w[j * T] = (EnT)mnew, i_w[j * T] = (EnT)inew, d_w[j * T] = (EnT)dnew;
                }
                if (done) result = s;
            }
            if (result < 0) unresolved = true;
        }
    }
    wave_append(todo, todo_count, unresolved, (uint32_t)i);
    if (have && !unresolved) out.put(i, result);
}

// --------------------------------------------------------------------------------------------------------
// NW for unit penalties (x = o = e = 1): global edit distance by the Myers/Hyyro bit-parallel recurrence —
// the column of vertical deltas of the DP matrix lives in bit-vectors, one thread per pair, the read is the
// vertical string.  Gives exactly the penalty parasail's NW returns for these scores (benchmark_utils.h:
// 139-142,288 with matrix (0,-1), open = extend = 1, i.e. Levenshtein distance).
// --------------------------------------------------------------------------------------------------------
// Full-height bit-parallel column sweep: W64 64-bit words hold all m vertical deltas.
template <int W64>
ASM_DEV int nw_unit_full(const VW<W64>& A0, const VW<W64>& A1, const VW<W64>& B0, const VW<W64>& B1, int m, int nn) {
    if (m == 0) return nn;
    const VW<W64> VA = vw_low_ones<W64>(m);
    VW<W64> Pv, Mv;
#pragma unroll
    for (int q = 0; q < W64; q++) Pv.w[q] = ~0ull, Mv.w[q] = 0ull;
    int score = m;
    const int top_word = (m - 1) >> 6;
    const u64 top_bit = 1ull << ((m - 1) & 63);
    for (int j = 0; j < nn; j++) {
        // code of text character j, broadcast to all bits
        u64 t0 = 0, t1 = 0;
#pragma unroll
        for (int q = 0; q < W64; q++) {
            if ((j >> 6) == q) {
                t0 = (B0.w[q] >> (j & 63)) & 1ull;
                t1 = (B1.w[q] >> (j & 63)) & 1ull;
            }
        }
        const u64 T0 = 0ull - t0, T1 = 0ull - t1;
        u64 carry = 0, ph_in = 1ull, mh_in = 0ull; /* ph_in = 1: D[0][j] = j (global alignment) */
        int delta = 0;
#pragma unroll
        for (int q = 0; q < W64; q++) {
            const u64 Eq = ~(A0.w[q] ^ T0) & ~(A1.w[q] ^ T1) & VA.w[q];
            const u64 pv = Pv.w[q], mv = Mv.w[q];
            const u64 Xv = Eq | mv;
            const u64 x1 = Eq & pv;
            const u64 s1 = x1 + pv;
            const u64 c1 = s1 < x1 ? 1ull : 0ull;
            const u64 s2 = s1 + carry;
            const u64 c2 = s2 < s1 ? 1ull : 0ull;
            carry = c1 | c2;
            const u64 Xh = (s2 ^ pv) | Eq;
            u64 Ph = mv | ~(Xh | pv);
            u64 Mh = pv & Xh;
            if (q == top_word) {
                delta = (Ph & top_bit) ? 1 : ((Mh & top_bit) ? -1 : 0);
            }
            const u64 ph_out = Ph >> 63, mh_out = Mh >> 63;
            Ph = (Ph << 1) | ph_in;
            Mh = (Mh << 1) | mh_in;
            ph_in = ph_out, mh_in = mh_out;
            Pv.w[q] = Mh | ~(Xv | Ph);
            Mv.w[q] = Ph & Xv;
        }
        score += delta;
    }
    return score;
}

template <int W64>
__global__ __launch_bounds__(ASM_BLOCK) void nw_unit_kernel(const uint4* __restrict__ planes,
                                                            const uint32_t* __restrict__ lens, long n, int w4,
                                                            OutMap out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t ln = lens[i];
    const int m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
    VW<W64> A0, A1, B0, B1;
    load_planes<W64>(planes, n, w4, i, A0, A1, B0, B1);
    out.put(i, nw_unit_full<W64>(A0, A1, B0, B1, m, nn));
}

// (the banded sweeps themselves, nw_band<> and nw_band2x16<>, are in asm_nwband.h, which also compiles for the host)
template <int ND, int FIRSTW>
ASM_DEV int nw_banded_pair(const uint4* __restrict__ planes, const uint32_t* __restrict__ lens, long n, int w4, long i) {
    const uint32_t ln = lens[i];
    const int m = (int)(ln & 0xffffu), nn = (int)(ln >> 16);
    uint32_t A0[ND + 2], A1[ND + 2], B0[ND], B1[ND];
#pragma unroll
    for (int g = 0; g < ND / 4; g++) {
        uint4 q;
        q = planes[((long)0 * w4 + g) * n + i];
        A0[4 * g] = q.x, A0[4 * g + 1] = q.y, A0[4 * g + 2] = q.z, A0[4 * g + 3] = q.w;
        q = planes[((long)1 * w4 + g) * n + i];
        A1[4 * g] = q.x, A1[4 * g + 1] = q.y, A1[4 * g + 2] = q.z, A1[4 * g + 3] = q.w;
        q = planes[((long)2 * w4 + g) * n + i];
        B0[4 * g] = q.x, B0[4 * g + 1] = q.y, B0[4 * g + 2] = q.z, B0[4 * g + 3] = q.w;
        q = planes[((long)3 * w4 + g) * n + i];
        B1[4 * g] = q.x, B1[4 * g + 1] = q.y, B1[4 * g + 2] = q.z, B1[4 * g + 3] = q.w;
    }
    A0[ND] = A1[ND] = A0[ND + 1] = A1[ND + 1] = 0u;

    int result = -1;
    if (FIRSTW == 32) result = nw_band<ND, 32>(A0, A1, B0, B1, m, nn);
    if (result < 0) result = nw_band<ND, 64>(A0, A1, B0, B1, m, nn);
    if (result < 0) {
        // outside both proven bands: full-height sweep for this lane
        constexpr int W64 = ND / 2;
        VW<W64> a0, a1, b0, b1;
#pragma unroll
        for (int q = 0; q < W64; q++) {
            a0.w[q] = (u64)A0[2 * q] | ((u64)A0[2 * q + 1] << 32);
            a1.w[q] = (u64)A1[2 * q] | ((u64)A1[2 * q + 1] << 32);
            b0.w[q] = (u64)B0[2 * q] | ((u64)B0[2 * q + 1] << 32);
            b1.w[q] = (u64)B1[2 * q] | ((u64)B1[2 * q + 1] << 32);
        }
        result = nw_unit_full<W64>(a0, a1, b0, b1, m, nn);
    }
    return result;
}
// Mixed-length buckets (config C5): the banded sweep costs one step per reference character, and a wave runs as long as its
// longest pair — with the pairs of a width class in input order a wave of 64 holds lengths from all over the class's 128-base
// range and two thirds... three quarters of its lane-steps do work (lane utilisation 0.76 measured).  BYLEN: each workgroup
// counting-sorts its window of NW_SORT_PAIRS slots by reference length in LDS (128 bins: one per base of the class's range) and
// thread t takes the slot of rank t (t + 256, ... for wider windows): a wave then works on a quarter of the window's lengths.
// Loads stay inside the window (4 KB per plane granule: what a wave leaves of a sector its neighbours take from the cache),
// results go where they always went.
// (NW_SORT_PAIRS, the slots a workgroup sorts, and what was measured for it: asm_limits.h)
template <int ND, int FIRSTW, bool BYLEN> /* plane dwords per string: 4 * w4; FIRSTW = 32 or 64: the first window tried */
__global__ __launch_bounds__(ASM_BLOCK) void nw_banded_kernel(const uint4* __restrict__ planes,
                                                              const uint32_t* __restrict__ lens, long n, int w4,
                                                              OutMap out) {
    if (!BYLEN) {
        const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n) out.put(i, nw_banded_pair<ND, FIRSTW>(planes, lens, n, w4, i));
        return;
    }
    __shared__ uint16_t s_sorted[NW_SORT_PAIRS];
    __shared__ int s_bin[128];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * NW_SORT_PAIRS;
    const int cnt = (n - base) < NW_SORT_PAIRS ? (int)(n - base) : NW_SORT_PAIRS;
    if (t < 128) s_bin[t] = 0;
    __syncthreads();
    int key[NW_SORT_PAIRS / ASM_BLOCK];
#pragma unroll
    for (int q = 0; q < NW_SORT_PAIRS / ASM_BLOCK; q++) {
        const int local = t + q * ASM_BLOCK;
        key[q] = -1;
        if (local < cnt) {
            const int cols = (int)(lens[base + local] >> 16) - 128 * (w4 - 1) - 1; /* 0 .. 127 inside the class */
            key[q] = cols < 0 ? 0 : (cols > 127 ? 127 : cols);
            atomicAdd(&s_bin[key[q]], 1);
        }
    }
    __syncthreads();
    if (t < 64) { /* exclusive scan of 128 bins by one wave: two bins per lane, wave prefix by DPP-free shuffles */
        const int a = s_bin[2 * t], c = s_bin[2 * t + 1];
        int v = a + c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(v, d, 64);
            if (t >= d) v += up;
        }
        s_bin[2 * t] = v - a - c;
        s_bin[2 * t + 1] = v - c;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NW_SORT_PAIRS / ASM_BLOCK; q++)
        if (key[q] >= 0) s_sorted[atomicAdd(&s_bin[key[q]], 1)] = (uint16_t)(t + q * ASM_BLOCK);
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < NW_SORT_PAIRS / ASM_BLOCK; q++) {
        const int rank = t + q * ASM_BLOCK;
        if (rank < cnt) {
            const long i = base + s_sorted[rank];
            out.put(i, nw_banded_pair<ND, FIRSTW>(planes, lens, n, w4, i));
        }
    }
}

// One-granule batches in input order (config C2): a workgroup of ASM_BLOCK threads owns 2 * ASM_BLOCK consecutive pairs and
// thread t carries pairs base + t and base + ASM_BLOCK + t through ONE sweep, each in a 16-row window in its half of the
// dword (nw_band2x16<>): loads and both stores stay coalesced.  A half the 16-row window does not prove, and the pair of a
// thread that has no partner, goes through nw_banded_pair<ND, 32> — the cascade 32 rows -> 64 rows -> full height of
// nw_banded_kernel, which reads the pair's planes again — so every pair gets exactly what nw_banded_kernel gives it.
#define NW_PAIR2_MIN_WAVES 6 /* two pairs' planes are 32 dwords: keep the allocator at 80 VGPRs or fewer */
template <int ND>
__global__ __launch_bounds__(ASM_BLOCK, NW_PAIR2_MIN_WAVES) void nw_banded2_kernel(const uint4* __restrict__ planes,
                                                                                   const uint32_t* __restrict__ lens, long n, int w4,
                                                                                   OutMap out) {
    const long ip = (long)blockIdx.x * (2 * ASM_BLOCK) + threadIdx.x, iq = ip + ASM_BLOCK;
    if (ip >= n) return;
    int rp = -1, rq = -1;
    if (iq < n) {
        const uint32_t lp = lens[ip], lq = lens[iq];
        uint32_t P[4][ND], Q[4][ND]; /* planes A0, A1, B0, B1 */
#pragma unroll
        for (int pl = 0; pl < 4; pl++) {
#pragma unroll
            for (int g = 0; g < ND / 4; g++) {
                const uint4 a = planes[((long)pl * w4 + g) * n + ip], b = planes[((long)pl * w4 + g) * n + iq];
                P[pl][4 * g] = a.x, P[pl][4 * g + 1] = a.y, P[pl][4 * g + 2] = a.z, P[pl][4 * g + 3] = a.w;
                Q[pl][4 * g] = b.x, Q[pl][4 * g + 1] = b.y, Q[pl][4 * g + 2] = b.z, Q[pl][4 * g + 3] = b.w;
            }
        }
        nw_band2x16<ND>(P[0], P[1], P[2], P[3], (int)(lp & 0xffffu), (int)(lp >> 16), Q[0], Q[1], Q[2], Q[3], (int)(lq & 0xffffu),
                        (int)(lq >> 16), rp, rq);
    }
#pragma unroll 1
    for (int h = 0; h < 2; h++) { /* one copy of the cascade for both halves */
        const long i = h ? iq : ip;
        int r = h ? rq : rp;
        if (i >= n) break;
        if (r < 0) r = nw_banded_pair<ND, 32>(planes, lens, n, w4, i);
        out.put(i, r);
    }
}

// --------------------------------------------------------------------------------------------------------
// Seed-hit batches, the shape of the reference's read mapper (GASMA/mapper/main.cpp:77-86): for a hit of read i at
// reference position p the aligner sees reference[start, start + len_i + 1) with start = p ? p - 1 : 0 (clipped at
// the reference's end).  The reference text stays resident in HBM; windows are gathered on the device (text_gather_kernel).
// --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASM_BLOCK) void hit_window_lengths_kernel(const uint32_t* __restrict__ read_off,
                                                                       const unsigned long long* __restrict__ hit_pos,
                                                                       unsigned long long ref_len, long n,
                                                                       uint32_t* __restrict__ win_len,
                                                                       unsigned long long* __restrict__ win_start) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        win_len[n] = 0u; /* so that an exclusive scan over n+1 entries yields the total */
        return;
    }
    const unsigned long long p = hit_pos[i];
    const unsigned long long start = p ? p - 1ull : 0ull;
    const unsigned long long want = (unsigned long long)(read_off[i + 1] - read_off[i]) + 1ull;
    const unsigned long long room = start < ref_len ? ref_len - start : 0ull;
    win_len[i] = (uint32_t)(want < room ? want : room);
    win_start[i] = start; /* for text_gather_kernel (asm_ingest.h) */
}

// accuracy counters (benchmark_utils.h:249-255).  A single hot word saturates at ~88 atomics/us on this chip
// (MI355X_MICROARCH.md "dequeue"), so: wave shuffle -> LDS -> ONE atomic per workgroup, and a small grid.
ASM_DEV unsigned int block_sum_256(unsigned int v, unsigned int* s_part /* [4] */) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned int r = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(ASM_BLOCK) void count_equal_kernel(const int32_t* __restrict__ a,
                                                                const int32_t* __restrict__ b, long n,
                                                                unsigned long long* __restrict__ count) {
    __shared__ unsigned int s_part[4];
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    unsigned int local = 0;
    for (; i < n; i += stride) local += (a[i] == b[i]) ? 1u : 0u;
    const unsigned int tot = block_sum_256(local, s_part);
    if (threadIdx.x == 0 && tot) atomicAdd(count, (unsigned long long)tot);
}

// All of `_run_benchmark`'s counters in one pass: counters = {total_tests, nw_correct, LEAP_correct,
// greedy_correct}; the correct answer is answers[i] when given and != INT32_MIN, else the NW penalty
// (benchmark_utils.h:249-252).  leap / greedy may be null (aligner not run).
__global__ __launch_bounds__(ASM_BLOCK) void accuracy_kernel(const int32_t* __restrict__ nw,
                                                             const int32_t* __restrict__ leap,
                                                             const int32_t* __restrict__ greedy,
                                                             const int32_t* __restrict__ answers, long n,
                                                             unsigned long long* __restrict__ counters) {
    __shared__ unsigned int s_part[4];
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    unsigned int c_nw = 0, c_leap = 0, c_greedy = 0;
    // four pairs per thread and iteration: 16-byte loads, and enough independent loads in flight to cover HBM latency.
    // Without NW (nw == nullptr) the correct answer of a pair is its entry of the answers file, or nothing (INT32_MIN never
    // equals a penalty): total_tests still counts every pair.
    const long n4 = (nw != nullptr || answers != nullptr) ? n >> 2 : 0;
    const long n_cmp = (nw != nullptr || answers != nullptr) ? n : 0;
    const int4* nw4 = reinterpret_cast<const int4*>(nw);
    const int4* leap4 = reinterpret_cast<const int4*>(leap);
    const int4* greedy4 = reinterpret_cast<const int4*>(greedy);
    const int4* ans4 = reinterpret_cast<const int4*>(answers);
    // ... and ACC_AHEAD such groups in flight per thread: with one group per iteration the kernel is a chain of HBM round trips
    // (eight of them at 10^6 pairs), which is what it costs inside a step, where it sits on the NW -> LEAP -> counters chain.
    constexpr int ACC_AHEAD = 4;
    for (long q0 = i; q0 < n4; q0 += ACC_AHEAD * stride) {
        int4 p[ACC_AHEAD], a[ACC_AHEAD], l[ACC_AHEAD], g[ACC_AHEAD];
#pragma unroll
        for (int u = 0; u < ACC_AHEAD; u++) {
            const long q = q0 + u * stride;
            const long qq = q < n4 ? q : q0; /* a group beyond the end re-reads the first one and is not counted */
            p[u] = a[u] = l[u] = g[u] = make_int4(INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN);
            if (nw != nullptr) p[u] = nw4[qq];
            if (answers != nullptr) a[u] = ans4[qq];
            if (leap != nullptr) l[u] = leap4[qq];
            if (greedy != nullptr) g[u] = greedy4[qq];
        }
#pragma unroll
        for (int u = 0; u < ACC_AHEAD; u++) {
            if (q0 + u * stride >= n4) break;
            int4 want = p[u];
            if (answers != nullptr) {
                want.x = a[u].x != INT32_MIN ? a[u].x : p[u].x, want.y = a[u].y != INT32_MIN ? a[u].y : p[u].y;
                want.z = a[u].z != INT32_MIN ? a[u].z : p[u].z, want.w = a[u].w != INT32_MIN ? a[u].w : p[u].w;
            }
            if (nw != nullptr) c_nw += (p[u].x == want.x) + (p[u].y == want.y) + (p[u].z == want.z) + (p[u].w == want.w);
            if (leap != nullptr) c_leap += (l[u].x == want.x) + (l[u].y == want.y) + (l[u].z == want.z) + (l[u].w == want.w);
            if (greedy != nullptr) c_greedy += (g[u].x == want.x) + (g[u].y == want.y) + (g[u].z == want.z) + (g[u].w == want.w);
        }
    }
    for (long r = (n4 << 2) + i; r < n_cmp; r += stride) { /* the last n mod 4 pairs */
        const int32_t p = nw != nullptr ? nw[r] : INT32_MIN;
        int32_t want = p;
        if (answers != nullptr && answers[r] != INT32_MIN) want = answers[r];
        if (nw != nullptr) c_nw += (p == want) ? 1u : 0u;
        if (leap != nullptr) c_leap += (leap[r] == want) ? 1u : 0u;
        if (greedy != nullptr) c_greedy += (greedy[r] == want) ? 1u : 0u;
    }
    const unsigned int t_nw = block_sum_256(c_nw, s_part);
    const unsigned int t_leap = block_sum_256(c_leap, s_part);
    const unsigned int t_greedy = block_sum_256(c_greedy, s_part);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) atomicAdd(&counters[0], (unsigned long long)n);
        if (t_nw) atomicAdd(&counters[1], (unsigned long long)t_nw);
        if (t_leap) atomicAdd(&counters[2], (unsigned long long)t_leap);
        if (t_greedy) atomicAdd(&counters[3], (unsigned long long)t_greedy);
    }
}

// --------------------------------------------------------------------------------------------------------
// Device generator (asm_batch_generate): same inline code as the host generator (asm_gen.h).
// --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASM_BLOCK) void gen_lengths_kernel(asm_gen_config cfg, long first, long n,
                                                                uint32_t* __restrict__ mlen,
                                                                uint32_t* __restrict__ nlen) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int m, nn;
    asm_gen_lengths(&cfg, (uint64_t)(first + i), &m, &nn);
    mlen[i] = (uint32_t)m;
    nlen[i] = (uint32_t)nn;
}

__global__ __launch_bounds__(64) void gen_fill_kernel(asm_gen_config cfg, long first, long n,
                                                      const uint32_t* __restrict__ read_off,
                                                      const uint32_t* __restrict__ ref_off,
                                                      char* __restrict__ reads, char* __restrict__ refs) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    char rd[ASM_MAX_LENGTH + 8];
    char tx[ASM_GEN_MAX_TEXT];
    int m, nn;
    asm_gen_pair(&cfg, (uint64_t)(first + i), rd, tx, &m, &nn);
    char* r = reads + read_off[i];
    char* t = refs + ref_off[i];
    for (int j = 0; j < m; j++) r[j] = rd[j];
    for (int j = 0; j < nn; j++) t[j] = tx[j];
}
