// The pair aligners' and the filters' dispatch as pure functions: which kernel family, with which template constants, grid,
// block and dynamic LDS bytes, a width class of a batch goes to, and the parameter rules in front of it.  The host side
// (asm_align_host.h) computes a plan per bucket and only launches what it says; nothing there compares k, a length or a penalty.
//
// Plain C++17, no HIP: host/plan_host_check.cpp prints plans for lists of queries, and tests/test_plan_host.py holds every plan
// of a full grid against a transcription of the dispatch this header replaced.
//
// ONE decision is not made here because it needs the device: the plan says GREEDY_FAST, and the launcher takes GREEDY_PERSIST's
// kernel (greedy_persist_kernel<K, true>, through greedy_persist_plan below) when g3_prepare cannot build the rank table for the
// call's significance constants.  There is no other run-time fallback.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/asm_mi355x.h"
#include "asm_affine.h" /* LvRings, NW_BIG */
#include "asm_limits.h"

enum AlignFamily {
    GREEDY_FAST,     /* greedy_fast_kernel<K, G3_THREADS> */
    GREEDY_PERSIST,  /* greedy_persist_kernel<K, unit> */
    GREEDY_GROUP,    /* greedy_group_kernel<16, 5> */
    GREEDY_WAVE,     /* greedy_wave_kernel<unit> */
    GREEDY_WAVE2,    /* greedy_wave2_kernel */
    GREEDY_WIDE,     /* greedy_wide_kernel */
    LEAP_UNIT,       /* leap_unit_kernel<K, words> or, hinted, leap_unit_hint_kernel<K, words>; words of 64 bits */
    LEAP_GENERAL,    /* leap_general_kernel<K, words, entry>; words of 64 bits */
    LEAP_QUAD,       /* leap_quad_kernel<words, entry, unit, waves>; words of 32 bits */
    LEAP_WIDE,       /* leap_wide_kernel<words>; words of 64 bits */
    NW_UNIT_FULL,    /* nw_unit_kernel<words>; words of 64 bits */
    NW_BANDED,       /* nw_banded_kernel<words, window, false>; words = plane dwords */
    NW_BANDED_BYLEN, /* nw_banded_kernel<words, window, true> */
    NW_PAIR2,        /* nw_banded2_kernel<4> */
    NW_WFA,          /* nw_wfa_kernel<NW_WFA_K, words, entry>, [nw_oct_kernel<2 words, oct_entry>,] nw_affine_kernel<words, 64 words> */
    NW_AFFINE_FULL,  /* nw_affine_kernel<words, 64 words> over every pair */
    ALIGN_FAMILIES
};

/* how `grid` becomes the launch's grid */
enum GridRule {
    GRID_EXACT,     /* grid workgroups */
    GRID_PER_CU,    /* min(grid, grid_arg * num_cus) */
    GRID_OCCUPANCY, /* min(grid, resident workgroups per CU * num_cus); grid_arg = the count taken when the runtime gives none, 0 = its
                       error is the launch's */
};

struct AlignSwitches { /* filled once per call from the handle */
    bool wave_kernels, nw_banded, nw_bylen, nw_pair2, nw_wfa, greedy_fast, leap_hint, leap_sort;
};

struct AlignShape { /* one width class */
    int64_t n;
    int maxlen, w4;
    bool mixed;
};

struct AlignPlan {
    int family;
    int k;          /* template band K (LEAP_UNIT, LEAP_GENERAL, GREEDY_FAST, GREEDY_PERSIST, NW_WFA), else 0: the band is a run-time value */
    int words;      /* words per string the kernel is instantiated with (the family says of what) */
    int window;     /* NW_BANDED*: rows of the first window; NW_PAIR2: 16, fixed in the kernel */
    int entry;      /* bytes of a ring entry (1 or 2), 0 where there is no ring */
    int gm, gi;     /* depths of the rings (LvRings), 0 where there is no ring */
    bool unit;      /* the kernel's UNIT template argument (GREEDY_PERSIST, GREEDY_WAVE, LEAP_QUAD) */
    bool hinted;    /* the kernel reads the work hint (LEAP_UNIT: the hint kernel; LEAP_QUAD: sorted by it, see waves and sort) */
    int waves;      /* LEAP_QUAD: 4 = work-sorted inside workgroups of four waves, 1 = in input order or by the global sort */
    bool sort;      /* LEAP_QUAD: the global hint sort runs first ... */
    int sort_div;   /* ... on keys hint / sort_div */
    int oct_entry;  /* NW_WFA: the second pass runs with ring entries of this many bytes; 0 = no second pass */
    size_t oct_lds; /* ... and this much LDS */
    unsigned block;
    int64_t grid;
    int grid_rule, grid_arg;
    size_t lds;
};

/* first listed value >= v, the last one beyond: what with_const_of does with the same list */
template <int N>
static inline int plan_first_of(int v, const int (&list)[N]) {
    for (int q = 0; q + 1 < N; q++)
        if (v <= list[q]) return list[q];
    return list[N - 1];
}
static inline int plan_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static inline int64_t plan_blocks(int64_t n, int64_t per) { return (n + per - 1) / per; }

typedef uint16_t g3_stage_t; /* 0xFFFF: "this cost did not fit and went straight to memory" (never at 128 characters in practice) */
/* greedy_fast_kernel's LDS: the rank table, 16 B per lane vector per thread, the staged costs */
constexpr size_t g3_lds_bytes(int K, int NT) {
    return (size_t)G3_TABLE_ENTRIES * 8 + (size_t)(2 * K + 1) * NT * 16 + (size_t)G3_STAGE_ENTRIES * sizeof(g3_stage_t);
}

static inline bool plan_unit(const asm_params& p) { return p.x == 1 && p.o == 1 && p.e == 1; }

/* Persistent launch: grid = what is resident (CUs x occupancy); each wave owns a static slice of the batch. */
static inline AlignPlan greedy_persist_plan(int k, bool unit, int64_t n) {
    AlignPlan pl = {};
    pl.family = GREEDY_PERSIST, pl.k = k, pl.unit = unit;
    pl.block = ASM_BLOCK, pl.grid = plan_blocks(n, ASM_BLOCK), pl.grid_rule = GRID_OCCUPANCY, pl.grid_arg = 0;
    return pl;
}

static inline AlignPlan greedy_plan(const asm_params& p, const AlignShape& s, const AlignSwitches& sw) {
    AlignPlan pl = {};
    const bool semi = p.alignment_type == ASM_ALIGN_SEMI_GLOBAL;
    const bool unit = plan_unit(p) && !semi;
    if (p.k >= 1 && p.k <= 16) {
        /* Thread per pair.  K = 17, 18 still win at 100 bp (0.71, 0.79 ms against 0.90) but lose at 150 bp, err 0.20 (1.67, 1.83
         * against 1.60).  The straight-line integer-key kernel for the benchmark's own configuration (k <= 3, unit penalties,
         * GLOBAL), the FP64 lane-refilling kernel for everything else (unit and general penalties, GLOBAL and SEMI_GLOBAL: at k = 8
         * with (2,3,1) 0.27 ms per 10^6 pairs against 0.87 for the wave-per-pair kernel). */
        if (p.k > 3 || !sw.greedy_fast || !unit) return greedy_persist_plan(p.k, unit, s.n);
        /* One 512-thread workgroup per CU = two waves per SIMD (LDS: the table alone is 33 KB, with the lane vectors above 64 KB at
         * every K).  The waves of a SIMD are served oldest first and this kernel is a dense stream of 4-cycle vector operations, so
         * a third wave adds little issue rate and a third more lanes to drain at the end: stand-alone 1 / 2 / 3 waves take 130 /
         * 118 / 107 us, inside asm_run_benchmark_async's overlapped step 0.234 / 0.227 / 0.244 ms per step (1.5 and 2.5 waves:
         * 0.237, —).  The other instantiations were removed in round 4 (last in 312851a). */
        pl.family = GREEDY_FAST, pl.k = p.k, pl.unit = true;
        pl.block = G3_THREADS, pl.grid = plan_blocks(s.n, G3_THREADS), pl.grid_rule = GRID_PER_CU, pl.grid_arg = 1;
        pl.lds = g3_lds_bytes(p.k, G3_THREADS);
    } else if (sw.wave_kernels && p.k >= 32 && p.k <= 39 && (long)p.o + 110L * p.e < 16000L) {
        /* 65..79 band lanes: sixteen threads per pair, five lanes each (asm_group.h): 1.78 ms per 10^6 C2 pairs against 2.25 ms for
         * the two-wavefront kernel */
        pl.family = GREEDY_GROUP;
        pl.block = ASM_BLOCK, pl.grid = plan_blocks(s.n * 16, ASM_BLOCK), pl.grid_rule = GRID_OCCUPANCY, pl.grid_arg = 4;
    } else if (p.k <= ASM_WAVE_MAX_K && sw.wave_kernels && (unit || (long)p.o + 62L * p.e < 16000L)) {
        pl.family = GREEDY_WAVE, pl.unit = unit;
        pl.block = ASM_BLOCK, pl.grid = plan_blocks(s.n, 4); /* four waves (pairs in flight) per workgroup */
        pl.grid_rule = GRID_OCCUPANCY, pl.grid_arg = 8;
    } else if (sw.wave_kernels && (long)p.o + 100L * p.e < 16000L) {
        pl.family = GREEDY_WAVE2;
        pl.block = GREEDY_WAVE2_THREADS, pl.grid = s.n, pl.grid_rule = GRID_PER_CU, pl.grid_arg = 16; /* two waves each; the kernel strides over the pairs */
    } else {
        pl.family = GREEDY_WIDE;
        pl.block = ASM_WIDE_THREADS, pl.grid = s.n < 256 * 32 ? s.n : 256 * 32;
    }
    return pl;
}

static inline AlignPlan leap_wide_plan(const AlignShape& s) {
    static const int words[] = {2, 4, 8};
    AlignPlan pl = {};
    pl.family = LEAP_WIDE, pl.words = plan_first_of(2 * s.w4, words);
    pl.block = ASM_WIDE_THREADS, pl.grid = s.n < 256 * 32 ? s.n : 256 * 32;
    return pl;
}

static inline AlignPlan leap_plan(const asm_params& p, const AlignShape& s, const AlignSwitches& sw, bool hint) {
    /* LV's other ED_modes have no caller in the reference: one kernel serves them, the workgroup-per-pair form that takes any band
     * and any penalties (asm_wide.h) */
    if (p.leap_mode != ASM_LEAP_GLOBAL) return leap_wide_plan(s);
    AlignPlan pl = {};
    const bool unit = plan_unit(p);
    const int k = (int)p.k;
    hint = hint && sw.leap_hint;
    const int quad_entry = s.maxlen + 2 <= 255 ? 1 : 2; /* every stored position + 2 fits a byte */
    const LvRings quad_rg = unit ? LvRings::unit() : LvRings::pow2(p.x, p.o, p.e); /* leap_quad_kernel's rings (LEAP penalties are at most 15) */
    if (unit && k >= 1 && ((k <= LEAP_UNIT_WIDE_K && s.maxlen <= 384) || (k <= LEAP_UNIT_MAX_K && s.maxlen <= 128))) {
        /* thread per pair, band lanes in registers: k <= 5 at any length; k = 6..10 for strings of one granule, where the
         * four-threads-per-pair kernel is 1.6-2 x slower (C2, 10^6 pairs, k = 6 / 8 / 10: 0.085 / 0.089 / 0.111 ms against 0.174 /
         * 0.181 / 0.180).  64-bit words per string, one instantiation per count up to six (C5's longest class, 257-300, on five
         * words); the wider bands (6..10 lanes each side) are kept in registers for one granule only */
        pl.family = LEAP_UNIT, pl.k = k, pl.words = plan_clamp((s.maxlen + 63) / 64, 2, k <= LEAP_UNIT_WIDE_K ? 6 : 2);
        pl.hinted = hint;
        pl.block = ASM_BLOCK, pl.grid = plan_blocks(s.n, hint ? LEAP_HINT_PAIRS : ASM_BLOCK);
    } else if (!unit && k >= 1 && ((k <= 5 && s.maxlen <= 256) || (k <= 8 && s.maxlen <= 128)) && sw.wave_kernels &&
               LvRings::pow2(p.x, p.o, p.e).ring_bytes(2 * k + 1, LEAP_GEN_THREADS, sizeof(uint16_t)) <= 64 * 1024) {
        /* general penalties, narrow band: thread per pair with an LDS generation ring; bands 6..8 for strings of one granule only */
        const LvRings rg = LvRings::pow2(p.x, p.o, p.e);
        pl.family = LEAP_GENERAL, pl.k = k, pl.words = 2 * plan_clamp((s.maxlen + 127) / 128, 1, 2);
        /* bytes (every stored position + 2 fits) halve the LDS and double the waves per CU, but four threads then write into one
         * dword: worth it only where shorts would leave the CU underfilled */
        pl.entry = s.maxlen + 4 <= 255 && rg.ring_bytes(2 * k + 1, LEAP_GEN_THREADS, 2) > 20 * 1024 ? 1 : 2;
        pl.block = LEAP_GEN_THREADS, pl.grid = plan_blocks(s.n, LEAP_GEN_THREADS);
        pl.lds = rg.ring_bytes(2 * k + 1, LEAP_GEN_THREADS, (size_t)pl.entry), pl.gm = rg.gm, pl.gi = rg.gi;
    } else if (sw.wave_kernels && s.maxlen <= 512 &&
               quad_rg.quad_lds(LEAP_QUAD_PAIRS, (s.maxlen + 31) / 32, k, (size_t)quad_entry) <= 64 * 1024) {
        /* wide band: four threads per pair, generation rings and planes in LDS (asm_wave.h) */
        static const int words[] = {4, 5, 6, 8, 12, 16};
        pl.family = LEAP_QUAD, pl.words = plan_first_of((s.maxlen + 31) / 32, words), pl.entry = quad_entry, pl.unit = unit;
        pl.hinted = hint;
        /* long-running cases (long strings or general penalties): sort the whole bucket by the hint — one 6-bit radix pass — and let
         * every single-wave workgroup take sixteen neighbours of the order; short ones sort inside the workgroup */
        pl.sort = hint && sw.leap_sort && (s.maxlen > 128 || !unit);
        pl.sort_div = unit ? 1 : (int)(p.e < p.x ? p.e : p.x);
        const size_t lds1 = quad_rg.quad_lds(LEAP_QUAD_PAIRS, pl.words, k, (size_t)quad_entry);
        pl.waves = hint && !pl.sort && 4 * lds1 + 512 <= 64 * 1024 ? 4 : 1; /* work-sorted inside workgroups of four waves (64 pairs) */
        pl.block = (unsigned)(pl.waves * LEAP_QUAD_THREADS), pl.grid = plan_blocks(s.n, pl.waves * LEAP_QUAD_PAIRS);
        pl.lds = (size_t)pl.waves * lds1, pl.gm = quad_rg.gm, pl.gi = quad_rg.gi;
    } else {
        return leap_wide_plan(s);
    }
    return pl;
}

static inline AlignPlan nw_plan(const asm_params& p, const AlignShape& s, const AlignSwitches& sw) {
    AlignPlan pl = {};
    if (plan_unit(p)) {
        /* The one w4 -> kernel mapping of unit-cost NW.  A width class of w4 granules has ND = 4 * w4 plane dwords = 2 * w4 64-bit
         * words per string: full height is nw_unit_kernel<2 * w4>, banded nw_banded_kernel<ND, first window, SORT> with a first
         * window of 32 rows for one granule and 64 above. */
        const int w4 = plan_clamp(s.w4, 1, 4);
        pl.block = ASM_BLOCK, pl.grid = plan_blocks(s.n, ASM_BLOCK);
        if (!sw.nw_banded) {
            pl.family = NW_UNIT_FULL, pl.words = 2 * w4;
            return pl;
        }
        pl.words = 4 * w4, pl.window = w4 == 1 ? 32 : 64;
        if (s.mixed && sw.nw_bylen) { /* a width class of a mixed-length batch: workgroup-local sort by length */
            /* (measured and dropped in round 4: ONE wave per 256-pair sort window working through its four length quartiles in
             * turn, so that every wave of the grid gets the same mix — C5, 10^7 pairs: 2.16-2.21 ms against 2.12 for this form;
             * the dispatcher does not pile the long quartiles on one SIMD) */
            pl.family = NW_BANDED_BYLEN, pl.grid = plan_blocks(s.n, NW_SORT_PAIRS);
        } else if (s.w4 == 1 && sw.nw_pair2) {
            pl.family = NW_PAIR2, pl.window = 16, pl.grid = plan_blocks(s.n, 2 * ASM_BLOCK);
        } else {
            pl.family = NW_BANDED;
        }
        return pl;
    }
    /* a zero penalty makes the wavefront read the generation it is writing (ring slot s - 0): plain Gotoh handles it */
    const bool positive = p.x >= 1 && p.o >= 1 && p.e >= 1;
    const LvRings rg = LvRings::exact(p.x, p.o, p.e);
    pl.block = 64, pl.grid = plan_blocks(s.n, 64); /* nw_affine_kernel: NW_AFFINE_FULL's only launch, NW_WFA's last */
    if (sw.nw_wfa && positive && s.maxlen <= 256 && rg.ring_bytes(2 * NW_WFA_K + 1, LEAP_GEN_THREADS, 2) <= 64 * 1024) {
        /* Banded wavefront pass (|d| <= 7), a second one with |d| <= 15 over the pairs the first could not settle (the unsettled
         * percent or two: eight threads per pair, asm_wave.h), then the full-matrix kernel over what is left.  block, grid and lds
         * are the first pass's. */
        static const int words[] = {2, 4};
        pl.family = NW_WFA, pl.k = NW_WFA_K, pl.words = plan_first_of((s.maxlen + 63) / 64, words);
        pl.entry = pl.words == 2 ? 1 : 2; /* strings up to 128: every stored position + 2 fits a byte, half the LDS */
        pl.block = LEAP_GEN_THREADS, pl.grid = plan_blocks(s.n, LEAP_GEN_THREADS);
        pl.lds = rg.ring_bytes(2 * NW_WFA_K + 1, LEAP_GEN_THREADS, (size_t)pl.entry), pl.gm = rg.gm, pl.gi = rg.gi;
        const int en = s.maxlen + 2 <= 255 ? 1 : 2;
        const size_t oct_lds = rg.quad_lds(NW_OCT_PAIRS, 2 * pl.words, NW_WFA_K2, (size_t)en);
        if (oct_lds <= 64 * 1024) pl.oct_entry = en, pl.oct_lds = oct_lds;
    } else {
        static const int words[] = {2, 4, 8};
        pl.family = NW_AFFINE_FULL, pl.words = plan_first_of((s.maxlen + 127) / 128 * 2, words);
    }
    return pl;
}

/* one aligner over one width class; p has passed check_params_rule */
static inline AlignPlan align_plan(int aligner, const asm_params& p, const AlignShape& s, const AlignSwitches& sw, bool hint) {
    return aligner == ASM_GREEDY ? greedy_plan(p, s, sw) : aligner == ASM_LEAP ? leap_plan(p, s, sw, hint) : nw_plan(p, s, sw);
}

/* SIMD_ED events of one bucket (asm_filter.h): simd_ed_kernel<reg_t, words>, words of 64 bits */
struct SimdEdPlan {
    int reg_t; /* 1 .. ASM_FILTER_REG_MAX_T: the register form, every lane live from generation 0; 0: the run-time form */
    int words;
    unsigned block;
    int64_t grid;
    size_t lds;
};
static inline SimdEdPlan simd_ed_plan(int T, int ed_mode, int64_t n, int maxlen) {
    static const int words[] = {2, 4};
    SimdEdPlan pl = {};
    pl.words = plan_first_of((maxlen + 63) / 64, words);
    pl.block = SIMD_ED_THREADS, pl.grid = plan_blocks(n, SIMD_ED_THREADS);
    if (T <= ASM_FILTER_REG_MAX_T && ed_mode != 1 && ed_mode != 2)
        pl.reg_t = plan_clamp(T, 1, ASM_FILTER_REG_MAX_T);
    else
        pl.lds = (size_t)2 * (2 * T + 3) * SIMD_ED_THREADS * sizeof(short);
    return pl;
}

/* The affine SIMD_ED filter of one bucket: simd_ed_affine_quad_kernel or simd_ed_affine_kernel<4>. */
struct SimdEdAffinePlan {
    bool refused; /* "generation rings exceed the LDS": decided for the whole call, whatever its buckets */
    bool quad;    /* four threads per pair (thread per pair measured 0.28/0.71/3.5 ms per 10^6 C2 pairs at gap 3/8/30 against
                     0.29/0.46/0.79); else thread per pair: the only instantiation kept is the one for strings beyond one granule */
    unsigned block;
    int64_t grid;
    size_t lds;
    int gm, gi;
};
static inline SimdEdAffinePlan simd_ed_affine_plan(int gap_threshold, int x, int o, int e, int64_t n, int maxlen) {
    SimdEdAffinePlan pl = {};
    const LvRings rg = LvRings::pow2(x, o, e);
    const int rows = 2 * gap_threshold + 3;
    int threads = 64;
    while (threads > 16 && rg.ring_bytes(rows, threads, sizeof(uint16_t)) > 150 * 1024) threads >>= 1;
    const size_t lds = rg.ring_bytes(rows, threads, sizeof(uint16_t));
    /* threads and lds are the thread-per-pair kernel's (strings beyond one granule); the refusal also meets batches whose buckets
     * all go to the quad kernel, which has its own LDS layout.  Stricter than needed there, but callers can observe it: kept as it
     * is. */
    pl.refused = lds > 150 * 1024;
    pl.quad = maxlen <= 128;
    pl.gm = rg.gm, pl.gi = rg.gi;
    if (pl.quad)
        pl.block = 64, pl.grid = plan_blocks(n, 16), pl.lds = rg.quad_lds(16, SIMD_QUAD_W32, gap_threshold, sizeof(uint8_t));
    else
        pl.block = (unsigned)threads, pl.grid = plan_blocks(n, threads), pl.lds = lds;
    return pl;
}

/* The parameter rules of the aligners: ASM_OK, or the code and the message of the first rule broken. */
struct ParamVerdict {
    int code;
    const char* msg;
};
static inline ParamVerdict check_params_rule(int aligner, const asm_params* p, int maxlen) {
    if (!p) return {ASM_EINVAL, "params is NULL"};
    if (p->x < 0 || p->o < 0 || p->e < 0) return {ASM_EINVAL, "penalties must be non-negative"};
    if (aligner == ASM_GREEDY) {
        if (p->k < 0 || p->k > ASM_GREEDY_MAX_K) return {ASM_EINVAL, "Greedy: k must be in [0, 50] (MAX_K, hurdle_matrix.h:8)"};
        if (!(p->p_match > 0 && p->p_mismatch > 0 && p->p_indel > 0)) return {ASM_EINVAL, "Greedy: probabilities must be positive"};
        if (p->alignment_type != ASM_ALIGN_GLOBAL && p->alignment_type != ASM_ALIGN_SEMI_GLOBAL)
            return {ASM_EUNSUPPORTED, "Greedy: alignment type must be GLOBAL or SEMI_GLOBAL (LOCAL is unsupported in the reference too, hurdle_matrix.h:467)"};
    } else if (aligner == ASM_LEAP) {
        if (p->k < 0 || p->k > ASM_WIDE_MAX_K) return {ASM_EINVAL, "LEAP: k out of range"};
        /* the recurrence reads generation e-o / e-ext / e-x: zero penalties would be same-generation reads,
         * and LV_BAG.cpp:165 assumes open >= extend */
        if (p->x < 1 || p->o < 1 || p->e < 1 || p->o < p->e) return {ASM_EINVAL, "LEAP: need x >= 1, o >= e >= 1 (LV_BAG.cpp:165-166)"};
        if (p->x > ASM_WIDE_MAX_PENALTY || p->o > ASM_WIDE_MAX_PENALTY)
            return {ASM_EUNSUPPORTED, "LEAP: penalties above the compiled history depth"};
        if (p->leap_mode < ASM_LEAP_GLOBAL || p->leap_mode > ASM_LEAP_SEMI_FREE_END)
            return {ASM_EINVAL, "LEAP: leap_mode must be one of ASM_LEAP_GLOBAL/LOCAL/SEMI_FREE_BEGIN/SEMI_FREE_END"};
        if (p->leap_mode != ASM_LEAP_GLOBAL && maxlen > 512)
            return {ASM_EUNSUPPORTED, "LEAP: the non-GLOBAL modes are built for strings up to 512 characters"};
    } else if (aligner == ASM_NW) {
        /* nw_affine_kernel keeps H/E/F below NW_BIG (int16 halves of one dword at the block boundary): every cell is at most
         * gap(i) + gap(j), and E/F one gap-open above that */
        const long worst = 2L * ((long)p->o + (long)(maxlen > 0 ? maxlen - 1 : 0) * (long)p->e) + (long)p->o;
        if (p->x > 10000 || p->o > 10000 || p->e > 10000 || worst >= (long)NW_BIG)
            return {ASM_EUNSUPPORTED, "NW: penalties too large for this batch's longest sequence "
                                      "(need 2*(o + (maxlen-1)*e) + o < 30000 and x, o, e <= 10000)"};
    } else {
        return {ASM_EINVAL, "unknown aligner id"};
    }
    return {ASM_OK, nullptr};
}
