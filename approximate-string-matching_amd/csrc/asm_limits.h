// The numeric limits that both the kernels and the aligner dispatch (asm_plan.h) read: thread shapes, compiled band and length
// limits, table sizes.  Each is defined here once; the kernel headers include this file and describe what the number means to
// the kernel.  Plain C, no HIP: asm_plan.h and the host checks compile with g++.
#pragma once

#define ASM_BLOCK 256

/* Greedy (asm_greedy3.h, asm_greedy3_kernel.h, asm_wave.h, asm_wide.h) */
#ifndef G3_TMAX
#define G3_TMAX 32  /* table domain: hurdles + switches < G3_TMAX; beyond it the FP64 path of the same kernel */
#endif
#define G3_LENS 129 /* highway lengths 0..128 */
#define G3_TABLE_ENTRIES (G3_LENS * G3_TMAX)
#ifndef G3_THREADS
#define G3_THREADS 512
#endif
/* G3_THREADS: one workgroup per CU: 8 waves = 2 per SIMD; LDS = table + 16 B per lane vector per thread */
#ifndef G3_STAGE_ENTRIES
#define G3_STAGE_ENTRIES 4096
#endif
#define ASM_WAVE_MAX_K 31
#define GREEDY_WAVE2_THREADS 128

/* the workgroup-per-pair kernels (asm_wide.h) */
#define ASM_WIDE_MAX_K 63       /* 2k+1 <= 127 lanes -> one 128-thread workgroup                         */
#define ASM_WIDE_MAX_PENALTY 15 /* LEAP history ring depth 16; NW boundary values stay inside int16       */
#define ASM_WIDE_THREADS 128

/* LEAP (asm_kernels.h, asm_wave.h) */
#define LEAP_UNIT_WIDE_K 5 /* thread-per-pair unit-cost LEAP at every string length up to this band */
#define LEAP_UNIT_MAX_K 10 /* ... and for strings of one granule (<= 128 characters) up to this one (k = 12: 0.148 ms against
                              0.180 at C2, but 0.120 against 0.104 at C4's 2.5 % errors, where four threads per pair have little to do) */
#define LEAP_HINT_PAIRS 256
#define LEAP_GEN_THREADS 128
#define LEAP_QUAD_THREADS 64
#define LEAP_QUAD_PAIRS 16

/* NW (asm_kernels.h, asm_wave.h) */
#define NW_SORT_PAIRS 256 /* slots a workgroup sorts by length: one per thread, a wave gets a quarter of the window's lengths.
                             Measured at C5, 10^7 pairs: no sort 2.31 ms, 256 slots 2.07, 1024 slots (four per thread) 2.21 — the
                             wider window is sorted better but its scattered 16-byte loads no longer share their sectors in cache */
#define NW_WFA_K 7
#define NW_WFA_K2 15 /* second pass over the pairs the first band could not settle (maxlen <= 128 only: 31 masks of 4 dwords) */
#define NW_OCT_THREADS 64
#define NW_OCT_Q 8
#define NW_OCT_PAIRS (NW_OCT_THREADS / NW_OCT_Q)

/* the filters (asm_filter.h) */
#define ASM_FILTER_MAX_T 32    /* lanes 2T+1 <= 65 */
#define ASM_FILTER_REG_MAX_T 8 /* masks of all lanes held in registers up to here; computed per use beyond */
#define SIMD_ED_THREADS 128
#define SIMD_QUAD_PD 6 /* zero dword, 4 plane dwords, zero dword */
/* what LvRings::quad_lds takes for the plane part: it counts w32 + 1 dwords per plane (data and one zero dword), here 4 + 2 */
#define SIMD_QUAD_W32 (SIMD_QUAD_PD - 1)
