// The host side of the pair aligners and the filters: the launchers, align_bucket / align_batch and the aligner entries, the
// coverage passes, and the SIMD_ED / SHD entries.  asm_capi.hip includes this file inside its extern "C" block, behind the handle, the
// pool, the error path, the launch, the batch, g3_prepare and check_params.
//
// Which kernel a bucket goes to, with which template constants, grid, block and LDS, is decided in asm_plan.h (align_plan,
// simd_ed_plan, simd_ed_affine_plan) and nowhere else: a launcher here turns a plan's constants into template arguments
// (with_const / with_const_of) and launches.  The one run-time fallback is launch_greedy_fast's (see asm_plan.h).
#pragma once
#include "asm_plan.h"

extern "C++" {
/* a plan's grid on this handle's device (GridRule, asm_plan.h) */
template <class Kern>
static hipError_t plan_grid(asm_handle* h, const AlignPlan& pl, Kern kern, unsigned& grid) {
    int64_t cap = pl.grid;
    if (pl.grid_rule == GRID_PER_CU) cap = (int64_t)pl.grid_arg * h->num_cus;
    if (pl.grid_rule == GRID_OCCUPANCY) {
        int per_cu = pl.grid_arg;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int)pl.block, 0);
        if (e != hipSuccess && pl.grid_arg == 0) return e;
        cap = (int64_t)(per_cu < 1 ? 1 : per_cu) * h->num_cus;
    }
    grid = (unsigned)std::min(pl.grid, cap);
    return hipSuccess;
}

/* the launch a plan describes: its grid, block and LDS bytes */
template <class... P, class... A>
static hipError_t launch_plan(asm_handle* h, const AlignPlan& pl, void (*kernel)(P...), A&&... args) {
    unsigned grid = 0;
    if (const hipError_t e = plan_grid(h, pl, kernel, grid)) return e;
    return launch_on(h->stream, kernel, grid, pl.block, pl.lds, std::forward<A>(args)...);
}

#ifdef GREEDY_DIAG
static void* g_diag_buf = nullptr; /* diagnostic build only (never the shipped library): per-wave cycle stamps of the Greedy kernel */
extern "C" void asm_diag_set_buffer(void* d) { g_diag_buf = d; }
#endif

template <int K>
static hipError_t launch_greedy_persist(asm_handle* h, const asm_bucket& b, const AlignPlan& pl, const GreedyArgs& ga, OutMap out,
                                        CigarSink cig) {
    const auto go = [&](auto kernel) {
        return launch_plan(h, pl, kernel, (const uint4*)b.planes, (const uint32_t*)b.lens, (long)b.n, b.w4, ga, out, cig, h->refill_greedy);
    };
    return pl.unit ? go(greedy_persist_kernel<K, true>) : go(greedy_persist_kernel<K, false>);
}

template <int K>
static hipError_t launch_greedy_fast(asm_handle* h, const asm_bucket& b, const AlignPlan& pl, const GreedyArgs& ga, OutMap out,
                                     CigarSink cig) {
    /* the significance constants do not have the structure the integer keys need: the FP64 kernel */
    if (!g3_prepare(h, ga, K)) return launch_greedy_persist<K>(h, b, greedy_persist_plan(K, true, b.n), ga, out, cig);
    const G3Sig sig = {ga.sig_match, ga.sig_mismatch, ga.sig_indel};
    return launch_plan(h, pl, greedy_fast_kernel<K, G3_THREADS>, (const uint4*)b.planes, (const uint32_t*)b.lens, (long)b.n, b.w4, sig,
                       h->d_g3_table, out, cig, h->refill_greedy);
}

static int launch_greedy(asm_handle* h, const asm_bucket& b, const asm_params* p, const AlignPlan& pl, OutMap out, CigarSink cig) {
    GreedyArgs ga;
    ga.x = p->x, ga.o = p->o, ga.e = p->e;
    ga.semi = p->alignment_type == ASM_ALIGN_SEMI_GLOBAL ? 1 : 0;
    ga.sig_match = log(p->p_match / 0.25); /* hurdle_matrix.h:536-538 */
    ga.sig_mismatch = log(p->p_mismatch / 0.25);
    ga.sig_indel = log(p->p_indel / 2 / 0.25);
    const long n = (long)b.n;
    const int k = (int)p->k;
    switch (pl.family) {
    case GREEDY_FAST:
    case GREEDY_PERSIST:
#ifdef GREEDY_DIAG
        if (cig.ops == nullptr && g_diag_buf) cig.nops = (uint8_t*)g_diag_buf;
#endif
        if (pl.family == GREEDY_FAST)
            HIPCHK(h, (with_const<1, 3>(pl.k, [&](auto kc) { return launch_greedy_fast<decltype(kc)::value>(h, b, pl, ga, out, cig); })));
        else
            HIPCHK(h, (with_const<1, 16>(pl.k, [&](auto kc) { return launch_greedy_persist<decltype(kc)::value>(h, b, pl, ga, out, cig); })));
        break;
    case GREEDY_GROUP:
        HIPCHK(h, launch_plan(h, pl, greedy_group_kernel<16, 5>, b.planes, b.lens, n, b.w4, k, ga, out, cig));
        break;
    case GREEDY_WAVE: {
        HIPCHK(h, hipMemsetAsync(h->d_pair_queue, 0, sizeof(unsigned long long), h->stream));
        const auto go = [&](auto kernel) {
            return launch_plan(h, pl, kernel, b.planes, b.lens, n, b.w4, k, ga, out, cig, h->d_pair_queue, (const uint32_t*)nullptr,
                               (const uint32_t*)nullptr);
        };
        HIPCHK(h, pl.unit ? go(greedy_wave_kernel<true>) : go(greedy_wave_kernel<false>));
        break;
    }
    case GREEDY_WAVE2:
        HIPCHK(h, launch_plan(h, pl, greedy_wave2_kernel, b.planes, b.lens, n, b.w4, k, ga, out, cig));
        break;
    default:
        HIPCHK(h, launch_plan(h, pl, greedy_wide_kernel, b.planes, b.lens, n, b.w4, k, ga, out, cig));
    }
    return ASM_OK;
}

template <int K, int W64>
static hipError_t launch_leap_unit_w(asm_handle* h, const asm_bucket& b, const AlignPlan& pl, OutMap out, const int32_t* hint) {
    if (pl.hinted) return launch_plan(h, pl, leap_unit_hint_kernel<K, W64>, b.planes, b.lens, (long)b.n, b.w4, out, hint);
    return launch_plan(h, pl, leap_unit_kernel<K, W64>, b.planes, b.lens, (long)b.n, b.w4, out);
}

/* 64-bit words per string: one instantiation per count up to six for the bands up to LEAP_UNIT_WIDE_K, two words above */
template <int K>
static hipError_t launch_leap_unit(asm_handle* h, const asm_bucket& b, const AlignPlan& pl, OutMap out, const int32_t* hint) {
    constexpr int WMAX = K <= LEAP_UNIT_WIDE_K ? 6 : 2;
    return with_const<2, WMAX>(pl.words, [&](auto w) { return launch_leap_unit_w<K, decltype(w)::value>(h, b, pl, out, hint); });
}

/* granules: one or two for the bands up to 5, one above */
template <int K>
static hipError_t launch_leap_general(asm_handle* h, const asm_bucket& b, const asm_params* p, const AlignPlan& pl, OutMap out) {
    constexpr int GMAX = K <= 5 ? 2 : 1;
    return with_const<1, GMAX>(pl.words / 2, [&](auto g) {
        constexpr int W64 = 2 * decltype(g)::value;
        const auto go = [&](auto kernel) {
            return launch_plan(h, pl, kernel, b.planes, b.lens, (long)b.n, b.w4, (int)p->x, (int)p->o, (int)p->e, pl.gm, pl.gi, out);
        };
        return pl.entry == 1 ? go(leap_general_kernel<K, W64, uint8_t>) : go(leap_general_kernel<K, W64, uint16_t>);
    });
}

/* the global work sort of leap_quad_kernel: the bucket's slots ordered by hint / sort_div, one 6-bit radix pass */
static int leap_hint_sort(asm_handle* h, const asm_bucket& b, const AlignPlan& pl, const int32_t* hint, OutMap out, const uint32_t** perm) {
    const size_t n = (size_t)b.n;
    size_t tmp_bytes = 0;
    HIPCHK(h, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (uint8_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr,
                                                 (uint32_t*)nullptr, (int)n, 0, 6, h->stream));
    const size_t need = 2 * n + 8 * n + tmp_bytes + 256; /* keys, keys', idx, perm, temp */
    if (const int rc = grow_device(h, h->d_sort, h->sort_cap, need)) return rc;
    uint32_t* const d_idx = (uint32_t*)h->d_sort;
    uint32_t* const d_perm = d_idx + n;
    uint8_t* const d_keys = (uint8_t*)(d_perm + n);
    uint8_t* const d_keys2 = d_keys + n;
    void* const d_tmp = (void*)(((uintptr_t)(d_keys2 + n) + 255) & ~(uintptr_t)255);
    HIPCHK(h, launch(h, leap_sort_keys_kernel, (unsigned)((n + 255) / 256), 256, hint, out, (long)n, pl.sort_div, d_keys, d_idx));
    HIPCHK(h, hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_keys, d_keys2, d_idx, d_perm, (int)n, 0, 6, h->stream));
    *perm = d_perm;
    return ASM_OK;
}

/* four threads per pair: W32 32-bit words per string, ring entries of EnT; four waves take the hint, one wave the sort's order */
template <int W32, typename EnT>
static hipError_t launch_leap_quad(asm_handle* h, const asm_bucket& b, const asm_params* p, const AlignPlan& pl, OutMap out,
                                   const int32_t* hint, const uint32_t* perm) {
    const auto go = [&](auto kernel, const int32_t* hnt, const uint32_t* prm) {
        return launch_plan(h, pl, kernel, b.planes, b.lens, (long)b.n, b.w4, (int)p->k, (int)p->x, (int)p->o, (int)p->e, pl.gm, pl.gi, out,
                           hnt, prm);
    };
    if (pl.waves == 4)
        return pl.unit ? go(leap_quad_kernel<W32, EnT, true, 4>, hint, nullptr) : go(leap_quad_kernel<W32, EnT, false, 4>, hint, nullptr);
    return pl.unit ? go(leap_quad_kernel<W32, EnT, true, 1>, nullptr, perm) : go(leap_quad_kernel<W32, EnT, false, 1>, nullptr, perm);
}

static int launch_leap(asm_handle* h, const asm_bucket& b, const asm_params* p, const AlignPlan& pl, OutMap out, const int32_t* hint) {
    switch (pl.family) {
    case LEAP_UNIT:
        HIPCHK(h, (with_const<1, LEAP_UNIT_MAX_K>(pl.k, [&](auto k) { return launch_leap_unit<decltype(k)::value>(h, b, pl, out, hint); })));
        break;
    case LEAP_GENERAL:
        HIPCHK(h, (with_const<1, 8>(pl.k, [&](auto k) { return launch_leap_general<decltype(k)::value>(h, b, p, pl, out); })));
        break;
    case LEAP_QUAD: {
        const uint32_t* perm = nullptr;
        if (pl.sort)
            if (const int rc = leap_hint_sort(h, b, pl, hint, out, &perm)) return rc;
        HIPCHK(h, (with_const_of<4, 5, 6, 8, 12, 16>(pl.words, [&](auto w) {
                   constexpr int W32 = decltype(w)::value;
                   return pl.entry == 1 ? launch_leap_quad<W32, uint8_t>(h, b, p, pl, out, hint, perm)
                                        : launch_leap_quad<W32, uint16_t>(h, b, p, pl, out, hint, perm);
               })));
        break;
    }
    default:
        HIPCHK(h, (with_const_of<2, 4, 8>(pl.words, [&](auto w) {
                   return launch_plan(h, pl, leap_wide_kernel<decltype(w)::value>, b.planes, b.lens, (long)b.n, b.w4, (int)p->k, (int)p->x,
                                      (int)p->o, (int)p->e, (int)p->leap_mode, out);
               })));
    }
    return ASM_OK;
}

/* Affine NW: the plan's wavefront pass, its second pass over the pairs the first could not settle where the plan has one, then
 * the full-matrix kernel over what is left.  Two todo lists of n + 1 words each.  Ring entries are bytes on two words. */
template <int W64>
static int launch_nw_wfa(asm_handle* h, const asm_bucket& b, const asm_params* p, const AlignPlan& pl, OutMap out) {
    typedef typename std::conditional<W64 == 2, uint8_t, uint16_t>::type EnT;
    if (const int rc = grow_device(h, h->d_todo, h->todo_cap, 2 * ((size_t)b.n + 1))) return rc;
    uint32_t* const list_a = h->d_todo;                 /* [0] = count, [1..] = pair slots */
    uint32_t* const list_b = h->d_todo + (size_t)b.n + 1;
    HIPCHK(h, hipMemsetAsync(list_a, 0, sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(list_b, 0, sizeof(uint32_t), h->stream));
    HIPCHK(h, launch_plan(h, pl, nw_wfa_kernel<NW_WFA_K, W64, EnT, false>, b.planes, b.lens, (long)b.n, b.w4, (int)p->x, (int)p->o, (int)p->e,
                          pl.gm, pl.gi, out, nullptr, nullptr, list_a + 1, list_a));
    const uint32_t* rest = list_a;
    if (pl.oct_entry) { /* eight threads per pair, |d| <= 15 (asm_wave.h) */
        const unsigned grid = (unsigned)std::min<int64_t>((b.n + NW_OCT_PAIRS - 1) / NW_OCT_PAIRS, (int64_t)h->num_cus * 16);
        const auto oct = [&](auto kernel) {
            return launch_lds(h, kernel, grid, NW_OCT_THREADS, pl.oct_lds, b.planes, b.lens, (long)b.n, b.w4, NW_WFA_K2, (int)p->x, (int)p->o,
                              (int)p->e, pl.gm, pl.gi, out, list_a + 1, list_a, list_b + 1, list_b);
        };
        HIPCHK(h, pl.oct_entry == 1 ? oct(nw_oct_kernel<2 * W64, uint8_t>) : oct(nw_oct_kernel<2 * W64, uint16_t>));
        rest = list_b;
    }
    HIPCHK(h, launch(h, nw_affine_kernel<W64, 64 * W64>, (unsigned)((b.n + 63) / 64), 64, b.planes, b.lens, (long)b.n, b.w4, (int)p->x,
                     (int)p->o, (int)p->e, out, rest + 1, rest));
    return ASM_OK;
}

static int launch_nw(asm_handle* h, const asm_bucket& b, const asm_params* p, const AlignPlan& pl, OutMap out) {
    const long n = (long)b.n;
    switch (pl.family) {
    case NW_UNIT_FULL:
        HIPCHK(h, (with_const<1, 4>(pl.words / 2, [&](auto w) {
                   return launch_plan(h, pl, nw_unit_kernel<2 * decltype(w)::value>, b.planes, b.lens, n, b.w4, out);
               })));
        break;
    case NW_BANDED:
    case NW_BANDED_BYLEN:
        /* ND = 4 * w4 plane dwords per string; a first window of 32 rows for one granule and 64 above */
        HIPCHK(h, (with_const<1, 4>(pl.words / 4, [&](auto w) {
                   constexpr int W4 = decltype(w)::value;
                   const auto go = [&](auto kernel) { return launch_plan(h, pl, kernel, b.planes, b.lens, n, b.w4, out); };
                   return pl.family == NW_BANDED_BYLEN ? go(nw_banded_kernel<4 * W4, (W4 == 1 ? 32 : 64), true>)
                                                       : go(nw_banded_kernel<4 * W4, (W4 == 1 ? 32 : 64), false>);
               })));
        break;
    case NW_PAIR2:
        HIPCHK(h, launch_plan(h, pl, nw_banded2_kernel<4>, b.planes, b.lens, n, b.w4, out));
        break;
    case NW_WFA:
        return with_const_of<2, 4>(pl.words, [&](auto w) { return launch_nw_wfa<decltype(w)::value>(h, b, p, pl, out); });
    default: /* every pair of the bucket: no todo list */
        HIPCHK(h, (with_const_of<2, 4, 8>(pl.words, [&](auto w) {
                   constexpr int W64 = decltype(w)::value;
                   return launch_plan(h, pl, nw_affine_kernel<W64, 64 * W64>, b.planes, b.lens, n, b.w4, (int)p->x, (int)p->o, (int)p->e, out,
                                      nullptr, nullptr);
               })));
    }
    return ASM_OK;
}

/* the switches of the handle that the plan reads */
static AlignSwitches align_switches(const asm_handle* h) {
    return AlignSwitches{h->wave_kernels, h->nw_banded, h->nw_bylen, h->nw_pair2, h->nw_wfa, h->greedy_fast, h->leap_hint, h->leap_sort};
}

/* one aligner over one width class */
static int align_bucket(asm_handle* h, const asm_bucket& b, int aligner, const asm_params* p, const AlignSwitches& sw, OutMap out,
                        CigarSink cig, const int32_t* hint) {
    if (b.n == 0) return ASM_OK;
    const AlignPlan pl = align_plan(aligner, *p, AlignShape{b.n, b.maxlen, b.w4, b.mixed}, sw, hint != nullptr);
    if (aligner == ASM_GREEDY) return launch_greedy(h, b, p, pl, out, cig);
    if (aligner == ASM_LEAP) return launch_leap(h, b, p, pl, out, hint);
    return launch_nw(h, b, p, pl, out);
}

/* SIMD_ED events of one bucket (asm_filter.h) */
static int launch_simd_ed_events(asm_handle* h, const asm_bucket& b, int T, int shd, OutMap ev, int ed_mode) {
    const SimdEdPlan pl = simd_ed_plan(T, ed_mode, b.n, b.maxlen);
    HIPCHK(h, (with_const_of<2, 4>(pl.words, [&](auto w) {
               constexpr int W64 = decltype(w)::value;
               if (pl.reg_t)
                   return with_const<1, ASM_FILTER_REG_MAX_T>(pl.reg_t, [&](auto t) {
                       return launch(h, simd_ed_kernel<decltype(t)::value, W64>, (unsigned)pl.grid, pl.block, b.planes, b.lens, (long)b.n, b.w4,
                                     T, shd, 0, ev);
                   });
               return launch_lds(h, simd_ed_kernel<0, W64>, (unsigned)pl.grid, pl.block, pl.lds, b.planes, b.lens, (long)b.n, b.w4, T, shd,
                                 ed_mode, ev);
           })));
    return ASM_OK;
}

/* Full-matrix Gotoh + traceback + coverage verdict (nw_trace_affine_kernel) over `count` slots of a bucket slice: the slots
 * listed in d_list (bucket-slice indices), or slots 0..count-1 when d_list is null.  Scratch: 4 direction bits per cell. */
static int cover_full_matrix(asm_handle* h, const asm_bucket& b, const asm_params* p, const uint4* planes, const uint32_t* lens,
                             const uint32_t* order, long slice_lo, const uint32_t* d_list, int64_t count, const CoverArgs& ca) {
    if (count <= 0) return ASM_OK;
    const int rows = b.maxlen > 0 ? b.maxlen : 1, cols8 = (rows + 7) / 8;
    const size_t per_pair = (size_t)rows * (size_t)cols8 * sizeof(uint32_t);
    int64_t chunk = (int64_t)((size_t)(6ull << 30) / per_pair);
    chunk = chunk < 64 ? 64 : chunk;
    chunk = chunk > count ? count : chunk;
    BigScratch<uint32_t> d_scratch;
    HIPCHK(h, d_scratch.alloc(h, per_pair * (size_t)chunk));
    for (int64_t lo = 0; lo < count; lo += chunk) {
        const int64_t c = count - lo < chunk ? count - lo : chunk;
        /* without a list the chunk is a contiguous run of slots: shift the base pointers like cover_bucket does */
        const uint4* pl = d_list ? planes : planes + lo;
        const uint32_t* ln = d_list ? lens : lens + lo;
        const uint32_t* od = (d_list || !order) ? order : order + lo;
        const long base = d_list ? slice_lo : slice_lo + lo;
        const uint32_t* list = d_list ? d_list + lo : nullptr;
        const hipError_t e = with_const_of<2, 4, 8>((b.maxlen + 63) / 64, [&](auto w) { /* 64-bit words per string; rows = positions they hold */
            constexpr int W64 = decltype(w)::value;
            return launch(h, nw_trace_affine_kernel<W64, 64 * W64>, (unsigned)((c + 63) / 64), 64, pl, ln, (long)c, (long)b.n, b.w4,
                          (int)p->x, (int)p->o, (int)p->e, d_scratch.p, cols8, list, od, base, ca);
        });
        if (e != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
            return fail(h, ASM_ENODEVICE, "asm_coverage: full-matrix traceback kernel failed");
    }
    return ASM_OK;
}

/* forward sweep + traceback/coverage for one width class with window W; pairs the band cannot answer go through the
 * full-matrix pass */
template <int ND, int W>
static int cover_bucket(asm_handle* h, const asm_bucket& b, const asm_params* p, const CoverArgs& ca) {
    typedef typename TraceCell<W>::T Cell;
    if (b.n == 0) return ASM_OK;
    // scratch: [column][pair]; processed in slices of pairs so that it stays below ~6 GiB
    const int64_t cols = b.maxlen > 0 ? b.maxlen : 1;
    int64_t slice = (int64_t)(6ll << 30) / (cols * (int64_t)sizeof(Cell));
    slice = slice > b.n ? b.n : (slice < 4096 ? 4096 : slice);
    if (const int rc = grow_device(h, h->d_todo, h->todo_cap, (size_t)slice + 1)) return rc;
    BigScratch<Cell> d_trace;
    BigScratch<int32_t> d_band;
    HIPCHK(h, d_trace.alloc(h, (size_t)cols * (size_t)slice * sizeof(Cell)));
    if (d_band.alloc(h, sizeof(int32_t) * (size_t)slice) != hipSuccess) return fail(h, ASM_ENOMEM, "asm_coverage: hipMalloc failed");
    for (int64_t lo = 0; lo < b.n; lo += slice) {
        const int64_t cnt = b.n - lo < slice ? b.n - lo : slice;
        // a slice is addressed as a sub-batch: plane rows keep the bucket's stride, so pass shifted base pointers
        const uint4* planes = b.planes + lo;
        const uint32_t* lens = b.lens + lo;
        const uint32_t* order = b.order ? b.order + lo : nullptr;
        uint32_t todo_count = 0;
        if (hipMemsetAsync(h->d_todo, 0, sizeof(uint32_t), h->stream) != hipSuccess) return fail(h, ASM_ENODEVICE, "asm_coverage: memset failed");
        // the kernels index planes as [(p*w4+g)*n + i] with n = pairs of the BUCKET: use dedicated strided variants
        if (launch(h, nw_trace_forward_kernel<ND, W>, grid_for(cnt), ASM_BLOCK, planes, lens, (long)cnt, (long)b.n, b.w4, d_trace.p,
                   d_band.p) != hipSuccess ||
            launch(h, nw_trace_cover_kernel<ND / 2, W>, grid_for(cnt), ASM_BLOCK, planes, lens, (long)cnt, (long)b.n, b.w4, d_trace.p,
                   d_band.p, order, lo, ca, h->d_todo + 1, h->d_todo) != hipSuccess ||
            hipMemcpyAsync(&todo_count, h->d_todo, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return fail(h, ASM_ENODEVICE, "asm_coverage: kernel failed");
        if (todo_count)
            if (const int rc = cover_full_matrix(h, b, p, planes, lens, order, lo, h->d_todo + 1, (int64_t)todo_count, ca)) return rc;
    }
    return ASM_OK;
}

/* one aligner over a batch: what the three entry points below have in common */
static int align_batch(asm_handle* h, const asm_batch* b, int aligner, const asm_params* p, int32_t* d_penalties, CigarSink cig,
                       const int32_t* hint, const char* who) {
    if (!h || !b || !d_penalties) return fail(h, ASM_EINVAL, std::string(who) + ": NULL argument");
    if (const int rc = check_params(h, aligner, p, b->maxlen)) return rc;
    if (b->n == 0) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const AlignSwitches sw = align_switches(h);
    return for_each_bucket(b, d_penalties, [&](const asm_bucket& k, OutMap out) { return align_bucket(h, k, aligner, p, sw, out, cig, hint); });
}

} /* extern "C++" */

int asm_align_batch_hinted_async(asm_handle* h, const asm_batch* b, int aligner, const asm_params* p,
                                 const int32_t* d_work_hint, int32_t* d_penalties) {
    return align_batch(h, b, aligner, p, d_penalties, CigarSink{nullptr, nullptr, 0}, d_work_hint, "asm_align_batch_hinted_async");
}

int asm_align_batch_async(asm_handle* h, const asm_batch* b, int aligner, const asm_params* p, int32_t* d_penalties) {
    return align_batch(h, b, aligner, p, d_penalties, CigarSink{nullptr, nullptr, 0}, nullptr, "asm_align_batch_async");
}

int asm_greedy_cigar_batch_async(asm_handle* h, const asm_batch* b, const asm_params* p, int32_t* d_penalties,
                                 uint16_t* d_ops, int cap, uint8_t* d_nops) {
    if (!h || !b || !d_penalties || !d_ops || !d_nops || cap < 1)
        return fail(h, ASM_EINVAL, "asm_greedy_cigar_batch_async: bad argument");
    return align_batch(h, b, ASM_GREEDY, p, d_penalties, CigarSink{d_ops, d_nops, cap}, nullptr, "asm_greedy_cigar_batch_async");
}

int asm_cigar_format(const uint16_t* ops, int nops, int cap, char* out, size_t out_cap) {
    return asm_host::cigar_format(ops, nops, cap, out, out_cap);
}

int asm_coverage(asm_handle* h, const asm_batch* b, const asm_params* p, const uint16_t* d_greedy_ops, int greedy_cap,
                 const uint8_t* d_greedy_nops, int window, uint8_t* d_cover, uint16_t* d_nw_ops, int nw_cap,
                 uint8_t* d_nw_nops, unsigned long long* d_counters) {
    if (!h || !b || !p || !d_greedy_ops || !d_greedy_nops || !d_cover || !d_counters || greedy_cap < 1)
        return fail(h, ASM_EINVAL, "asm_coverage: bad argument");
    int prc = check_params(h, ASM_NW, p, b->maxlen);
    if (prc) return prc;
    if (window != 32 && window != 64) return fail(h, ASM_EINVAL, "asm_coverage: window must be 32 or 64");
    if (d_nw_ops && (!d_nw_nops || nw_cap < 1)) return fail(h, ASM_EINVAL, "asm_coverage: bad NW CIGAR buffers");
    if (b->n == 0) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    CoverArgs ca;
    ca.g_ops = d_greedy_ops, ca.g_nops = d_greedy_nops, ca.g_cap = greedy_cap;
    ca.cover = d_cover, ca.nw_ops = d_nw_ops, ca.nw_nops = d_nw_nops, ca.nw_cap = nw_cap, ca.counters = d_counters;
    int rc = ASM_OK;
    const bool unit = p->x == 1 && p->o == 1 && p->e == 1;
    for (int q = 0; q < b->nb && !rc; q++) {
        const asm_bucket& k = b->bk[q];
        if (!unit) { /* general penalties: every pair through the full matrix */
            rc = cover_full_matrix(h, k, p, k.planes, k.lens, k.order, 0, nullptr, k.n, ca);
            continue;
        }
        rc = with_const<1, 4>(k.w4, [&](auto w) { /* ND = plane dwords per string */
            constexpr int ND = 4 * decltype(w)::value;
            return window == 32 ? cover_bucket<ND, 32>(h, k, p, ca) : cover_bucket<ND, 64>(h, k, p, ca);
        });
    }
    return rc;
}

int asm_align_batch(asm_handle* h, int aligner, int64_t n, const char* reads, const uint32_t* read_off, const char* refs,
                    const uint32_t* ref_off, const asm_params* p, int greedy_mode, int32_t* penalties) {
    if (!h || !penalties) return fail(h, ASM_EINVAL, "asm_align_batch: NULL argument");
    int rc = check_params(h, aligner, p);
    if (rc) return rc;
    asm_batch* raw = nullptr;
    rc = asm_batch_upload(h, n, reads, read_off, refs, ref_off, greedy_mode, &raw);
    if (rc) return rc;
    BatchPtr b(raw);
    Scratch<int32_t> d_out(h);
    HIPCHK(h, d_out.alloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1)));
    rc = asm_align_batch_async(h, b.get(), aligner, p, d_out.p);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n > 0) HIPCHK(h, hipMemcpy(penalties, d_out.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return ASM_OK;
}

/* hipcub's inclusive last-setter scan on the handle's stream; the first call asks for the temporary size and reserves it */
static hipError_t inclusive_scan_last_setter(asm_handle* h, Scratch<void>& tmp, size_t& tmp_bytes, int32_t* in, int32_t* out, long n) {
    if (!tmp.p) {
        if (const hipError_t e = hipcub::DeviceScan::InclusiveScan(nullptr, tmp_bytes, in, out, LastSetter(), (int)n, h->stream)) return e;
        if (const hipError_t e = tmp.alloc(tmp_bytes + 16)) return e;
    }
    return hipcub::DeviceScan::InclusiveScan(tmp.p, tmp_bytes, in, out, LastSetter(), (int)n, h->stream);
}

/* Sequential mode: the events in d_ed become verdicts in batch order (S2 of asm_simd_ed.h) — setter keys, their last-setter scan,
 * converge keys from it, their scan, verdicts — and `state` (may be null: zeros in, nothing out) becomes what the next batch of the
 * same stream of pairs starts from.  One wait, for the two trailing scan values. */
static int simd_ed_resolve_sequential(asm_handle* h, int32_t* d_ed, long n, int T, int32_t* state) {
    const int init_fe = state ? state[0] : 0, init_fd = state ? state[1] : 0, init_conv = state ? state[2] : 0;
    const unsigned g = grid_for(n), t = ASM_BLOCK;
    int32_t last_setter = -1, last_conv = -1;
    size_t tmp_bytes = 0;
    Scratch<int32_t> d_a(h), d_b(h);
    Scratch<void> d_tmp(h);
    HIPCHK(h, d_a.alloc(sizeof(int32_t) * (size_t)n));
    HIPCHK(h, d_b.alloc(sizeof(int32_t) * (size_t)n));
    HIPCHK(h, launch(h, simd_ed_setter_kernel, g, t, d_ed, n, d_a.p));
    HIPCHK(h, inclusive_scan_last_setter(h, d_tmp, tmp_bytes, d_a.p, d_b.p, n));
    /* enqueued here, not in the fetch below: the second scan writes over d_b */
    HIPCHK(h, hipMemcpyAsync(&last_setter, d_b.p + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, launch(h, simd_ed_converge_kernel, g, t, d_ed, d_b.p, n, init_fe, init_fd, d_a.p));
    HIPCHK(h, inclusive_scan_last_setter(h, d_tmp, tmp_bytes, d_a.p, d_b.p, n));
    HIPCHK(h, launch(h, simd_ed_verdict_kernel, g, t, d_ed, d_b.p, n, T, init_conv));
    HIPCHK(h, fetch(h, {fetched(&last_conv, (const int32_t*)d_b.p + (n - 1))})); /* the wait: last_setter has arrived too */
    if (state) {
        if (last_setter >= 0) state[0] = last_setter & 0xff, state[1] = last_setter >> 8;
        if (last_conv >= 0) state[2] = last_conv;
    }
    return ASM_OK;
}

int asm_simd_ed_batch_async(asm_handle* h, const asm_batch* b, int ed_threshold, int shd_enable, int mode,
                            int32_t* state, int32_t* d_ed) {
    return asm_simd_ed_mode_batch_async(h, b, ed_threshold, shd_enable, mode, ASM_LEAP_GLOBAL, state, d_ed);
}

int asm_simd_ed_mode_batch_async(asm_handle* h, const asm_batch* b, int ed_threshold, int shd_enable, int mode, int ed_mode,
                                 int32_t* state, int32_t* d_ed) {
    if (!h || !b || !d_ed) return fail(h, ASM_EINVAL, "asm_simd_ed_batch_async: NULL argument");
    if (ed_mode < ASM_LEAP_GLOBAL || ed_mode > ASM_LEAP_SEMI_FREE_END)
        return fail(h, ASM_EINVAL, "asm_simd_ed_mode_batch_async: ed_mode must be one of ASM_LEAP_GLOBAL/LOCAL/SEMI_FREE_BEGIN/SEMI_FREE_END");
    if (ed_threshold < 1 || ed_threshold > ASM_FILTER_MAX_T)
        return fail(h, ASM_EINVAL, "asm_simd_ed_batch_async: ED threshold must be in [1, 32]");
    if (shd_enable && ed_threshold > ASM_SHD_MAX_ERROR)
        return fail(h, ASM_EINVAL, "asm_simd_ed_batch_async: SHD needs an ED threshold <= 16 (MAX_ERROR_AVX)");
    if (mode != ASM_FILTER_SEQUENTIAL && mode != ASM_FILTER_CLEAN)
        return fail(h, ASM_EINVAL, "asm_simd_ed_batch_async: unknown mode");
    if (mode == ASM_FILTER_SEQUENTIAL && state && (state[0] < 0 || state[0] > 255 || state[1] < 0 || state[1] > 255 || state[2] < 0))
        return fail(h, ASM_EINVAL, "asm_simd_ed_batch_async: state out of range");
    if (b->n == 0) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (const int rc = for_each_bucket(b, d_ed, [&](const asm_bucket& k, OutMap ev) {
            return launch_simd_ed_events(h, k, ed_threshold, shd_enable ? 1 : 0, ev, ed_mode);
        }))
        return rc;
    const long n = (long)b->n;
    const unsigned g = grid_for(b->n), t = ASM_BLOCK;
    if (ed_mode == ASM_LEAP_LOCAL || ed_mode == ASM_LEAP_SEMI_FREE_END) { /* no converge_ED, no carried state: SEQUENTIAL = CLEAN */
        HIPCHK(h, launch(h, simd_ed_final_kernel, g, t, d_ed, n));
        return ASM_OK;
    }
    if (mode == ASM_FILTER_CLEAN) {
        HIPCHK(h, launch(h, simd_ed_clean_kernel, g, t, d_ed, n, ed_threshold));
        return ASM_OK;
    }
    return simd_ed_resolve_sequential(h, d_ed, n, ed_threshold, state);
}

static int simd_ed_affine_launch(asm_handle* h, const asm_batch* b, int gap_threshold, int af_threshold, int x, int o, int e, int mode,
                                 int32_t* d_ed) {
    if (!h || !b || !d_ed) return fail(h, ASM_EINVAL, "asm_simd_ed_affine_batch_async: NULL argument");
    if (mode < ASM_LEAP_GLOBAL || mode > ASM_LEAP_SEMI_FREE_END)
        return fail(h, ASM_EINVAL, "asm_simd_ed_affine_mode_batch_async: mode must be one of ASM_LEAP_GLOBAL/LOCAL/SEMI_FREE_BEGIN/SEMI_FREE_END");
    if (gap_threshold < 1 || gap_threshold > ASM_FILTER_MAX_T)
        return fail(h, ASM_EINVAL, "asm_simd_ed_affine_batch_async: gap threshold must be in [1, 32]");
    if (af_threshold < 1 || af_threshold > 512)
        return fail(h, ASM_EINVAL, "asm_simd_ed_affine_batch_async: affine threshold must be in [1, 512]");
    if (x < 1 || x > 15 || o < 1 || o > 15 || e < 1 || e > o)
        return fail(h, ASM_EINVAL, "asm_simd_ed_affine_batch_async: penalties must satisfy 1 <= e <= o <= 15, 1 <= x <= 15");
    if (b->n == 0) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    /* the refusal is the thread-per-pair kernel's, for the whole call (simd_ed_affine_plan) */
    if (simd_ed_affine_plan(gap_threshold, x, o, e, b->n, b->maxlen).refused)
        return fail(h, ASM_EINVAL, "asm_simd_ed_affine_batch_async: generation rings exceed the LDS");
    return for_each_bucket(b, d_ed, [&](const asm_bucket& k, OutMap out) -> int {
        const SimdEdAffinePlan pl = simd_ed_affine_plan(gap_threshold, x, o, e, k.n, k.maxlen);
        const auto go = [&](auto kernel) {
            return launch_lds(h, kernel, (unsigned)pl.grid, pl.block, pl.lds, k.planes, k.lens, (long)k.n, k.w4, gap_threshold, af_threshold, x,
                              o, e, pl.gm, pl.gi, mode, out);
        };
        HIPCHK(h, pl.quad ? go(simd_ed_affine_quad_kernel) : go(simd_ed_affine_kernel<4>));
        return ASM_OK;
    });
}

int asm_simd_ed_affine_batch_async(asm_handle* h, const asm_batch* b, int gap_threshold, int af_threshold, int x, int o, int e,
                                   int32_t* d_ed) {
    return simd_ed_affine_launch(h, b, gap_threshold, af_threshold, x, o, e, ASM_LEAP_GLOBAL, d_ed);
}

int asm_simd_ed_affine_shd_batch_async(asm_handle* h, const asm_batch* b, int gap_threshold, int af_threshold, int x, int o, int e,
                                       int shd_threshold, int32_t* d_ed) {
    if (shd_threshold < 0) return fail(h, ASM_EINVAL, "asm_simd_ed_affine_shd_batch_async: SHD threshold must be in [0, min(16, gap threshold)]");
    return asm_simd_ed_affine_mode_batch_async(h, b, gap_threshold, af_threshold, x, o, e, shd_threshold, ASM_LEAP_GLOBAL, d_ed);
}

int asm_simd_ed_affine_mode_batch_async(asm_handle* h, const asm_batch* b, int gap_threshold, int af_threshold, int x, int o, int e,
                                        int shd_threshold, int mode, int32_t* d_ed) {
    if (shd_threshold < 0) return simd_ed_affine_launch(h, b, gap_threshold, af_threshold, x, o, e, mode, d_ed); /* SHD off */
    if (shd_threshold > ASM_SHD_MAX_ERROR || shd_threshold > gap_threshold)
        return fail(h, ASM_EINVAL, "asm_simd_ed_affine_shd_batch_async: SHD threshold must be in [0, min(16, gap threshold)] "
                                   "(the reference reads 2*SHD_threshold+1 of its 2*gap_threshold+1 lane masks)");
    const int rc = simd_ed_affine_launch(h, b, gap_threshold, af_threshold, x, o, e, mode, d_ed);
    if (rc != ASM_OK || b->n == 0) return rc;
    return for_each_bucket(b, d_ed, [&](const asm_bucket& k, OutMap out) -> int {
        HIPCHK(h, (with_const_of<2, 4>((k.maxlen + 63) / 64, [&](auto w) {
                   return launch(h, simd_affine_shd_kernel<decltype(w)::value>, grid_for(k.n), ASM_BLOCK, k.planes, k.lens, (long)k.n, k.w4,
                                 gap_threshold, shd_threshold, out);
               })));
        return ASM_OK;
    });
}

int asm_shd_filter_batch_async(asm_handle* h, const asm_batch* b, int max_error, int32_t* d_pass) {
    if (!h || !b || !d_pass) return fail(h, ASM_EINVAL, "asm_shd_filter_batch_async: NULL argument");
    if (max_error < 0 || max_error > ASM_SHD_MAX_ERROR)
        return fail(h, ASM_EINVAL, "asm_shd_filter_batch_async: max_error must be in [0, 16] (MAX_ERROR_AVX)");
    if (b->n == 0) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return for_each_bucket(b, d_pass, [&](const asm_bucket& k, OutMap out) -> int {
        HIPCHK(h, (with_const_of<2, 4>((k.maxlen + 63) / 64, [&](auto w) {
                   return launch(h, shd_kernel<decltype(w)::value>, grid_for(k.n), ASM_BLOCK, k.planes, k.lens, (long)k.n, k.w4, max_error, out);
               })));
        return ASM_OK;
    });
}
