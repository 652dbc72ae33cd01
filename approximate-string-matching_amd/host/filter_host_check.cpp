// Host build of the filters' per-thread core (csrc/asm_simd_ed.h) for the CPU test-suite, driven serially in the kernels' shapes:
//   filter_host_events     simd_ed_kernel's thread: load and clip, the mask-array SHD, run_levenshtein with the register column
//                          (form 0: T <= 8, ED_GLOBAL / SEMI_FREE_END) or the column in memory (form 1) -> one event per pair
//   filter_host_verdicts   the clean, final and sequential resolvers over the events; the two last-setter scans as serial loops
//   filter_host_affine     simd_ed_affine_kernel's thread (form 0, 256-bit vectors) or a serial mirror of simd_ed_affine_quad_kernel
//                          (form 1: four "threads" per pair over the staged dword planes, batches of at most 128 characters), then
//                          simd_affine_shd_kernel's thread
//   filter_host_shd        shd_kernel's thread
//   filter_host_quad_extend  simd_quad_extend on the staged planes against simd_extend(simd_lane_mask(d), st, len) on VW<2>
//   filter_host_selfcheck  all of the above on one batch in reduced size, the forms against each other, folded into one digest
// A batch is laid out as a bucket of the device batch is — planes [4][w4][n], lens — so that the strides are the kernels'.
// Built as a library for tests/test_filter_host.py and, with FILTER_HOST_CHECK_MAIN, as a stand-alone program (filter_host_check
// BATCH: prints the self-check's digest), which the same tests build under ASan + UBSan.  Test support only: nothing in the product
// links this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_simd_ed.h"

namespace {
struct Bucket { /* one width class: every pair of the batch */
    long n = 0;
    int w4 = 1, maxlen = 0;
    std::vector<lu_quad> planes;
    std::vector<uint32_t> lens;
    int words() const { return maxlen <= 128 ? 2 : 4; } /* simd_ed_plan */
    bool quad() const { return maxlen <= 128; }         /* simd_ed_affine_plan */
};

// bit_convert.cpp:340-355: A=00 C=01 G=10 T=11, anything else 00; plane 0 holds the low bit of base q at bit q
void fill(Bucket& b, int plane, long i, const unsigned char* s, int len) {
    for (int q = 0; q < len; q++) {
        const int code = s[q] == 'C' ? 1 : s[q] == 'G' ? 2 : s[q] == 'T' ? 3 : 0;
        for (int bit = 0; bit < 2; bit++) {
            if (!(code >> bit & 1)) continue;
            lu_quad& g = b.planes[((long)(plane + bit) * b.w4 + (q >> 7)) * b.n + i];
            uint32_t* const d[4] = {&g.x, &g.y, &g.z, &g.w};
            *d[(q >> 5) & 3] |= 1u << (q & 31);
        }
    }
}

bool load(Bucket& b, long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs, const uint32_t* ref_off) {
    b.n = n;
    for (long i = 0; i < n; i++) {
        const int m = (int)(read_off[i + 1] - read_off[i]), nn = (int)(ref_off[i + 1] - ref_off[i]);
        if (m > 0xffff || nn > 0xffff) return false;
        b.maxlen = m > b.maxlen ? m : b.maxlen, b.maxlen = nn > b.maxlen ? nn : b.maxlen;
    }
    b.w4 = b.maxlen > 128 ? (b.maxlen + 127) / 128 : 1;
    b.planes.assign((size_t)4 * b.w4 * (n > 0 ? n : 1), lu_quad{0u, 0u, 0u, 0u});
    b.lens.resize(n);
    for (long i = 0; i < n; i++) {
        const int m = (int)(read_off[i + 1] - read_off[i]), nn = (int)(ref_off[i + 1] - ref_off[i]);
        b.lens[i] = (uint32_t)m | ((uint32_t)nn << 16);
        fill(b, 0, i, reads + read_off[i], m), fill(b, 2, i, refs + ref_off[i], nn);
    }
    return true;
}

// ---- simd_ed_kernel's thread ------------------------------------------------------------------------------------------------------
template <int TT, int W64>
int event_reg(const SimdPair<W64>& p, int shd) {
    constexpr int NLC = 2 * TT + 1;
    VW<W64> hm[NLC];
    for (int j = 0; j < NLC; j++) hm[j] = simd_lane_mask<W64>(p, j - TT);
    if (shd && simd_shd_rejects<W64, NLC>(p, TT, [&](int j) -> const VW<W64>& { return hm[j]; })) return EV_REJECTED;
    return simd_lev_events_reg<TT, W64>(p, hm);
}
template <int W64>
int event_col(const SimdPair<W64>& p, int T, int shd, int ed_mode) {
    if (shd && simd_shd_rejects<W64, 0>(p, T, [&](int j) { return simd_lane_mask<W64>(p, j - T); })) return EV_REJECTED;
    std::vector<short> col((size_t)2 * (2 * T + 3)); /* the thread's LDS column, exactly */
    return simd_lev_events_col<W64>(p, T, simd_all_start(ed_mode), SimdEndColumn<1>{col.data(), 2 * T + 3});
}
template <int W64>
int event_one(const Bucket& b, long i, int T, int shd, int ed_mode, int form) {
    const SimdPair<W64> p = simd_load_pair<W64>(b.planes.data(), b.lens.data(), b.n, b.w4, i);
    if (form == 1) return event_col<W64>(p, T, shd, ed_mode);
    switch (T) {
        case 1: return event_reg<1, W64>(p, shd);
        case 2: return event_reg<2, W64>(p, shd);
        case 3: return event_reg<3, W64>(p, shd);
        case 4: return event_reg<4, W64>(p, shd);
        case 5: return event_reg<5, W64>(p, shd);
        case 6: return event_reg<6, W64>(p, shd);
        case 7: return event_reg<7, W64>(p, shd);
        default: return event_reg<8, W64>(p, shd);
    }
}

// ---- the affine kernels' threads --------------------------------------------------------------------------------------------------------
// the generation loop of both kernels, `threads` of them per pair taking turns where the device has a fence
template <typename EnT, class Extend>
int affine_run(const SimdAffine& a, int len, int threads, Extend extend) {
    const LvRings rg = LvRings::pow2(a.x, a.o, a.ext);
    const int rows = 2 * a.T + 3;
    std::vector<EnT> ring(rg.ring_bytes(rows, 1, sizeof(EnT)) / sizeof(EnT), 0); /* one column, zero = never reached */
    const SimdAffineRings<EnT> r{ring.data(), ring.data() + rg.gm * rows, ring.data() + (rg.gm + rg.gi) * rows, rg, rows, 1};
    bool exact = false;
    for (int q = 0; q < threads; q++) exact = simd_affine_seed(r, a, len, q, threads, extend) || exact;
    int result = exact ? a.exact() : -2;
    for (int e = 1; e <= a.af_t && result == -2; e++) {
        int conv = SIMD_AF_NONE;
        for (int q = 0; q < threads; q++) {
            const int c = simd_affine_generation(r, a, len, e, q, threads, extend);
            conv = c < conv ? c : conv;
        }
        if (conv != SIMD_AF_NONE) result = conv;
    }
    return result == -2 ? -1 : result;
}
int affine_thread(const Bucket& b, long i, const SimdAffine& a) {
    const SimdPair<4> p = simd_load_pair<4>(b.planes.data(), b.lens.data(), b.n, b.w4, i);
    return affine_run<uint16_t>(a, p.len, 1, [&](int d, int st) { return simd_extend<4>(simd_lane_mask<4>(p, d), st, p.len); });
}
struct QuadPlanes {
    uint32_t pl[SIMD_QUAD_PW]; /* what one pair owns in the kernel's LDS */
    int len;
};
QuadPlanes quad_stage(const Bucket& b, long i) {
    QuadPlanes s;
    memset(s.pl, 0xff, sizeof s.pl); /* whatever the LDS held before */
    const SimdClip c = simd_clip(b.lens[i], 128);
    s.len = c.len;
    for (int q = 0; q < 4; q++) simd_quad_stage(s.pl + q * SIMD_QUAD_PD, b.planes[((long)q * b.w4) * b.n + i], q < 2 ? c.len : c.ref);
    return s;
}
int affine_quad(const Bucket& b, long i, const SimdAffine& a) {
    const QuadPlanes s = quad_stage(b, i);
    return affine_run<uint8_t>(a, s.len, 4, [&](int d, int st) { return simd_quad_extend(s.pl, d, st, s.len); });
}
template <int W64>
bool affine_shd_rejects(const Bucket& b, long i, int gap_t, int shd_t) {
    const SimdPair<W64> p = simd_load_pair<W64>(b.planes.data(), b.lens.data(), b.n, b.w4, i);
    return simd_shd_rejects<W64, 0>(p, shd_t, [&](int j) { return simd_lane_mask<W64>(p, j - gap_t); });
}

void events(const Bucket& b, int T, int shd, int ed_mode, int form, int32_t* ev) {
    for (long i = 0; i < b.n; i++) ev[i] = b.words() == 2 ? event_one<2>(b, i, T, shd, ed_mode, form) : event_one<4>(b, i, T, shd, ed_mode, form);
}
void affine(const Bucket& b, const SimdAffine& a, int shd_t, int form, int32_t* out) {
    for (long i = 0; i < b.n; i++) {
        out[i] = form == 1 && b.quad() ? affine_quad(b, i, a) : affine_thread(b, i, a);
        if (shd_t >= 0 && (b.words() == 2 ? affine_shd_rejects<2>(b, i, a.T, shd_t) : affine_shd_rejects<4>(b, i, a.T, shd_t))) out[i] = -1;
    }
}
void shd(const Bucket& b, int max_error, int32_t* out) {
    for (long i = 0; i < b.n; i++)
        out[i] = b.words() == 2 ? shd_pass<2>(simd_load_pair<2>(b.planes.data(), b.lens.data(), b.n, b.w4, i), max_error)
                                : shd_pass<4>(simd_load_pair<4>(b.planes.data(), b.lens.data(), b.n, b.w4, i), max_error);
}
// how: 0 clean, 1 final (ED_modes LOCAL / SEMI_FREE_END), 2 sequential from state[3] = (final_ED, lane, converge_ED), which moves on
void verdicts(long n, int32_t* ev_to_ed, int T, int how, int32_t* state) {
    if (how != 2) {
        for (long i = 0; i < n; i++) ev_to_ed[i] = how == 0 ? simd_verdict_clean(ev_to_ed[i], T) : simd_verdict_final(ev_to_ed[i]);
        return;
    }
    const LastSetter last;
    std::vector<int32_t> after(n);
    int32_t run = -1;
    for (long i = 0; i < n; i++) after[i] = run = last(run, simd_setter_key(ev_to_ed[i]));
    const int32_t last_setter = run;
    run = -1;
    for (long i = 0; i < n; i++) after[i] = run = last(run, simd_converge_key(ev_to_ed[i], after[i], state[0], state[1]));
    for (long i = 0; i < n; i++) ev_to_ed[i] = simd_verdict_sequential(ev_to_ed[i], i > 0 ? after[i - 1] : -1, after[i], T, state[2]);
    if (last_setter >= 0) state[0] = last_setter & 0xff, state[1] = last_setter >> 8;
    if (run >= 0) state[2] = run;
}
// pairs x shifts x starts at which the quad extension and the vector one part
long quad_extend_differ(const Bucket& b) {
    long bad = 0;
    for (long i = 0; i < b.n; i++) {
        const QuadPlanes s = quad_stage(b, i);
        const SimdPair<2> p = simd_load_pair<2>(b.planes.data(), b.lens.data(), b.n, b.w4, i);
        for (int d = -32; d <= 32; d++) {
            const VW<2> mask = simd_lane_mask<2>(p, d);
            for (int st = 0; st <= s.len; st++) bad += simd_quad_extend(s.pl, d, st, s.len) != simd_extend<2>(mask, st, p.len) || s.len != p.len;
        }
    }
    return bad;
}
}  // namespace

#define FILTER_LOAD                                                  \
    Bucket b;                                                        \
    if (!load(b, n, reads, read_off, refs, ref_off)) return -2

// ev[i]: the event of pair i.  form 0 needs T in [1, 8] and ed_mode 0 or 3.
extern "C" int filter_host_events(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                                  const uint32_t* ref_off, int T, int shd, int ed_mode, int form, int32_t* ev) {
    if (T < 1 || T > ASM_FILTER_MAX_T || (shd && T > ASM_SHD_MAX_ERROR) || ed_mode < 0 || ed_mode > 3 || form < 0 || form > 1) return -1;
    if (form == 0 && (T > ASM_FILTER_REG_MAX_T || simd_all_start(ed_mode))) return -1;
    FILTER_LOAD;
    events(b, T, shd, ed_mode, form, ev);
    return 0;
}
extern "C" int filter_host_verdicts(long n, int32_t* ev_to_ed, int T, int how, int32_t* state) {
    if (how < 0 || how > 2 || (how == 2 && !state)) return -1;
    verdicts(n, ev_to_ed, T, how, state);
    return 0;
}
// shd_t < 0: SHD off
extern "C" int filter_host_affine(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                                  const uint32_t* ref_off, int T, int af_t, int x, int o, int ext, int mode, int shd_t, int form,
                                  int32_t* out) {
    if (T < 1 || T > ASM_FILTER_MAX_T || af_t < 1 || x < 1 || x > 15 || o < 1 || o > 15 || ext < 1 || ext > o || mode < 0 || mode > 3 ||
        shd_t > ASM_SHD_MAX_ERROR || shd_t > T || form < 0 || form > 1)
        return -1;
    FILTER_LOAD;
    affine(b, SimdAffine{T, af_t, x, o, ext, mode}, shd_t, form, out);
    return 0;
}
extern "C" int filter_host_shd(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                               const uint32_t* ref_off, int max_error, int32_t* out) {
    if (max_error < 0 || max_error > ASM_SHD_MAX_ERROR) return -1;
    FILTER_LOAD;
    shd(b, max_error, out);
    return 0;
}
// every d in [-32, 32] and every st in [0, len] of every pair; *differ = the number of (pair, d, st) at which the two extensions part
extern "C" int filter_host_quad_extend(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                                       const uint32_t* ref_off, int64_t* differ) {
    FILTER_LOAD;
    if (!b.quad()) return -1;
    *differ = quad_extend_differ(b);
    return 0;
}

// The whole core on one batch: *digest folds every result; the return value counts the places where two forms of the same function
// part (register against memory column, quad against thread per pair, quad extension against the vector one): 0 when all is well.
extern "C" long filter_host_selfcheck(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                                      const uint32_t* ref_off, uint64_t* digest) {
    FILTER_LOAD;
    uint64_t h = 0xcbf29ce484222325ull;
    long bad = 0;
    std::vector<int32_t> a(n), c(n);
    const auto fold = [&](const std::vector<int32_t>& v) {
        for (long i = 0; i < n; i++) h = (h ^ (uint32_t)v[i]) * 0x100000001b3ull;
    };
    const auto differ = [&]() {
        for (long i = 0; i < n; i++) bad += a[i] != c[i];
    };
    int32_t state[3] = {1, 1, 2};
    for (int T : {1, 3, 8, 9, 16, 32})
        for (int shd_on = 0; shd_on <= (T <= ASM_SHD_MAX_ERROR ? 1 : 0); shd_on++)
            for (int ed_mode = 0; ed_mode < 4; ed_mode++) {
                events(b, T, shd_on, ed_mode, 1, a.data());
                if (T <= ASM_FILTER_REG_MAX_T && !simd_all_start(ed_mode)) events(b, T, shd_on, ed_mode, 0, c.data()), differ();
                fold(a);
                c = a, verdicts(n, c.data(), T, ed_mode == 1 || ed_mode == 3 ? 1 : 0, nullptr), fold(c);
                if (ed_mode == 0 || ed_mode == 2) verdicts(n, a.data(), T, 2, state), fold(a);
            }
    h = ((h ^ (uint32_t)state[0]) * 31 ^ (uint32_t)state[1]) * 31 ^ (uint32_t)state[2];
    static const int settings[3][5] = {{3, 60, 2, 3, 1}, {8, 100, 4, 6, 2}, {32, 200, 15, 15, 15}};
    for (const auto& s : settings)
        for (int mode = 0; mode < 4; mode++)
            for (int shd_t : {-1, 0, s[0] < 16 ? s[0] : 16}) {
                const SimdAffine af{s[0], s[1], s[2], s[3], s[4], mode};
                affine(b, af, shd_t, 0, a.data());
                if (b.quad()) affine(b, af, shd_t, 1, c.data()), differ();
                fold(a);
            }
    for (int e : {0, 1, 16}) shd(b, e, a.data()), fold(a);
    if (b.quad()) bad += quad_extend_differ(b);
    *digest = h;
    return bad;
}

#ifdef FILTER_HOST_CHECK_MAIN
// Stand-alone form (the one a sanitizer build takes): filter_host_check BATCH.  BATCH holds one batch as the tests have it in memory —
// int32 n, uint32 read_off[n+1], uint32 ref_off[n+1], then the reads' bytes and the references' — in arrays of exactly that size.
// Prints the self-check's digest; exit status 1 when two forms part.
int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s batch\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || fread(&n, sizeof n, 1, f) != 1 || n < 0) return fprintf(stderr, "%s: cannot read\n", argv[1]), 2;
    std::vector<uint32_t> ro((size_t)n + 1), fo((size_t)n + 1);
    if (fread(ro.data(), 4, ro.size(), f) != ro.size() || fread(fo.data(), 4, fo.size(), f) != fo.size()) return 2;
    std::vector<unsigned char> reads(ro[n]), refs(fo[n]);
    if (fread(reads.data(), 1, reads.size(), f) != reads.size() || fread(refs.data(), 1, refs.size(), f) != refs.size()) return 2;
    fclose(f);
    uint64_t digest = 0;
    const long bad = filter_host_selfcheck(n, reads.data(), ro.data(), refs.data(), fo.data(), &digest);
    printf("%016llx %ld\n", (unsigned long long)digest, bad);
    return bad ? 1 : 0;
}
#endif
