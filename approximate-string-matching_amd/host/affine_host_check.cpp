// Host build of what the general-penalty kernels share (csrc/asm_affine.h) for the CPU test-suite, driven pair by pair:
//   affine_host_nw        gotoh_sweep with the empty sink: what nw_affine_kernel runs per thread
//   affine_host_nw_cigar  gotoh_sweep with the trace sink, then gotoh_traceback: what nw_trace_affine_kernel runs per thread
//   affine_host_leap      a plain single-thread LV loop built from lv_affine_step, LvRingView and LvRings, with the lane masks and the
//                         scan of asm_leapunit.h: the shape of leap_general_kernel with the band a run-time value
// so that tests/test_affine_host.py can diff them against the oracle without a GPU.  Built as a library for the tests and, with
// AFFINE_HOST_CHECK_MAIN, as a stand-alone program, which the same tests build under ASan + UBSan and run on the same batches.  Test support only: nothing in the product
// links this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_affine.h"

namespace {
constexpr int W64 = 2; /* strings up to 128 */

// bit_convert.cpp:340-355: A=00 C=01 G=10 T=11, anything else 00; plane 0 holds the low bit of base q at bit q
void fill(VW<W64>& p0, VW<W64>& p1, const unsigned char* s, int len) {
    memset(&p0, 0, sizeof p0), memset(&p1, 0, sizeof p1);
    for (int q = 0; q < len; q++) {
        const int code = s[q] == 'C' ? 1 : s[q] == 'G' ? 2 : s[q] == 'T' ? 3 : 0;
        if (code & 1) p0.w[q >> 6] |= 1ull << (q & 63);
        if (code & 2) p1.w[q >> 6] |= 1ull << (q & 63);
    }
}

struct Pair {
    VW<W64> A0, A1, B0, B1;
    int m, nn;
    bool load(long i, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs, const uint32_t* ref_off) {
        m = (int)(read_off[i + 1] - read_off[i]), nn = (int)(ref_off[i + 1] - ref_off[i]);
        if (m > 64 * W64 || nn > 64 * W64) return false;
        fill(A0, A1, reads + read_off[i], m), fill(B0, B1, refs + ref_off[i], nn);
        return true;
    }
};

// LV::run (LV_BAG.cpp:127-245), ED_GLOBAL, one pair: rings [slot][lane], one column
int leap_one(const Pair& P, int k, int x, int o, int ext) {
    const int nl = 2 * k + 1, len = P.m > P.nn ? P.m : P.nn;
    const LvRings rg = LvRings::pow2(x, o, ext);
    std::vector<uint16_t> ring(rg.ring_bytes(nl, 1, sizeof(uint16_t)) / sizeof(uint16_t) + 1, 0); /* zero = never reached */
    uint16_t* const r_en = ring.data();
    uint16_t* const r_ip = r_en + rg.gm * nl;
    uint16_t* const r_dp = r_ip + rg.gi * nl;
    const VW<W64> VA = vw_low_ones<W64>(P.m), VB = vw_low_ones<W64>(P.nn);
    std::vector<VW<W64>> mask(nl);
    for (int j = 0; j < nl; j++) mask[j] = leap_lane_mask<W64>(P.A0, P.A1, P.B0, P.B1, VA, VB, j - k);
    {
        int e0 = vw_next_one<W64>(mask[k], 0);
        e0 = e0 > len ? len : e0;
        r_en[k] = (uint16_t)(e0 + 2);
        if (e0 == len) return 0;
    }
    for (int e = 1; e <= ASM_LEAP_AF_THRESHOLD; e++) {
        const LvRingView<uint16_t> g(r_en, r_ip, r_dp, rg, nl, e, x, o, ext);
        bool pass = false;
        for (int j = 0; j < nl; j++) {
            const int d = j - k;
            const int e_up = j > 0 ? (int)g.en_o[j - 1] - 2 : -2, i_up = j > 0 ? (int)g.ip_e[j - 1] - 2 : -2;
            const int e_dn = j < nl - 1 ? (int)g.en_o[j + 1] - 2 : -2, d_dn = j < nl - 1 ? (int)g.dp_e[j + 1] - 2 : -2;
            const LvStep s = lv_affine_step(e_up, i_up, e_dn, d_dn, (int)g.en_x[j] - 2, d >= 0, d <= 0);
            int enew = -2;
            if (s.st >= 0) {
                int r = vw_next_one<W64>(mask[j], s.st > len ? len : s.st);
                r = r > len ? len : r;
                enew = r > s.st ? r : s.st;
                if (enew == len && e + affine_gap(d < 0 ? -d : d, o, ext) <= ASM_LEAP_AF_THRESHOLD) pass = true;
            }
            g.en_w[j] = (uint16_t)(enew + 2), g.ip_w[j] = (uint16_t)(s.inew + 2), g.dp_w[j] = (uint16_t)(s.dnew + 2);
        }
        if (pass) return e;
    }
    return -1;
}
}  // namespace

extern "C" int affine_host_nw(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                              const uint32_t* ref_off, int x, int o, int e, int32_t* out) {
    std::vector<uint32_t> bound(64 * W64 + 1);
    for (long i = 0; i < n; i++) {
        Pair P;
        if (!P.load(i, reads, read_off, refs, ref_off)) return -2;
        NoCellSink sink;
        out[i] = gotoh_sweep<W64>(P.A0, P.A1, P.B0, P.B1, P.m, P.nn, x, o, e, bound.data(), 1, sink);
    }
    return 0;
}

// cigars: n rows of `stride` bytes, the oracle's text form ("12=1X3D", NUL-terminated, cut where the row ends)
extern "C" int affine_host_nw_cigar(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                                    const uint32_t* ref_off, int x, int o, int e, int32_t* out, char* cigars, int stride) {
    std::vector<uint32_t> bound(64 * W64 + 1);
    struct Run {
        int op, count;
    };
    std::vector<Run> list;
    for (long i = 0; i < n; i++) {
        Pair P;
        if (!P.load(i, reads, read_off, refs, ref_off)) return -2;
        const int rows = P.m > 0 ? P.m : 1, cols8 = (P.nn + 7) / 8 > 0 ? (P.nn + 7) / 8 : 1;
        std::vector<uint32_t> scratch((size_t)rows * cols8, 0u); /* exactly the dwords a pair of these lengths may touch */
        GotohTraceSink trace{scratch.data(), 1, 0, cols8, {}};
        out[i] = gotoh_sweep<W64>(P.A0, P.A1, P.B0, P.B1, P.m, P.nn, x, o, e, bound.data(), 1, trace);
        list.clear();
        int read_left = P.m;
        bool starts_ok = true;
        auto runs = [&](int op, int count, int at) {
            list.push_back(Run{op, count});
            if (op != 2) read_left -= count;
            starts_ok = starts_ok && at == read_left; /* `at`: the read position the run starts at */
        };
        gotoh_traceback<W64>(P.A0, P.A1, P.B0, P.B1, P.m, P.nn, trace, runs);
        if (!starts_ok || read_left != 0) return -3;
        char* row = cigars + (size_t)i * stride;
        int len = 0;
        row[0] = 0;
        for (size_t q = list.size(); q-- > 0;) {
            const int w = snprintf(row + len, stride - len, "%d%c", list[q].count, "?ID=X"[list[q].op]);
            if (w > 0 && len + w < stride) len += w;
        }
    }
    return 0;
}

// k = band half-width (any k >= 1 with 2k+1 lanes of 128 bits in memory); out[i] = final_ED or -1
extern "C" int affine_host_leap(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                                const uint32_t* ref_off, int k, int x, int o, int e, int32_t* out) {
    if (k < 1 || k > 63 || x < 1 || o < 1 || e < 1) return -1;
    for (long i = 0; i < n; i++) {
        Pair P;
        if (!P.load(i, reads, read_off, refs, ref_off)) return -2;
        out[i] = leap_one(P, k, x, o, e);
    }
    return 0;
}

#ifdef AFFINE_HOST_CHECK_MAIN
// Stand-alone form (the one a sanitizer build takes): affine_host_check BATCH k x o e.  BATCH holds one batch as the tests have it in
// memory — int32 n, uint32 read_off[n+1], uint32 ref_off[n+1], then the reads' bytes and the references' — in arrays of exactly
// that size, so that a read beyond either end is one a sanitizer sees.  Prints per pair: sweep score, traced score, LEAP, CIGAR.
int main(int argc, char** argv) {
    if (argc != 6) return fprintf(stderr, "usage: %s batch k x o e\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || fread(&n, sizeof n, 1, f) != 1 || n < 0) return fprintf(stderr, "%s: cannot read\n", argv[1]), 2;
    std::vector<uint32_t> ro((size_t)n + 1), fo((size_t)n + 1);
    if (fread(ro.data(), 4, ro.size(), f) != ro.size() || fread(fo.data(), 4, fo.size(), f) != fo.size()) return 2;
    std::vector<unsigned char> reads(ro[n]), refs(fo[n]);
    if (fread(reads.data(), 1, reads.size(), f) != reads.size() || fread(refs.data(), 1, refs.size(), f) != refs.size()) return 2;
    fclose(f);
    const int k = atoi(argv[2]), x = atoi(argv[3]), o = atoi(argv[4]), e = atoi(argv[5]), stride = 1024;
    std::vector<int32_t> score(n), traced(n), leap(n);
    std::vector<char> cig((size_t)n * stride + 1);
    if (affine_host_nw(n, reads.data(), ro.data(), refs.data(), fo.data(), x, o, e, score.data()) ||
        affine_host_nw_cigar(n, reads.data(), ro.data(), refs.data(), fo.data(), x, o, e, traced.data(), cig.data(), stride) ||
        affine_host_leap(n, reads.data(), ro.data(), refs.data(), fo.data(), k, x, o, e, leap.data()))
        return 3;
    for (int32_t i = 0; i < n; i++) printf("%d %d %d %s\n", score[i], traced[i], leap[i], cig.data() + (size_t)i * stride);
    return 0;
}
#endif
