// Host build of the unit-penalty LEAP core (csrc/asm_leapunit.h) for the CPU test-suite: the very functions a thread of
// leap_unit_kernel and leap_unit_hint_kernel runs for its pair — leap_unit_generic<K, W64>, the form every width ran before, and
// leap_unit_w2<K>, the one-granule form — driven pair by pair on the host, so that tests/test_leap_unit_host.py can diff old
// against new and both against the oracle without a GPU.  The device primitives take their plain C++ meaning here.
// Built as a library for the tests and, with LEAP_HOST_CHECK_MAIN, as a stand-alone program (the form a sanitizer build takes).
// Test support only: nothing in the product links this file.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../csrc/asm_leapunit.h"

namespace {
// bit_convert.cpp:340-355: A=00 C=01 G=10 T=11, anything else 00; plane 0 holds the low bit of base q at bit q
template <int W64>
void fill(VW<W64>& p0, VW<W64>& p1, const unsigned char* s, int len) {
    memset(&p0, 0, sizeof p0), memset(&p1, 0, sizeof p1);
    for (int q = 0; q < len; q++) {
        const int code = s[q] == 'C' ? 1 : s[q] == 'G' ? 2 : s[q] == 'T' ? 3 : 0;
        if (code & 1) p0.w[q >> 6] |= 1ull << (q & 63);
        if (code & 2) p1.w[q >> 6] |= 1ull << (q & 63);
    }
}

// form 0: leap_unit_generic<K, W64>; 1: leap_unit_core<K, W64> (what the kernels call); 2: leap_unit_w2<K, true> (W64 == 2 only:
// the clamp-free lane step with the clamped one beside it, *differ counting the lane steps where the two part)
template <int K, int W64>
int one(int form, const unsigned char* a, int m, const unsigned char* b, int nn, int* differ) {
    VW<W64> A0, A1, B0, B1;
    fill<W64>(A0, A1, a, m), fill<W64>(B0, B1, b, nn);
    if (form == 0) return leap_unit_generic<K, W64>(A0, A1, B0, B1, m, nn);
    if (form == 1) return leap_unit_core<K, W64>(A0, A1, B0, B1, m, nn);
    if constexpr (W64 == 2) return leap_unit_w2<K, true>(A0, A1, B0, B1, m, nn, differ);
    return -3;
}

template <int K>
int by_width(int form, int W64, const unsigned char* a, int m, const unsigned char* b, int nn, int* differ) {
    return W64 == 2 ? one<K, 2>(form, a, m, b, nn, differ) : one<K, 3>(form, a, m, b, nn, differ);
}
}  // namespace

// out[i] = the chosen form's result for pair i (final_ED, or -1); *differ (may be null) is raised once per lane step of form 2
// in which the unclamped scan and the clamped one disagree.  k = 1, 2, 3 or 5; W64 = 2 (strings up to 128) or 3 (up to 192).
// Returns 0, or -1 for a k or width this build does not hold, -2 for a pair too long for W64.
extern "C" int leap_host_unit(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                              const uint32_t* ref_off, int k, int W64, int form, int32_t* out, int64_t* differ) {
    if ((W64 != 2 && W64 != 3) || form < 0 || form > 2 || (form == 2 && W64 != 2)) return -1;
    int d = 0;
    for (long i = 0; i < n; i++) {
        const unsigned char* a = reads + read_off[i];
        const unsigned char* b = refs + ref_off[i];
        const int m = (int)(read_off[i + 1] - read_off[i]), nn = (int)(ref_off[i + 1] - ref_off[i]);
        if (m > 64 * W64 || nn > 64 * W64) return -2;
        switch (k) {
            case 1: out[i] = by_width<1>(form, W64, a, m, b, nn, &d); break;
            case 2: out[i] = by_width<2>(form, W64, a, m, b, nn, &d); break;
            case 3: out[i] = by_width<3>(form, W64, a, m, b, nn, &d); break;
            case 5: out[i] = by_width<5>(form, W64, a, m, b, nn, &d); break;
            default: return -1;
        }
    }
    if (differ != nullptr) *differ = d;
    return 0;
}

#ifdef LEAP_HOST_CHECK_MAIN
// Stand-alone form: seeded pairs over every length 1..128 and k = 1, 2, 3, old against new and clamped against unclamped.
int main() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() {
        rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
        return (uint32_t)(rng >> 32);
    };
    long pairs = 0, bad = 0;
    for (int rep = 0; rep < 40; rep++)
        for (int m = 1; m <= 128; m++) {
            unsigned char a[128], b[128];
            for (int q = 0; q < m; q++) a[q] = "ACGT"[next() & 3];
            int nn = 0;
            static const uint32_t rates[4] = {0, 100, 300, 1000}; /* edits per thousand bases of this repetition */
            const uint32_t rate = rates[rep % 4];
            for (int q = 0; q < m && nn < 128; q++) {
                const uint32_t u = next() % 1000;
                if (u < rate / 3) continue; /* deletion */
                b[nn++] = u < rate ? "ACGT"[next() & 3] : a[q];
                if (u >= 1000 - rate / 3 && nn < 128) b[nn++] = "ACGT"[next() & 3]; /* insertion */
            }
            if (nn == 0) b[nn++] = 'A';
            const uint32_t ro[2] = {0, (uint32_t)m}, fo[2] = {0, (uint32_t)nn};
            for (int k = 1; k <= 3; k++) {
                int32_t r0 = 0, r1 = 0, r2 = 0;
                int64_t d = 0;
                if (leap_host_unit(1, a, ro, b, fo, k, 2, 0, &r0, nullptr) || leap_host_unit(1, a, ro, b, fo, k, 2, 1, &r1, nullptr) ||
                    leap_host_unit(1, a, ro, b, fo, k, 2, 2, &r2, &d))
                    return 2;
                pairs++;
                if (r0 != r1 || r0 != r2 || d != 0) {
                    bad++;
                    printf("m=%d n=%d k=%d: generic %d core %d checked %d, %ld lane steps differ\n", m, nn, k, r0, r1, r2, (long)d);
                }
            }
        }
    printf("%ld pairs, %ld differ\n", pairs, bad);
    return bad ? 1 : 0;
}
#endif
