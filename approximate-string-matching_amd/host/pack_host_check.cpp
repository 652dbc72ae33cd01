// Host build of pack_kernel's per-thread pieces (csrc/asm_pack.h): the very pack_vec a thread runs per 16-byte vector and the very
// pack_cut_begin / pack_cut_granule it cuts its string out with, driven on the CPU and compared with the oracle's conversion
// (planes_of of oracle/asm_oracle.c, linked in through host/pack_oracle_planes.c).  The device primitives take their plain meaning.
// A stand-alone program (tests/test_pack_host.py builds it under ASan + UBSan): the plane arrays are allocated at exactly the
// size the kernel's LDS rule gives them, so a read past them is the sanitizer's to report.  Test support only.
//   pack_host_check bytes      every byte value at every position of a vector, among bases and among non-bases
//   pack_host_check cut W4     the cut at the lengths of its list and byte offsets 0..47, for W4 = 1 or 2
// Prints "<what> <cases> ok" and returns 0, or prints the first mismatches and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_pack.h"

extern "C" void pack_oracle_planes(const uint8_t* buf128, uint64_t* out);

namespace {
int g_bad = 0;

// planes of a string of up to 128 * w4 characters as the oracle gives them: dword w of granule g of plane p at out[(p * w4 + g) * 4 + w]
void oracle_string(const uint8_t* s, int len, int w4, std::vector<uint32_t>& out) {
    out.assign((size_t)8 * w4, 0u);
    for (int g = 0; g < w4; g++) {
        uint8_t buf[128];
        memset(buf, 0, sizeof buf); /* beyond the string: NUL, code 00 */
        const int part = len - 128 * g < 0 ? 0 : (len - 128 * g > 128 ? 128 : len - 128 * g);
        memcpy(buf, s + 128 * g, (size_t)part);
        uint64_t pl[4];
        pack_oracle_planes(buf, pl);
        for (int p = 0; p < 2; p++)
            for (int w = 0; w < 4; w++) out[(size_t)(p * w4 + g) * 4 + w] = (uint32_t)(pl[2 * p + (w >> 1)] >> (32 * (w & 1)));
    }
}

uint4 load_vec(const uint8_t* b) {
    uint32_t d[4];
    memcpy(d, b, 16);
    return make_uint4(d[0], d[1], d[2], d[3]);
}

int check_bytes() {
    static const char* const fills[2] = {"ACGTTGCAACGTGTCA", "N\0nacgt-*B\xff\x80@RU."};
    int cases = 0;
    for (int f = 0; f < 2; f++)
        for (int pos = 0; pos < 16; pos++)
            for (int val = 0; val < 256; val++, cases++) {
                uint8_t buf[128];
                memset(buf, 0, sizeof buf);
                memcpy(buf, fills[f], 16);
                buf[pos] = (uint8_t)val;
                uint32_t p0, p1;
                pack_vec(load_vec(buf), p0, p1);
                uint64_t pl[4];
                pack_oracle_planes(buf, pl);
                if (p0 != (uint32_t)(pl[0] & 0xffffu) || p1 != (uint32_t)(pl[2] & 0xffffu)) {
                    if (g_bad++ < 8)
                        printf("bytes: fill %d position %d value 0x%02x: planes %04x %04x, oracle %04x %04x\n", f, pos, val, p0, p1,
                               (unsigned)(pl[0] & 0xffffu), (unsigned)(pl[2] & 0xffffu));
                }
                const bool base = val == 'C' || val == 'G' || val == 'T';
                if (((((p0 | p1) >> pos) & 1u) != 0u) != base) g_bad++; /* exactly 'C', 'G', 'T' set bits */
            }
    return cases;
}

template <int W4>
int check_cut(const int* lens, int nlens) {
    int cases = 0;
    uint32_t seed = 12345u;
    for (int li = 0; li < nlens; li++)
        for (uint32_t off = 0; off < 48; off++, cases++) {
            const int len = lens[li];
            // the range: `off` bytes of the strings before, the string, and a 'T' where the next string starts
            const int bytes = (int)off + len + 1, nv = (bytes + 15) >> 4, pd = pack_plane_dwords(nv);
            std::vector<uint8_t> text((size_t)16 * nv, (uint8_t)'T');
            for (int q = 0; q < (int)off + len; q++) seed = seed * 1664525u + 1013904223u, text[(size_t)q] = (uint8_t)"ACGT"[seed >> 30];
            // the kernel's conversion of the range: vector v -> u16 v of each plane array; what no vector wrote stays all ones
            uint32_t* const P0 = (uint32_t*)malloc(4 * (size_t)pd);
            uint32_t* const P1 = (uint32_t*)malloc(4 * (size_t)pd);
            memset(P0, 0xff, 4 * (size_t)pd), memset(P1, 0xff, 4 * (size_t)pd);
            for (int v = 0; v < nv; v++) {
                uint32_t p0, p1;
                pack_vec(load_vec(&text[(size_t)16 * v]), p0, p1);
                const uint16_t h0 = (uint16_t)p0, h1 = (uint16_t)p1;
                memcpy((uint8_t*)P0 + 2 * v, &h0, 2), memcpy((uint8_t*)P1 + 2 * v, &h1, 2);
            }
            std::vector<uint32_t> want;
            oracle_string(&text[off], len, W4, want);
            PackCut c = pack_cut_begin(P0, P1, off, len);
            for (int g = 0; g < W4; g++) {
                uint4 v0, v1;
                pack_cut_granule(P0, P1, c, len, g, v0, v1);
                const uint32_t got[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                for (int p = 0; p < 2; p++)
                    for (int w = 0; w < 4; w++)
                        if (got[4 * p + w] != want[(size_t)(p * W4 + g) * 4 + w]) {
                            if (g_bad++ < 8)
                                printf("cut W4 %d: length %d offset %u granule %d plane %d dword %d: %08x, oracle %08x\n", W4, len, off, g, p, w,
                                       got[4 * p + w], want[(size_t)(p * W4 + g) * 4 + w]);
                        }
            }
            free(P0), free(P1);
        }
    return cases;
}
}  // namespace

int main(int argc, char** argv) {
    static const int lens1[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128};
    static const int lens2[] = {129, 160, 255, 256};
    int cases = -1;
    if (argc == 2 && !strcmp(argv[1], "bytes")) cases = check_bytes();
    if (argc == 3 && !strcmp(argv[1], "cut") && !strcmp(argv[2], "1")) cases = check_cut<1>(lens1, (int)(sizeof lens1 / sizeof *lens1));
    if (argc == 3 && !strcmp(argv[1], "cut") && !strcmp(argv[2], "2")) cases = check_cut<2>(lens2, (int)(sizeof lens2 / sizeof *lens2));
    if (cases < 0) {
        fprintf(stderr, "usage: pack_host_check bytes | cut 1 | cut 2\n");
        return 2;
    }
    if (g_bad) {
        printf("%s %d cases, %d mismatches\n", argv[1], cases, g_bad);
        return 1;
    }
    printf("%s %d ok\n", argv[1], cases);
    return 0;
}
