// pack_kernel's per-thread pieces (asm_kernels.h): the conversion of one 16-byte vector of ASCII into 16 bits of each plane, and the cut
// of one string out of the position-space plane arrays.  The header compiles for the host as well (ASM_HD, as asm_bits.h):
// host/pack_host_check.cpp runs these very functions on the CPU against the oracle's conversion (tests/test_pack_host.py).  Each
// primitive that is one instruction on the device keeps that instruction there and has its plain meaning beside it.
//
// Written by opcode price (docs/design/kernels.md, `pack_kernel<W4>`; profiles/pack_valu_rates.txt): a VOP2 operation issues in about
// 2.2 cycles per wave-instruction on this chip and every VOP3 one (v_perm_b32, v_dot4_u32_u8, v_lshl_or_b32, v_bitop3_b32 ...) in
// about 4.2, so the conversion below is counted in VOP3 operations: 4 look-ups, 2 merges, 4 dots and 2 joins per 16 characters.
#pragma once
#include <stdint.h>

#include "asm_bits.h"

#if defined(__HIP_DEVICE_COMPILE__)
ASM_HD uint32_t asm_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
ASM_HD uint32_t asm_udot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
// x as it is, in a register of its own: keeps the compiler from folding a merge into each of its users
ASM_HD uint32_t asm_pin(uint32_t x) {
    asm("" : "+v"(x));
    return x;
}
#else
ASM_HD uint32_t asm_pin(uint32_t x) { return x; }
// v_perm_b32: byte q of the result is byte sel.byte[q] of { hi : lo } for selectors 0-7; 8-11 spread the sign of byte 1, 3, 5, 7;
// 12 gives 0x00 and anything above 0xFF
ASM_HD uint32_t asm_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    const u64 in = ((u64)hi << 32) | (u64)lo;
    uint32_t r = 0u;
    for (int q = 0; q < 4; q++) {
        const uint32_t s = (sel >> (8 * q)) & 0xffu;
        uint32_t b;
        if (s >= 13u) b = 0xffu;
        else if (s == 12u) b = 0x00u;
        else if (s >= 8u) b = ((in >> (16 * (s - 8u) + 15)) & 1ull) ? 0xffu : 0x00u;
        else b = (uint32_t)(in >> (8 * s)) & 0xffu;
        r |= b << (8 * q);
    }
    return r;
}
// v_dot4_u32_u8 without clamp: the four byte products summed onto c
ASM_HD uint32_t asm_udot4(uint32_t a, uint32_t b, uint32_t c) {
    for (int q = 0; q < 4; q++) c += ((a >> (8 * q)) & 0xffu) * ((b >> (8 * q)) & 0xffu);
    return c;
}
#endif

ASM_HD uint32_t swar_zero_bytes(uint32_t t) { /* bit 7 of each byte set iff that byte of t is zero (exact) */
    return ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu);
}

// dwords of ONE plane array for a range of `nv` vectors: two vectors per dword, plus the dword the funnel shift of a
// string's last output word reads past the range
ASM_HD int pack_plane_dwords(int nv) { return ((nv + 1) >> 1) + 1; }

// Four characters -> per byte, the 2-bit code in bits 0-1 (A=00 C=01 G=10 T=11) and, in bits 3-7, what the byte differs by from the
// one byte of its class that the code is right for.  The low three bits of a byte pick its class (a v_perm_b32 look-up in eight
// bytes); the table holds that class's byte with its code XOR-ed into the low bits, so one XOR with the character leaves the code
// and the difference side by side:
//   class 1 'A' 0x41 code 0    class 3 'C' 0x43 code 1    class 7 'G' 0x47 code 2    class 4 'T' 0x54 code 3
//   classes 0, 2, 5, 6 hold no base: code 0 for NUL, 0x02, 0x05 and 'N' (so that padding and N take the fast branch too)
// A byte whose bits 3-7 come out non-zero is not its class's byte, hence no base: code 00 (pack_keep).
#define PACK_TABLE_LO 0x42024100u /* classes 0-3: 0x00, 'A', 0x02, 'C' ^ 1 */
#define PACK_TABLE_HI 0x454E0557u /* classes 4-7: 'T' ^ 3, 0x05, 'N', 'G' ^ 2 */
ASM_HD uint32_t pack_codes(uint32_t ch) { return asm_perm(PACK_TABLE_HI, PACK_TABLE_LO, ch & 0x07070707u) ^ ch; }
// 0x03 in every byte of y = pack_codes(ch) whose character is its class's byte, 0x00 in the others
ASM_HD uint32_t pack_keep(uint32_t y) {
    const uint32_t ok = swar_zero_bytes(y & 0xf8f8f8f8u);
    return (ok >> 7) | (ok >> 6);
}

// 16 characters -> their 16 bits of plane 0 (C|T) and plane 1 (G|T); codes A=00 C=01 G=10 T=11, any other byte 00.
ASM_HD void pack_vec(const uint4 q, uint32_t& p0, uint32_t& p1) {
    uint32_t y0 = pack_codes(q.x), y1 = pack_codes(q.y), y2 = pack_codes(q.z), y3 = pack_codes(q.w);
    if (((y0 | y1 | y2 | y3) & 0xf8f8f8f8u) != 0u) { /* rare: a byte that is neither a base nor NUL / 'N' */
        y0 &= pack_keep(y0), y1 &= pack_keep(y1), y2 &= pack_keep(y2), y3 &= pack_keep(y3);
    }
    // two dwords' codes in one: character k at bits 0-1 of byte k, character 4 + k at bits 4-5.  v_dot4_u32_u8 with weights 1, 2, 4, 8
    // then gathers one plane's eight bits at once (the plane-1 flags sit at bit 1 resp. 5: that sum comes out doubled)
    // (pinned: one v_lshl_or_b32 and two v_and_b32 per merge; left alone the compiler shifts and folds the OR into four v_bitop3_b32)
    const uint32_t lo = asm_pin(y0 | (y1 << 4)), hi = asm_pin(y2 | (y3 << 4));
    const uint32_t lo0 = asm_udot4(lo & 0x11111111u, 0x08040201u, 0u), hi0 = asm_udot4(hi & 0x11111111u, 0x08040201u, 0u);
    const uint32_t lo1 = asm_udot4(lo & 0x22222222u, 0x08040201u, 0u), hi1 = asm_udot4(hi & 0x22222222u, 0x08040201u, 0u);
    p0 = lo0 | (hi0 << 8);
    p1 = (lo1 | (hi1 << 8)) >> 1;
}

// The cut: one string (byte offset `off` into the converted range, `len` characters) out of the plane arrays P0 / P1, granule by
// granule.  PackCut holds the plane dwords under the current output word.
struct PackCut {
    int i;       /* first plane dword of the string */
    uint32_t sh; /* bit of that dword the string starts at */
    uint32_t c0, c1;
};
ASM_HD PackCut pack_cut_begin(const uint32_t* P0, const uint32_t* P1, uint32_t off, int len) {
    PackCut c;
    c.i = (int)(off >> 5), c.sh = off & 31u, c.c0 = 0u, c.c1 = 0u;
    if (len > 0) c.c0 = P0[c.i], c.c1 = P1[c.i];
    return c;
}
// granule g (positions [128g, 128g + 128)) of both planes; granules are taken in order
ASM_HD void pack_cut_granule(const uint32_t* P0, const uint32_t* P1, PackCut& c, int len, int g, uint4& v0, uint4& v1) {
    uint32_t q0[4] = {0u, 0u, 0u, 0u}, q1[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int k = 4 * g + w;
        if (32 * k < len) {
            const uint32_t n0 = P0[c.i + k + 1], n1 = P1[c.i + k + 1];
            // characters beyond the string's end (the next pair's bytes) are dropped once per 32 positions; the mask by a shift
            // right (v_lshrrev_b32 is a VOP2 operation, a shift left is priced as VOP3)
            const int keep = len - 32 * k; /* > 0 */
            const uint32_t km = keep >= 32 ? ~0u : (~0u >> ((32 - keep) & 31));
            q0[w] = asm_alignbit(n0, c.c0, c.sh) & km;
            q1[w] = asm_alignbit(n1, c.c1, c.sh) & km;
            c.c0 = n0, c.c1 = n1;
        }
    }
    v0 = make_uint4(q0[0], q0[1], q0[2], q0[3]);
    v1 = make_uint4(q1[0], q1[1], q1[2], q1[3]);
}
