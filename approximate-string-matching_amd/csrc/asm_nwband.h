// NW for unit penalties (x = o = e = 1), BANDED: the Myers/Hyyro bit-parallel recurrence of nw_unit_full (asm_kernels.h)
// restricted to a W-row window that slides down the main diagonal one row per column.  With C = W/2 the window of column j
// holds rows j-C+1 .. j+C, that is the diagonals (row - column) -(C-1) .. C; for the first C columns it sits on rows 1..W, a
// superset.  Cells outside the band are taken as "one more than their in-band neighbour" (vertical delta +1 for the row
// entering at the bottom, horizontal delta +1 for the row leaving at the top), which makes every in-band value an upper
// bound of the true DP value, and exact whenever an optimal path stays inside the band.
//
// When a banded result is proven exact.  A path from (0,0) to (m,n) of cost r makes v vertical and h horizontal moves with
// v + h <= r and v - h = m - n, so it never leaves diagonal 0 by more than (r + (m-n))/2 downwards or (r - (m-n))/2 upwards.
// The banded value r' is never below the distance d.  Hence r' <= 2(C-1) - |n-m| puts every optimal path (cost d <= r')
// within C-1 diagonals on either side, inside the band, and r' = d.  W = 16 proves results up to 14 - |n-m|, W = 32 up to
// 30 - |n-m|, W = 64 up to 62 - |n-m|.  Any other outcome (a larger r', or row m outside the last window) is -1: the caller
// tries the next wider window and at last the full-height sweep.
// Rows beyond the read's end hold arbitrary plane bits: they only feed cells below row m, never D[m][n].
//
// nw_band<ND, W>: one pair per thread, W = 32 (one dword per vector) or 64.  nw_band2x16<ND>: TWO pairs per thread, each in
// a 16-row window, side by side in the halves of one dword.
//
// The header compiles for the host as well (NWB_HD): host/nw_host_check.cpp runs the very same sweeps on the CPU against the
// oracle (tests/test_nw_pair2_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NWB_HD __device__ __forceinline__
#else
#define NWB_HD inline
#endif

typedef unsigned long long nwb_u64;

// ---- small primitives (device: one instruction each; host: the plain meaning) ------------------------------------------
#if defined(__HIPCC__)
NWB_HD int nwb_popc(uint32_t x) { return __popc(x); }
NWB_HD int nwb_popc64(nwb_u64 x) { return __popcll(x); }
NWB_HD uint32_t nwb_alignbit(uint32_t hi, uint32_t lo, uint32_t s) { return __builtin_amdgcn_alignbit(hi, lo, s); }
NWB_HD uint32_t nwb_sbfe1(uint32_t b, int r) { return (uint32_t)__builtin_amdgcn_sbfe((int)b, r, 1); }
// packed 16-bit halves of a dword (v_pk_add_u16, v_pk_lshlrev_b16, v_pk_lshrrev_b16, v_pk_ashrrev_i16): nothing crosses
// from bit 15 into bit 16 or back.  Shift counts are 0..15.
typedef unsigned short nwb_u16x2 __attribute__((ext_vector_type(2)));
typedef short nwb_i16x2 __attribute__((ext_vector_type(2)));
NWB_HD uint32_t nwb_pk_add(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(nwb_u16x2, a) + __builtin_bit_cast(nwb_u16x2, b));
}
NWB_HD uint32_t nwb_pk_shl(uint32_t a, int s) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(nwb_u16x2, a) << (nwb_u16x2)((unsigned short)s));
}
NWB_HD uint32_t nwb_pk_shr(uint32_t a, int s) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(nwb_u16x2, a) >> (nwb_u16x2)((unsigned short)s));
}
NWB_HD uint32_t nwb_pk_sar(uint32_t a, int s) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(nwb_i16x2, a) >> (nwb_i16x2)((short)s));
}
// One v_bitop3_b32 with the truth table TT: bit (4a + 2b + c) of TT is the result for the input bits a, b, c.  Named, not
// left to the compiler: two-input operations next to it stay the two-input VOP2 forms, which issue in half the cycles of
// any VOP3 one (docs/design/kernels.md, the opcode prices).
template <int TT>
NWB_HD uint32_t nwb_bitop3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
// x << 1 as v_add_u32 x, x (the compiler writes v_lshlrev_b32, which issues at half the rate of the add)
NWB_HD uint32_t nwb_dbl(uint32_t x) {
    uint32_t r;
    asm("v_add_u32 %0, %1, %1" : "=v"(r) : "v"(x));
    return r;
}
NWB_HD uint32_t nwb_brev(uint32_t x) { return __builtin_bitreverse32(x); }
#else
NWB_HD int nwb_popc(uint32_t x) { return __builtin_popcount(x); }
NWB_HD int nwb_popc64(nwb_u64 x) { return __builtin_popcountll(x); }
NWB_HD uint32_t nwb_alignbit(uint32_t hi, uint32_t lo, uint32_t s) {
    return (uint32_t)((((nwb_u64)hi << 32) | (nwb_u64)lo) >> (s & 31u));
}
NWB_HD uint32_t nwb_sbfe1(uint32_t b, int r) { return 0u - ((b >> r) & 1u); }
NWB_HD uint32_t nwb_pk_add(uint32_t a, uint32_t b) {
    return ((a & 0x7FFF7FFFu) + (b & 0x7FFF7FFFu)) ^ ((a ^ b) & 0x80008000u);
}
NWB_HD uint32_t nwb_pk_shl(uint32_t a, int s) { return (a << s) & (0x00010001u * ((0xFFFFu << s) & 0xFFFFu)); }
NWB_HD uint32_t nwb_pk_shr(uint32_t a, int s) { return (a >> s) & (0x00010001u * (0xFFFFu >> s)); }
NWB_HD uint32_t nwb_pk_sar(uint32_t a, int s) {
    const uint32_t lo = (uint32_t)((int32_t)(int16_t)(a & 0xFFFFu) >> s) & 0xFFFFu;
    const uint32_t hi = (uint32_t)((int32_t)(int16_t)(a >> 16) >> s) & 0xFFFFu;
    return lo | (hi << 16);
}
template <int TT>
NWB_HD uint32_t nwb_bitop3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0u;
    for (int i = 0; i < 8; i++)
        if ((TT >> i) & 1) r |= ((i & 4) ? a : ~a) & ((i & 2) ? b : ~b) & ((i & 1) ? c : ~c);
    return r;
}
NWB_HD uint32_t nwb_dbl(uint32_t x) { return x + x; }
NWB_HD uint32_t nwb_brev(uint32_t x) {
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
}
#endif
// a truth table is written as the expression itself over these three
constexpr int NWB_A = 0xF0, NWB_B = 0xCC, NWB_C = 0xAA;

// largest banded result that is proven exact in a window of 2C rows (see above)
NWB_HD int nwb_band_bound(int C, int m, int nn) { return 2 * (C - 1) - (nn > m ? nn - m : m - nn); }

template <int W>
struct BandWord;
template <>
struct BandWord<32> {
    typedef uint32_t T;
};
template <>
struct BandWord<64> {
    typedef nwb_u64 T;
};

struct NoColumnSink {
    static constexpr bool kNeedsColumns = false;
    template <typename WT>
    NWB_HD void operator()(int, WT, WT) const {}
};

// `sink(j, VP, VN)` sees the vertical delta vectors of every finished column j (1-based, in that column's window
// coordinates); the traceback of asm_cover.h stores them.
// all-ones / all-zeros word from bit r of the text block (one v_bfe_i32 for the 32-bit window)
template <int W>
NWB_HD typename BandWord<W>::T band_text_bit(typename BandWord<W>::T b, int r);
template <>
NWB_HD uint32_t band_text_bit<32>(uint32_t b, int r) {
    return nwb_sbfe1(b, r);
}
template <>
NWB_HD nwb_u64 band_text_bit<64>(nwb_u64 b, int r) {
    return 0ull - ((b >> r) & 1ull);
}

template <int ND, int W, typename Sink = NoColumnSink> /* ND = plane dwords per string (4 * w4); A arrays carry two zero dwords of padding */
NWB_HD int nw_band(const uint32_t (&A0)[ND + 2], const uint32_t (&A1)[ND + 2], const uint32_t (&B0)[ND],
                    const uint32_t (&B1)[ND], int m, int nn, const Sink& sink = Sink()) {
    typedef typename BandWord<W>::T WT;
    constexpr int C = W / 2;          /* window top row of column j is max(1, j - C + 1) */
    constexpr int NBLK = ND * 32 / W; /* W-column blocks */
    constexpr WT TOP = (WT)1 << (W - 1);
#define BLK(ARR, q) (W == 32 ? (WT)ARR[(q)] : (WT)((nwb_u64)ARR[2 * (q)] | ((nwb_u64)ARR[2 * (q) + 1] << 32)))
    WT VP = ~(WT)0, VN = 0; /* column 0: D[i][0] = i */
    int S = W;              /* D[bottom row of the window][column] */
    WT lo0 = BLK(A0, 0), lo1 = BLK(A1, 0), hi0 = 0, hi1 = 0;

#define NW_BAND_COLUMN(SLIDE, BW0, BW1, R)                                                           \
    {                                                                                                 \
        if (SLIDE) {                                                                                  \
            lo0 = (lo0 >> 1) | (hi0 << (W - 1)), hi0 >>= 1;                                           \
            lo1 = (lo1 >> 1) | (hi1 << (W - 1)), hi1 >>= 1;                                           \
            VP = (VP >> 1) | TOP, VN >>= 1;                                                           \
        }                                                                                             \
        const WT T0 = (WT)0 - (((BW0) >> (R)) & (WT)1);                                               \
        const WT T1 = (WT)0 - (((BW1) >> (R)) & (WT)1);                                               \
        const WT Eq = ~((lo0 ^ T0) | (lo1 ^ T1));                                                     \
        const WT D0 = ((((Eq & VP) + VP) ^ VP) | Eq) | VN;                                            \
        const WT HP = VN | ~(D0 | VP);                                                                \
        const WT HN = VP & D0;                                                                        \
        if (SLIDE)                                                                                    \
            S += 1 - (int)(D0 >> (W - 1));                                                            \
        else                                                                                          \
            S += (int)(HP >> (W - 1)) - (int)(HN >> (W - 1));                                         \
        const WT X = (HP << 1) | (WT)1;                                                               \
        VP = (HN << 1) | ~(D0 | X);                                                                   \
        VN = D0 & X;                                                                                  \
    }

    // columns 1..C: the window still sits on rows 1..W
    {
        const WT b0 = BLK(B0, 0), b1 = BLK(B1, 0);
        const int c1 = nn < C ? nn : C;
        for (int r = 0; r < c1; r++) {
            NW_BAND_COLUMN(false, b0, b1, r)
            sink(r + 1, VP, VN);
        }
    }
    // columns C+1..n: slide one row per column; the reservoir's upper word is refilled every W slides.
    if (Sink::kNeedsColumns) {
        // plain form: every column's (VP, VN) in that column's own window coordinates, handed to the sink
#pragma unroll
        for (int bq = 0; bq < NBLK; bq++) {
            const WT b0 = BLK(B0, bq), b1 = BLK(B1, bq);
            const int r0 = bq == 0 ? C : 0;
            int rend = nn - W * bq;
            rend = rend > W ? W : rend;
            for (int r = r0; r < rend; r++) {
                if (r == C) hi0 = BLK(A0, bq + 1), hi1 = BLK(A1, bq + 1); /* wave-uniform */
                NW_BAND_COLUMN(true, b0, b1, r)
                sink(W * bq + r + 1, VP, VN);
            }
        }
    } else if (nn > C) {
        // Fused form (penalty only).  Algebraically the same recurrence: instead of producing a column's vertical deltas
        // in its own window and shifting them for the next column, produce them directly in the NEXT column's window:
        //   VPin' = HN | ~((D0 >> 1) | HP) | TOP ,  VNin' = HP & (D0 >> 1)
        // (the "+1 for the row entering at the bottom" is the TOP bit; the "+1 above the window" is the zero shifted
        // into D0 >> 1).  Three instructions fewer per column.  The bottom-row diagonal deltas are shifted into an
        // accumulator and counted once per block instead of being added column by column.
        WT VPin = (VP >> 1) | TOP, VNin = VN >> 1;
#pragma unroll
        for (int bq = 0; bq < NBLK; bq++) {
            const WT b0 = BLK(B0, bq), b1 = BLK(B1, bq);
            const int r0 = bq == 0 ? C : 0;
            int rend = nn - W * bq;
            rend = rend > W ? W : rend;
            WT acc = 0;
            // the block's columns in two runs: the pattern window of column 32*bq + r starts at row 32*bq + r - (C-1), i.e.
            // in pattern word bq-1 for r < C-1 and in word bq from there on
#pragma unroll
            for (int half = 0; half < 2; half++) {
                constexpr int CB = W == 32 ? C - 1 : C;
                const int ra = half == 0 ? r0 : (r0 > CB ? r0 : CB);
                const int rb = half == 0 ? (rend < CB ? rend : CB) : rend;
                if (W != 32 && half == 1) hi0 = BLK(A0, bq + 1), hi1 = BLK(A1, bq + 1);
                // W = 32: the window is cut straight out of two adjacent pattern words with one v_alignbit_b32 (wave-uniform
                // shift), no sliding state to update
                const uint32_t p0l = W == 32 ? (half == 0 ? (bq > 0 ? A0[bq > 0 ? bq - 1 : 0] : 0u) : A0[bq]) : 0u;
                const uint32_t p0h = W == 32 ? (half == 0 ? A0[bq] : A0[bq + 1]) : 0u;
                const uint32_t p1l = W == 32 ? (half == 0 ? (bq > 0 ? A1[bq > 0 ? bq - 1 : 0] : 0u) : A1[bq]) : 0u;
                const uint32_t p1h = W == 32 ? (half == 0 ? A1[bq] : A1[bq + 1]) : 0u;
                const int shb = half == 0 ? W - CB : -CB;
                for (int r = ra; r < rb; r++) {
                    if (W == 32) {
                        lo0 = (WT)nwb_alignbit(p0h, p0l, (uint32_t)(r + shb));
                        lo1 = (WT)nwb_alignbit(p1h, p1l, (uint32_t)(r + shb));
                    } else {
                        lo0 = (lo0 >> 1) | (hi0 << (W - 1)), hi0 >>= 1;
                        lo1 = (lo1 >> 1) | (hi1 << (W - 1)), hi1 >>= 1;
                    }
                    const WT T0 = band_text_bit<W>(b0, r), T1 = band_text_bit<W>(b1, r);
                    const WT Eq = ~((lo0 ^ T0) | (lo1 ^ T1));
                    const WT D0 = ((((Eq & VPin) + VPin) ^ VPin) | Eq) | VNin;
                    const WT HP = VNin | ~(D0 | VPin);
                    const WT HN = VPin & D0;
                    acc = (acc << 1) | (D0 >> (W - 1));
                    const WT D0s = D0 >> 1;
                    VPin = HN | ~(D0s | HP) | TOP;
                    VNin = HP & D0s;
                }
            }
            if (rend > r0) S += (rend - r0) - (W == 32 ? nwb_popc((uint32_t)acc) : nwb_popc64((nwb_u64)acc));
        }
        // back to the last column's own window: VP = VPin << 1 (its bit 0 is always 0); VN = VNin << 1 | D0[0] — only
        // the bits above row m are needed below, and bit 0 never is
        VP = VPin << 1;
        VN = VNin << 1;
    }
#undef NW_BAND_COLUMN
#undef BLK
    const int top = nn > C - 1 ? nn - (C - 1) : 1; /* window top row of the last column */
    const int bstar = m - top;                     /* bit of row m */
    if (bstar < 0 || bstar > W - 1) return -1;
    const WT above = bstar == W - 1 ? (WT)0 : (~(WT)0 << (bstar + 1));
    const int up = W == 32 ? nwb_popc((uint32_t)(VP & above)) : nwb_popc64((nwb_u64)(VP & above));
    const int dn = W == 32 ? nwb_popc((uint32_t)(VN & above)) : nwb_popc64((nwb_u64)(VN & above));
    const int result = S - up + dn;
    return result <= nwb_band_bound(C, m, nn) ? result : -1;
}


// --------------------------------------------------------------------------------------------------------
// Two pairs per thread: pair P's 16-row window in bits 0-15 of every vector, pair Q's in bits 16-31, the fused penalty-only
// form of nw_band<> above with C = 8.  Both pairs stand at the same column, so every shift count is wave-uniform:
//   * the add (Eq & VPin) + VPin is the packed 16-bit add and D0 >> 1 the packed shift: no carry and no bit passes from
//     one pair's half into the other's.  Bit 15 of each half of VPin is always 1 (the row entering at the bottom) and of VNin
//     always 0; that makes HP's top bits 0, and with the zero that the packed D0 >> 1 shifts in, HN | ~((D0 >> 1) | HP) has
//     its top bits set without an OR of its own;
//   * strings are consumed in 16-bit chunks, chunk k of P below chunk k of Q (nwb_chunk2).  The pattern windows of a run of
//     columns start in one chunk k (chunk bq-1 for the first 7 columns of block bq, chunk bq from there on, as in
//     nw_band<>): column s of the run wants bits s..s+15 of P's string from chunk k on in the low half and the same bits of
//     Q's in the high half.  Seen as 64 bits, that is bits s..s+31 of { Q's chunk k+1 : Q's chunk k : P's chunks k+1, k }
//     with P's bits up to 16+s and Q's from there on: one v_bfi_b32 with a constant mask picks the low dword out of P's 32
//     bits (nwb_run32) and the packed chunk, one v_alignbit_b32 cuts the window;
//   * the text chunk is packed the other way round (Q below P) and bit-reversed, so that column r's bits stand at bits 15
//     and 31 after r doublings; one packed arithmetic shift right by 15 makes them all-ones / all-zeros halves.  What the
//     doubling carries from the low half into the high one stays below the bit that is read;
//   * the bottom-row diagonal deltas of a block are collected in `acc`, P's entering at bit 15 and Q's at bit 31 and moving
//     down one bit per column with a plain 32-bit shift: within the 16 columns of a block Q's bits stay above bit 15.  They
//     are counted once per block.
// Which opcode does what is chosen by price (docs/design/kernels.md): 13 VOP3 and 8 VOP2 instructions per column of both pairs.
// The two pairs have their own m and n.  Columns run to max(nP, nQ).  Blocks that lie wholly inside both texts take the plain
// column; from the block that holds min(nP, nQ) on, a column keeps the state of a half whose text has ended (FREEZE), so
// that each half's (VPin, VNin, S) is left as of its own last column.  Each half is then read out with its own m and n as in
// nw_band<>: -1 when row m is not in its last window or the result is above 14 - |n-m|.
// --------------------------------------------------------------------------------------------------------
template <int ND, int N> /* the arrays may be longer than the string's ND dwords (nw_band<>'s padded read planes) */
NWB_HD uint32_t nwb_chunk2(const uint32_t (&P)[N], const uint32_t (&Q)[N], int k) {
    if (k < 0 || k >= 2 * ND) return 0u;
    const uint32_t p = P[k >> 1], q = Q[k >> 1];
    return (k & 1) ? (p >> 16) | (q & 0xFFFF0000u) : (p & 0xFFFFu) | (q << 16);
}
// chunks k and k+1 of one string as a dword (chunks outside the string's ND dwords are zero; k >= -1)
template <int ND, int N>
NWB_HD uint32_t nwb_run32(const uint32_t (&P)[N], int k) {
    const int d = k < 0 ? -1 : k >> 1; /* the dword that holds chunk k in its low (k even) or high half */
    const uint32_t lo = d >= 0 && d < ND ? P[d >= 0 && d < ND ? d : 0] : 0u;
    if (!(k & 1)) return lo;
    const uint32_t hi = d + 1 >= 0 && d + 1 < ND ? P[d + 1 >= 0 && d + 1 < ND ? d + 1 : 0] : 0u;
    return nwb_alignbit(hi, lo, 16);
}
// a dword whose low 16 bits are chunk k of the string (zero outside it); the upper bits are arbitrary
template <int ND, int N>
NWB_HD uint32_t nwb_low16(const uint32_t (&P)[N], int k) {
    if (k < 0 || k >= 2 * ND) return 0u;
    return (k & 1) ? P[k >> 1] >> 16 : P[k >> 1];
}
struct NoBlockSink {
    NWB_HD void operator()(int, uint32_t, uint32_t, int, int) const {}
};

// one half's result from its final vectors (in its last column's own window), as the tail of nw_band<>
NWB_HD int nwb_band16_result(uint32_t vp, uint32_t vn, int S, int m, int nn) {
    constexpr int W = 16, C = 8;
    const int top = nn > C - 1 ? nn - (C - 1) : 1;
    const int bstar = m - top;
    if (bstar < 0 || bstar > W - 1) return -1;
    const uint32_t above = (0xFFFFu << (bstar + 1)) & 0xFFFFu;
    const int result = S - nwb_popc(vp & above) + nwb_popc(vn & above);
    return result <= nwb_band_bound(C, m, nn) ? result : -1;
}

// `block_sink(bq, VPin, VNin, Sp, Sq)` sees the state after every 16-column block (the host check compares it)
template <int ND, int NA, typename BlockSink = NoBlockSink> /* plane dwords per string, as nw_band<>; A0/A1 the read's planes (NA >= ND
                             dwords: the padding of nw_band<> is accepted and not read), B0/B1 the reference's */
NWB_HD void nw_band2x16(const uint32_t (&A0p)[NA], const uint32_t (&A1p)[NA], const uint32_t (&B0p)[ND],
                        const uint32_t (&B1p)[ND], int mp, int np, const uint32_t (&A0q)[NA], const uint32_t (&A1q)[NA],
                        const uint32_t (&B0q)[ND], const uint32_t (&B1q)[ND], int mq, int nq, int& result_p, int& result_q,
                        const BlockSink& block_sink = BlockSink()) {
    constexpr int W = 16, C = 8, CB = C - 1;
    constexpr int NBLK = 2 * ND; /* 16-column blocks */
    constexpr uint32_t TOP = 0x80008000u, ONE = 0x00010001u, LOW = 0x0000FFFFu, HIGH = 0xFFFF0000u;
    const int nmin = np < nq ? np : nq, nmax = np < nq ? nq : np;
    uint32_t VP = ~0u, VN = 0u; /* column 0: D[i][0] = i */
    int Sp = W, Sq = W;         /* D[bottom row of the window][column], per half */

    // columns 1..C: the windows still sit on rows 1..16 (plain form; a half whose text is shorter keeps its state)
    {
        const uint32_t lo0 = nwb_chunk2<ND>(A0p, A0q, 0), lo1 = nwb_chunk2<ND>(A1p, A1q, 0);
        const uint32_t b0 = nwb_chunk2<ND>(B0p, B0q, 0), b1 = nwb_chunk2<ND>(B1p, B1q, 0);
        uint32_t hp = 0u, hn = 0u; /* bottom-row horizontal deltas, counted after the loop */
        const int c1 = nmax < C ? nmax : C;
        for (int r = 0; r < c1; r++) {
            const uint32_t L = (r < np ? LOW : 0u) | (r < nq ? HIGH : 0u);
            const uint32_t T0 = nwb_pk_sar(nwb_pk_shl(b0, 15 - r), 15), T1 = nwb_pk_sar(nwb_pk_shl(b1, 15 - r), 15);
            const uint32_t Eq = ~((lo0 ^ T0) | (lo1 ^ T1));
            const uint32_t D0 = ((nwb_pk_add(Eq & VP, VP) ^ VP) | Eq) | VN;
            const uint32_t HP = VN | ~(D0 | VP);
            const uint32_t HN = VP & D0;
            hp = nwb_pk_shr(hp, 1) | (HP & TOP & L);
            hn = nwb_pk_shr(hn, 1) | (HN & TOP & L);
            const uint32_t X = nwb_pk_shl(HP, 1) | ONE;
            VP = ((nwb_pk_shl(HN, 1) | ~(D0 | X)) & L) | (VP & ~L);
            VN = ((D0 & X) & L) | (VN & ~L);
        }
        Sp += nwb_popc(hp & LOW) - nwb_popc(hn & LOW);
        Sq += nwb_popc(hp >> 16) - nwb_popc(hn >> 16);
    }

    // columns C+1..max(nP, nQ), fused form: the vectors are kept in the NEXT column's window (see nw_band<>).  Bit 0 of VP is
    // lost on the way there and back; it is never above row m.
    uint32_t VPin = nwb_pk_shr(VP, 1) | TOP, VNin = nwb_pk_shr(VN, 1);
    constexpr int TT_EQ = ~((NWB_A ^ NWB_B) | NWB_C) & 0xFF;  /* ~((w0 ^ T0) | x1) */
    constexpr int TT_D0 = ((NWB_A ^ NWB_B) | NWB_C) & 0xFF;   /* (sum ^ VPin) | Eq */
    constexpr int TT_ORN = (NWB_A | ~(NWB_B | NWB_C)) & 0xFF; /* a | ~(b | c) */
    constexpr int TT_ACC = ((NWB_A & NWB_B) | NWB_C) & 0xFF;  /* (D0 & TOP) | acc */
    constexpr int TT_SEL = ((NWB_A & NWB_B) | (~NWB_A & NWB_C)) & 0xFF; /* a ? b : c */
    // the columns RA..RB-1 of block bq, whose windows start in pattern chunk K: column r wants bits s..s+15, s = r + SHB
#define NW2_COLUMNS(FREEZE, RA, RB, K, SHB)                                                                      \
    {                                                                                                             \
        const uint32_t rp0 = nwb_run32<ND>(A0p, (K)), rp1 = nwb_run32<ND>(A1p, (K));                              \
        const uint32_t u0 = nwb_chunk2<ND>(A0p, A0q, (K)), u1 = nwb_chunk2<ND>(A1p, A1q, (K));                    \
        const uint32_t hq0 = nwb_low16<ND>(A0q, (K) + 1), hq1 = nwb_low16<ND>(A1q, (K) + 1);                      \
        for (int r = (RA); r < (RB); r++) {                                                                       \
            const int s = r + (SHB);                        /* 0..15 */                                           \
            const uint32_t keep = (0x10000u << s) - 1u;     /* P's bits of the 64-bit run's low dword */           \
            const uint32_t w0 = nwb_alignbit(hq0, nwb_bitop3<TT_SEL>(keep, rp0, u0), (uint32_t)s);                \
            const uint32_t w1 = nwb_alignbit(hq1, nwb_bitop3<TT_SEL>(keep, rp1, u1), (uint32_t)s);                \
            const uint32_t T0 = nwb_pk_sar(y0, 15), T1 = nwb_pk_sar(y1, 15);                                      \
            y0 = nwb_dbl(y0), y1 = nwb_dbl(y1);                                                                   \
            const uint32_t x1 = w1 ^ T1;                                                                          \
            const uint32_t Eq = nwb_bitop3<TT_EQ>(w0, T0, x1);                                                    \
            const uint32_t sum = nwb_pk_add(Eq & VPin, VPin);                                                     \
            const uint32_t D0a = nwb_bitop3<TT_D0>(sum, VPin, Eq); /* D0 but for VNin, which HP and HN do not need: */ \
            const uint32_t HP = nwb_bitop3<TT_ORN>(VNin, D0a, VPin); /* VNin | ~(D0 | VPin) */                     \
            const uint32_t HN = VPin & D0a;                          /* VPin & VNin == 0 */                        \
            const uint32_t D0s = nwb_pk_shr(D0a | VNin, 1);                                                       \
            const uint32_t VPn = nwb_bitop3<TT_ORN>(HN, D0s, HP); /* both top bits come out set, see above */      \
            const uint32_t VNn = HP & D0s;                                                                        \
            if (FREEZE) {                                                                                         \
                const int col = W * bq + r;                                                                       \
                const uint32_t L = (col < np ? LOW : 0u) | (col < nq ? HIGH : 0u);                                \
                acc = nwb_bitop3<TT_ACC>(D0a, TOP & L, acc >> 1); /* VNin's top bits are 0: D0a's are D0's */      \
                VPin = (VPn & L) | (VPin & ~L);                                                                   \
                VNin = (VNn & L) | (VNin & ~L);                                                                   \
            } else {                                                                                              \
                acc = nwb_bitop3<TT_ACC>(D0a, TOP, acc >> 1);                                                     \
                VPin = VPn;                                                                                       \
                VNin = VNn;                                                                                       \
            }                                                                                                     \
        }                                                                                                         \
    }
    if (nmax > C) {
#pragma unroll
        for (int bq = 0; bq < NBLK; bq++) {
            const int r0 = bq == 0 ? C : 0;
            int rend = nmax - W * bq;
            rend = rend > W ? W : rend;
            if (rend <= r0) continue;
            // the text chunk, Q's below P's and bit-reversed: column r's bits are bits 31 - r (P) and 15 - r (Q)
            uint32_t y0 = nwb_brev(nwb_chunk2<ND>(B0q, B0p, bq)) << r0;
            uint32_t y1 = nwb_brev(nwb_chunk2<ND>(B1q, B1p, bq)) << r0;
            uint32_t acc = 0u;
            if (W * bq + W <= nmin) { /* the whole block lies inside both texts */
                if (r0 < CB) NW2_COLUMNS(false, r0, CB, bq - 1, W - CB)
                NW2_COLUMNS(false, (r0 > CB ? r0 : CB), W, bq, -CB)
            } else {
                if (r0 < CB) NW2_COLUMNS(true, r0, (rend < CB ? rend : CB), bq - 1, W - CB)
                NW2_COLUMNS(true, (r0 > CB ? r0 : CB), rend, bq, -CB)
            }
            // S += 1 - (the diagonal delta's bit) for every column of this block that the half's text has
            int cp = np - W * bq, cq = nq - W * bq;
            cp = (cp > W ? W : (cp < r0 ? r0 : cp)) - r0;
            cq = (cq > W ? W : (cq < r0 ? r0 : cq)) - r0;
            Sp += cp - nwb_popc(acc & LOW);
            Sq += cq - nwb_popc(acc >> 16);
            block_sink(bq, VPin, VNin, Sp, Sq);
        }
    }
#undef NW2_COLUMNS
    // back to the last column's own window, as nw_band<>
    const uint32_t VPf = nwb_pk_shl(VPin, 1), VNf = nwb_pk_shl(VNin, 1);
    result_p = nwb_band16_result(VPf & LOW, VNf & LOW, Sp, mp, np);
    result_q = nwb_band16_result(VPf >> 16, VNf >> 16, Sq, mq, nq);
}
