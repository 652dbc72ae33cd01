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
#endif

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
//   * the add (Eq & VPin) + VPin is the packed 16-bit add, D0 >> 1 and the other shifts are packed shifts: no carry and no
//     bit passes from one pair's half into the other's; TOP is 0x80008000;
//   * strings are consumed in 16-bit chunks, chunk k of P below chunk k of Q (nwb_chunk2).  A column's pattern window is cut
//     out of two adjacent chunks U, V of each plane as (U >> s) | ((V << 1) << (15 - s)), in two runs per 16-column block as
//     in nw_band<>: the window starts in chunk bq-1 for the first 7 columns of block bq and in chunk bq from there on;
//   * the text character's bits become all-ones / all-zeros halves by a shift left by 15 - r and an arithmetic shift right
//     by 15;
//   * the bottom-row diagonal deltas of a block are collected per half in `acc` and counted once per block.
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

template <int ND, int NA> /* plane dwords per string, as nw_band<>; A0/A1 the read's planes (NA >= ND dwords: the padding of
                             nw_band<> is accepted and not read), B0/B1 the reference's */
NWB_HD void nw_band2x16(const uint32_t (&A0p)[NA], const uint32_t (&A1p)[NA], const uint32_t (&B0p)[ND],
                        const uint32_t (&B1p)[ND], int mp, int np, const uint32_t (&A0q)[NA], const uint32_t (&A1q)[NA],
                        const uint32_t (&B0q)[ND], const uint32_t (&B1q)[ND], int mq, int nq, int& result_p, int& result_q) {
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
#define NW2_COLUMNS(FREEZE, RA, RB, U0, V0, U1, V1, SHB)                                                   \
    {                                                                                                       \
        const uint32_t v0s = nwb_pk_shl(V0, 1), v1s = nwb_pk_shl(V1, 1);                                    \
        for (int r = (RA); r < (RB); r++) {                                                                 \
            const int s = r + (SHB); /* 0..15 */                                                            \
            const uint32_t lo0 = nwb_pk_shr(U0, s) | nwb_pk_shl(v0s, 15 - s);                               \
            const uint32_t lo1 = nwb_pk_shr(U1, s) | nwb_pk_shl(v1s, 15 - s);                               \
            const uint32_t T0 = nwb_pk_sar(nwb_pk_shl(b0, 15 - r), 15), T1 = nwb_pk_sar(nwb_pk_shl(b1, 15 - r), 15); \
            const uint32_t Eq = ~((lo0 ^ T0) | (lo1 ^ T1));                                                 \
            const uint32_t D0 = ((nwb_pk_add(Eq & VPin, VPin) ^ VPin) | Eq) | VNin;                         \
            const uint32_t HP = VNin | ~(D0 | VPin);                                                        \
            const uint32_t HN = VPin & D0;                                                                  \
            const uint32_t D0s = nwb_pk_shr(D0, 1);                                                         \
            if (FREEZE) {                                                                                   \
                const int col = W * bq + r;                                                                 \
                const uint32_t L = (col < np ? LOW : 0u) | (col < nq ? HIGH : 0u);                          \
                acc = nwb_pk_shr(acc, 1) | (D0 & TOP & L);                                                  \
                VPin = ((HN | ~(D0s | HP) | TOP) & L) | (VPin & ~L);                                        \
                VNin = ((HP & D0s) & L) | (VNin & ~L);                                                      \
            } else {                                                                                        \
                acc = nwb_pk_shr(acc, 1) | (D0 & TOP);                                                      \
                VPin = HN | ~(D0s | HP) | TOP;                                                              \
                VNin = HP & D0s;                                                                            \
            }                                                                                               \
        }                                                                                                   \
    }
    if (nmax > C) {
#pragma unroll
        for (int bq = 0; bq < NBLK; bq++) {
            const int r0 = bq == 0 ? C : 0;
            int rend = nmax - W * bq;
            rend = rend > W ? W : rend;
            if (rend <= r0) continue;
            const uint32_t b0 = nwb_chunk2<ND>(B0p, B0q, bq), b1 = nwb_chunk2<ND>(B1p, B1q, bq);
            // pattern chunks bq-1, bq, bq+1 of both planes (zeros outside the string's dwords)
            const uint32_t a0m = nwb_chunk2<ND>(A0p, A0q, bq - 1), a0c = nwb_chunk2<ND>(A0p, A0q, bq), a0n = nwb_chunk2<ND>(A0p, A0q, bq + 1);
            const uint32_t a1m = nwb_chunk2<ND>(A1p, A1q, bq - 1), a1c = nwb_chunk2<ND>(A1p, A1q, bq), a1n = nwb_chunk2<ND>(A1p, A1q, bq + 1);
            uint32_t acc = 0u;
            if (W * bq + W <= nmin) { /* the whole block lies inside both texts */
                if (r0 < CB) NW2_COLUMNS(false, r0, CB, a0m, a0c, a1m, a1c, W - CB)
                NW2_COLUMNS(false, (r0 > CB ? r0 : CB), W, a0c, a0n, a1c, a1n, -CB)
            } else {
                if (r0 < CB) NW2_COLUMNS(true, r0, (rend < CB ? rend : CB), a0m, a0c, a1m, a1c, W - CB)
                NW2_COLUMNS(true, (r0 > CB ? r0 : CB), rend, a0c, a0n, a1c, a1n, -CB)
            }
            // S += 1 - (the diagonal delta's bit) for every column of this block that the half's text has
            int cp = np - W * bq, cq = nq - W * bq;
            cp = (cp > W ? W : (cp < r0 ? r0 : cp)) - r0;
            cq = (cq > W ? W : (cq < r0 ? r0 : cq)) - r0;
            Sp += cp - nwb_popc(acc & LOW);
            Sq += cq - nwb_popc(acc >> 16);
        }
    }
#undef NW2_COLUMNS
    // back to the last column's own window, as nw_band<>
    const uint32_t VPf = nwb_pk_shl(VPin, 1), VNf = nwb_pk_shl(VNin, 1);
    result_p = nwb_band16_result(VPf & LOW, VNf & LOW, Sp, mp, np);
    result_q = nwb_band16_result(VPf >> 16, VNf >> 16, Sq, mq, nq);
}
