// What the general-penalty kernels share: the affine Landau-Vishkin lane step (LV::run, LEAP_SIMD/LV_BAG.cpp:127-245), the
// generation rings it reads and writes, the LDS sizes of those rings, and the Gotoh column-block sweep with its traceback.
// The kernels keep their own thread shapes, lane loops and result rules (asm_kernels.h, asm_wave.h, asm_wide.h, asm_filter.h,
// asm_cover.h); docs/design/kernels.md describes both recurrences once.
//
// The header compiles for the host as well (LU_HD): host/affine_host_check.cpp drives every function here pair by pair on the CPU
// against the oracle (tests/test_affine_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "asm_leapunit.h"

#ifndef ASM_MAX_LENGTH
#define ASM_MAX_LENGTH 512 /* include/asm_mi355x.h has the same */
#endif

// ---- the LV lane step ---------------------------------------------------------------------------------------------------------
// gap(L) = o + (L-1) ext; the cost of converging from a lane `diff` diagonals off the main one (LV_BAG.cpp:220-238)
LU_HD int affine_gap(int diff, int o, int ext) { return diff ? o + (diff - 1) * ext : 0; }

struct LvStep {
    int inew, dnew, st; /* I and D of this lane and generation, and where its extension starts; -2 = never reached */
};
// One lane of generation e (LV_BAG.cpp:166-187).  e_up / e_dn: `end` of the lanes above and below at generation e - o; i_up / d_dn:
// their I and D at e - ext; own: this lane's `end` at e - x.  top / bot: 1 on and above / on and below the main lane.  All
// values unbiased, -2 = never reached.
// The reference guards each read (e >= o, e >= ext, e >= x).  A caller needs no guard of its own as long as a read that the
// reference would not make yields -2: `e_up >= 0 && ...` and `i_up >= 0` are then false exactly where `e >= o && ...` and
// `e >= ext && ...` would be, and own = -2 gives st = -2.  The ring kernels get that -2 for free — the slot of a generation
// before 0 is the slot of one not written yet (ring depth > penalty) and still holds the initial "never reached" —, so their five
// reads issue back to back instead of behind a branch and a wait each; leap_wide_kernel, whose ring is 16 deep whatever the
// penalties, passes -2 for a guarded read.
LU_HD LvStep lv_affine_step(int e_up, int i_up, int e_dn, int d_dn, int own, int top, int bot) {
    LvStep s;
    s.inew = -2, s.dnew = -2;
    if (e_up >= 0 && e_up > i_up)
        s.inew = e_up + top; /* LV_BAG.cpp:166-167 */
    else if (i_up >= 0)
        s.inew = i_up + top; /* :172-176 */
    if (e_dn >= 0 && e_dn > d_dn)
        s.dnew = e_dn + bot; /* :179-180 */
    else if (d_dn >= 0)
        s.dnew = d_dn + bot; /* :181-182 */
    s.st = own >= 0 ? own + 1 : -2; /* :186-187 */
    s.st = s.inew > s.st ? s.inew : s.st;
    s.st = s.dnew > s.st ? s.dnew : s.st;
    return s;
}

// ---- generation rings -----------------------------------------------------------------------------------------------------------
// Three rings: `end` (M of the wavefront kernels), gm slots deep, and I and D, gi slots each; a slot holds rows x columns elements
// (lanes x threads, or lane rows x pairs), values stored + 2 so that a zero fill is "never reached".  `end` is read at
// generations e - o and e - x, I and D at e - ext.
#define LEAP_QUAD_PAIR_DWORDS(PD) (4 * (PD) + 1) /* a pair's four planes of PD dwords in LDS, pairs an odd number of dwords apart */

struct LvRings {
    int gm, gi;
    LU_HD static int pow2_above(int v) {
        int g = 2;
        while (g <= v) g <<= 1;
        return g;
    }
    /* slot = generation & (depth - 1): the LV kernels */
    LU_HD static LvRings pow2(int x, int o, int e) { return LvRings{pow2_above(x > o ? x : o), pow2_above(e)}; }
    /* slot = score mod depth, kept in counters: the wavefront kernels */
    LU_HD static LvRings exact(int x, int o, int e) { return LvRings{(x > o ? x : o) + 1, e + 1}; }
    /* unit penalties: two `end` slots, no I and D (leap_quad_kernel<UNIT>) */
    LU_HD static LvRings unit() { return LvRings{2, 0}; }
    LU_HD size_t ring_bytes(int rows, int columns, size_t elem) const {
        return ((size_t)(gm + 2 * gi) * rows * columns * elem + 3) & ~(size_t)3;
    }
    /* the LDS of the threads-share-a-pair kernels: per pair four planes of w32 dwords and a zero dword, then the rings with lane l at
     * row l + 1 between two guard rows */
    LU_HD size_t quad_lds(int pairs, int w32, int half_band, size_t elem) const {
        return (size_t)pairs * LEAP_QUAD_PAIR_DWORDS(w32 + 1) * sizeof(uint32_t) + ring_bytes(2 * half_band + 3, pairs, elem);
    }
};

template <typename EnT>
struct LvRingView { /* the seven pointers of one generation */
    const EnT *en_o, *en_x, *ip_e, *dp_e;
    EnT *en_w, *ip_w, *dp_w;
    /* by slot numbers: of e - o, e - x and e in the `end` ring, of e - ext and e in the I and D rings */
    LU_HD LvRingView(EnT* r_en, EnT* r_ip, EnT* r_dp, int slot, int sl_o, int sl_x, int sl_w, int sj_e, int sj_w)
        : en_o(r_en + sl_o * slot), en_x(r_en + sl_x * slot), ip_e(r_ip + sj_e * slot), dp_e(r_dp + sj_e * slot),
          en_w(r_en + sl_w * slot), ip_w(r_ip + sj_w * slot), dp_w(r_dp + sj_w * slot) {}
    /* by generation, power-of-two depths */
    LU_HD LvRingView(EnT* r_en, EnT* r_ip, EnT* r_dp, LvRings rg, int slot, int e, int x, int o, int ext)
        : LvRingView(r_en, r_ip, r_dp, slot, (e - o) & (rg.gm - 1), (e - x) & (rg.gm - 1), e & (rg.gm - 1), (e - ext) & (rg.gi - 1),
                     e & (rg.gi - 1)) {}
};

// ---- Gotoh ----------------------------------------------------------------------------------------------------------------------
// bit p of a multi-word vector (p >= 0; 0 beyond the vector)
template <int W64>
LU_HD uint32_t vw_bit(const VW<W64>& v, int p) {
    u64 word = 0;
#pragma unroll
    for (int q = 0; q < W64; q++)
        if ((p >> 6) == q) word = v.w[q];
    return (uint32_t)(word >> (p & 63)) & 1u;
}

#define NW_CB 32     /* columns of a block: its H and F rows live in registers */
#define NW_BIG 30000 /* "no path": H, E and F stay inside int16 */

struct NoCellSink { /* score only */
    LU_HD void row_begin() {}
    LU_HD void cell(int, int, int, int, int, int, int) {}
    LU_HD void row_end(int, int, int) {}
};

// Four facts per cell, the ones the oracle's traceback asks for (oracle/asm_oracle.c, orc_nw_cigar_batch):
//   bit 0  H == H[i-1][j-1] + sub      bit 1  H == E      bit 2  E == E[i][j-1] + e      bit 3  F == F[i-1][j] + e
// packed 8 cells per dword in scratch[((i-1) * cols8 + (j-1)/8) * stride + slot] (on the device: coalesced across a wave's pairs).
struct GotohTraceSink {
    uint32_t* scratch;
    long stride, slot;
    int cols8;
    uint32_t bits[NW_CB / 8];
    LU_HD void row_begin() {
#pragma unroll
        for (int q = 0; q < NW_CB / 8; q++) bits[q] = 0u;
    }
    LU_HD void cell(int jj, int h, int dg, int ee, int eext, int f, int fext) {
        const uint32_t nib = (h == dg ? 1u : 0u) | (h == ee ? 2u : 0u) | (ee == eext ? 4u : 0u) | (f == fext ? 8u : 0u);
        bits[jj >> 3] |= nib << (4 * (jj & 7));
    }
    LU_HD void row_end(int r, int j0, int nn) {
#pragma unroll
        for (int q = 0; q < NW_CB / 8; q++)
            if (j0 + 8 * q < nn) scratch[((long)(r - 1) * cols8 + (j0 >> 3) + q) * stride + slot] = bits[q];
    }
    LU_HD uint32_t nibble(int i, int j) const { /* cell (i, j), both >= 1 */
        return (scratch[((long)(i - 1) * cols8 + ((j - 1) >> 3)) * stride + slot] >> (4 * ((j - 1) & 7))) & 15u;
    }
};

// NW with affine gaps, arbitrary penalties: match 0, mismatch x, gap(L) = o + (L-1)*e — the score parasail's nw returns negated
// (benchmark_utils.h:139-142,288).  The matrix is swept in column blocks of NW_CB: a block's H and F rows live in registers (fully
// unrolled), and only the block's right-hand boundary column (H, E per row, packed as two int16 in one dword) goes through
// bound[r * stride], r = 1..m — on the device LDS laid out [row][thread], so a wave's accesses hit 64 different banks.
// The sink sees every cell before the NW_BIG clamps.  Returns H[m][nn].
template <int W64, typename Sink>
LU_HD int gotoh_sweep(const VW<W64>& A0, const VW<W64>& A1, const VW<W64>& B0, const VW<W64>& B1, int m, int nn, int x, int o, int e,
                      uint32_t* bound, int stride, Sink& sink) {
    int result = nn == 0 ? (m == 0 ? 0 : o + (m - 1) * e) : 0;
    for (int j0 = 0; j0 < nn; j0 += NW_CB) {
        // text codes of this column block
        uint32_t tb0 = 0, tb1 = 0;
#pragma unroll
        for (int q = 0; q < W64; q++) {
            if ((j0 >> 6) == q) {
                tb0 = (uint32_t)(B0.w[q] >> (j0 & 63));
                tb1 = (uint32_t)(B1.w[q] >> (j0 & 63));
            }
        }
        int H[NW_CB], F[NW_CB];
#pragma unroll
        for (int jj = 0; jj < NW_CB; jj++) {
            H[jj] = o + (j0 + jj) * e; /* H[0][j], j = j0+jj+1 */
            F[jj] = NW_BIG;
        }
        int diag = j0 == 0 ? 0 : o + (j0 - 1) * e; /* H[0][j0] */
        for (int r = 1; r <= m; r++) {
            // code of read character r-1, broadcast
            uint32_t a0 = 0, a1 = 0;
#pragma unroll
            for (int q = 0; q < W64; q++) {
                if (((r - 1) >> 6) == q) {
                    a0 = (uint32_t)(A0.w[q] >> ((r - 1) & 63)) & 1u;
                    a1 = (uint32_t)(A1.w[q] >> ((r - 1) & 63)) & 1u;
                }
            }
            const uint32_t mm = (tb0 ^ (0u - a0)) | (tb1 ^ (0u - a1));
            int hleft, eleft;
            if (j0 == 0) {
                hleft = o + (r - 1) * e; /* H[r][0] */
                eleft = NW_BIG;
            } else {
                const uint32_t pk = bound[r * stride];
                hleft = (int)(pk & 0xffffu);
                eleft = (int)(pk >> 16);
            }
            const int next_diag = hleft;
            sink.row_begin();
#pragma unroll
            for (int jj = 0; jj < NW_CB; jj++) {
                const int up = H[jj];
                const int fext = F[jj] + e;
                int f = up + o < fext ? up + o : fext;
                const int eext = eleft + e;
                int ee = hleft + o < eext ? hleft + o : eext;
                const int dg = diag + (((mm >> jj) & 1u) ? x : 0);
                int h = dg < f ? dg : f;
                h = ee < h ? ee : h;
                sink.cell(jj, h, dg, ee, eext, f, fext);
                f = f > NW_BIG ? NW_BIG : f;
                ee = ee > NW_BIG ? NW_BIG : ee;
                diag = up;
                H[jj] = h, F[jj] = f;
                hleft = h, eleft = ee;
            }
            diag = next_diag;
            bound[r * stride] = (uint32_t)hleft | ((uint32_t)eleft << 16);
            sink.row_end(r, j0, nn);
        }
        if (nn > j0 && nn <= j0 + NW_CB) {
            const int want = nn - j0 - 1;
#pragma unroll
            for (int jj = 0; jj < NW_CB; jj++)
                if (jj == want) result = H[jj];
        }
    }
    return result;
}

// The oracle's traceback over the trace of gotoh_sweep, rule by rule (oracle/asm_oracle.c, orc_nw_cigar_batch): in H prefer the
// diagonal, then E ('D'), then F ('I'); inside a gap prefer extending.  Walks back from (m, nn) and hands every run to
// runs(op, count, i) — op 1 'I', 2 'D', 3 '=', 4 'X'; i = the read position the run starts at — last run first.
template <int W64, typename Runs>
LU_HD void gotoh_traceback(const VW<W64>& A0, const VW<W64>& A1, const VW<W64>& B0, const VW<W64>& B1, int m, int nn,
                           const GotohTraceSink& tr, Runs& runs) {
    int cur_op = -1, cur_cnt = 0;
    int ii = m, j = nn, state = 0; /* 0 = H, 1 = E ('D'), 2 = F ('I') */
    for (int guard = 0; guard < 2 * ASM_MAX_LENGTH + 4 && (ii > 0 || j > 0); guard++) {
        int op = 0;
        const uint32_t nib = (ii > 0 && j > 0) ? tr.nibble(ii, j) : 0u;
        if (state == 0) {
            if (ii > 0 && j > 0 && (nib & 1u)) {
                const bool match = ((vw_bit<W64>(A0, ii - 1) ^ vw_bit<W64>(B0, j - 1)) |
                                    (vw_bit<W64>(A1, ii - 1) ^ vw_bit<W64>(B1, j - 1))) == 0u;
                op = match ? 3 : 4;
            } else if (j > 0 && (ii == 0 || (nib & 2u))) {
                state = 1; /* H == E; on row 0 H is E by construction */
            } else {
                state = 2;
            }
        } else if (state == 1) {
            op = 2;
            /* E[i][j] == E[i][j-1] + e, j > 1: on row 0 E[0][j] = o + (j-1) e, so always */
            if (!(j > 1 && (ii == 0 || (nib & 4u)))) state = 0;
        } else {
            op = 1;
            if (!(ii > 1 && (j == 0 || (nib & 8u)))) state = 0;
        }
        if (op == 0) continue;
        if (op != cur_op) {
            if (cur_cnt > 0) runs(cur_op, cur_cnt, ii);
            cur_op = op, cur_cnt = 0;
        }
        cur_cnt++;
        ii -= op != 2, j -= op != 1;
    }
    if (cur_cnt > 0) runs(cur_op, cur_cnt, ii);
}
