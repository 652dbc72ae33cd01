// Host build of the banded unit-cost NW sweeps (csrc/asm_nwband.h) for the CPU test-suite: the very functions nw_banded_kernel
// and nw_banded2_kernel run per thread — nw_band<4, 32>, nw_band<4, 64> and the two-pairs-per-dword nw_band2x16<4> — driven
// pair by pair on the host, so that tests/test_nw_pair2_host.py can diff them against the oracle without a GPU.  The packed
// 16-bit operations take their plain C++ meaning here.  Test support only: nothing in the product links this file.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_nwband.h"

namespace {
constexpr int ND = 4; /* one 128-base granule per string */

struct Planes {
    uint32_t a0[ND + 2], a1[ND + 2], b0[ND], b1[ND]; /* the read's planes carry two zero dwords of padding (nw_band<>) */
    int m, n;
};

// bit_convert.cpp:340-355: A=00 C=01 G=10 T=11, anything else 00; plane 0 holds the low bit of base q at bit q
void fill(uint32_t* p0, uint32_t* p1, const unsigned char* s, int len) {
    for (int q = 0; q < len; q++) {
        const int code = s[q] == 'C' ? 1 : s[q] == 'G' ? 2 : s[q] == 'T' ? 3 : 0;
        if (code & 1) p0[q >> 5] |= 1u << (q & 31);
        if (code & 2) p1[q >> 5] |= 1u << (q & 31);
    }
}

bool load(Planes& P, long i, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs, const uint32_t* ref_off) {
    memset(&P, 0, sizeof P);
    P.m = (int)(read_off[i + 1] - read_off[i]);
    P.n = (int)(ref_off[i + 1] - ref_off[i]);
    if (P.m > 32 * ND || P.n > 32 * ND) return false;
    fill(P.a0, P.a1, reads + read_off[i], P.m);
    fill(P.b0, P.b1, refs + ref_off[i], P.n);
    return true;
}
}  // namespace

// nw_band<4, W> of every pair: out[i] = the banded result, or -1 where the window does not prove one.  W = 32 or 64.
extern "C" int nw_host_band(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                            const uint32_t* ref_off, int W, int32_t* out) {
    for (long i = 0; i < n; i++) {
        Planes P;
        if (!load(P, i, reads, read_off, refs, ref_off)) return -2;
        if (W == 32)
            out[i] = nw_band<ND, 32>(P.a0, P.a1, P.b0, P.b1, P.m, P.n);
        else if (W == 64)
            out[i] = nw_band<ND, 64>(P.a0, P.a1, P.b0, P.b1, P.m, P.n);
        else
            return -1;
    }
    return 0;
}

// nw_band2x16<4> of the k couples (ip[j], iq[j]): rp[j], rq[j] = what the low and the high half report (-1: not proven)
extern "C" int nw_host_pair2(const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs, const uint32_t* ref_off,
                             long k, const int64_t* ip, const int64_t* iq, int32_t* rp, int32_t* rq) {
    for (long j = 0; j < k; j++) {
        Planes P, Q;
        if (!load(P, ip[j], reads, read_off, refs, ref_off) || !load(Q, iq[j], reads, read_off, refs, ref_off)) return -2;
        int a = -1, b = -1;
        nw_band2x16<ND>(P.a0, P.a1, P.b0, P.b1, P.m, P.n, Q.a0, Q.a1, Q.b0, Q.b1, Q.m, Q.n, a, b);
        rp[j] = a, rq[j] = b;
    }
    return 0;
}

// ---- the packed column against a one-pair restatement, block by block (tests/test_nw_band2_column_host.py) ---------------
// One pair in a 16-row window, written out in uint16_t with the textbook column of nw_band<>'s fused form (every shift and the
// TOP bit explicit, nothing shared with nw_band2x16<>'s opcode choices): st[4 * bq .. + 3] = (VPin, VNin, S, 1) after the last
// column this pair has in block bq; blocks in which it has none stay as they were.
namespace {
void band16_blocks(const Planes& P, int32_t* st) {
    const auto bit = [](const uint32_t* pl, int q) -> uint16_t { return q >= 0 && q < 32 * ND ? (pl[q >> 5] >> (q & 31)) & 1u : 0u; };
    const auto window = [&](const uint32_t* pl, int top) { /* pattern rows top .. top+15 (1-based) at bits 0..15 */
        uint16_t w = 0;
        for (int k = 0; k < 16; k++) w |= (uint16_t)(bit(pl, top - 1 + k) << k);
        return w;
    };
    uint16_t VP = 0xFFFFu, VN = 0;
    int S = 16;
    for (int j = 1; j <= P.n && j <= 8; j++) { /* plain form on rows 1..16 */
        const uint16_t T0 = bit(P.b0, j - 1) ? 0xFFFFu : 0, T1 = bit(P.b1, j - 1) ? 0xFFFFu : 0;
        const uint16_t Eq = ~((window(P.a0, 1) ^ T0) | (window(P.a1, 1) ^ T1));
        const uint16_t D0 = (uint16_t)((((uint16_t)(Eq & VP) + VP) ^ VP) | Eq | VN);
        const uint16_t HP = VN | (uint16_t)~(D0 | VP), HN = VP & D0;
        S += (HP >> 15) - (HN >> 15);
        const uint16_t X = (uint16_t)(HP << 1) | 1u;
        VP = (uint16_t)(HN << 1) | (uint16_t)~(D0 | X);
        VN = D0 & X;
    }
    uint16_t VPin = (VP >> 1) | 0x8000u, VNin = VN >> 1;
    for (int j = 9; j <= P.n; j++) { /* column j's window: rows j-7 .. j+8 */
        const uint16_t T0 = bit(P.b0, j - 1) ? 0xFFFFu : 0, T1 = bit(P.b1, j - 1) ? 0xFFFFu : 0;
        const uint16_t Eq = ~((window(P.a0, j - 7) ^ T0) | (window(P.a1, j - 7) ^ T1));
        const uint16_t D0 = (uint16_t)((((uint16_t)(Eq & VPin) + VPin) ^ VPin) | Eq | VNin);
        const uint16_t HP = VNin | (uint16_t)~(D0 | VPin), HN = VPin & D0;
        S += 1 - (D0 >> 15);
        const uint16_t D0s = D0 >> 1;
        VPin = HN | (uint16_t)~(D0s | HP) | 0x8000u;
        VNin = HP & D0s;
        int32_t* o = st + 4 * ((j - 1) / 16);
        o[0] = VPin, o[1] = VNin, o[2] = S, o[3] = 1;
    }
}
struct BlockState {
    int32_t* p;
    int32_t* q;
    void operator()(int bq, uint32_t vpin, uint32_t vnin, int sp, int sq) const {
        p[4 * bq] = (int32_t)(vpin & 0xFFFFu), p[4 * bq + 1] = (int32_t)(vnin & 0xFFFFu), p[4 * bq + 2] = sp, p[4 * bq + 3] = 1;
        q[4 * bq] = (int32_t)(vpin >> 16), q[4 * bq + 1] = (int32_t)(vnin >> 16), q[4 * bq + 2] = sq, q[4 * bq + 3] = 1;
    }
};
}  // namespace

// For the k couples (ip[j], iq[j]): got_p / got_q[j][bq] = (VPin, VNin, S, seen) of each half after block bq of nw_band2x16<4>
// (seen = 0 where the sweep did not run the block), want_p / want_q the same from band16_blocks of each pair alone (seen = 0
// where the pair has no column in the block).  8 blocks of 4 int32 per couple and side, zeroed here.
extern "C" int nw_host_pair2_blocks(const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                                    const uint32_t* ref_off, long k, const int64_t* ip, const int64_t* iq, int32_t* got_p,
                                    int32_t* got_q, int32_t* want_p, int32_t* want_q) {
    constexpr int PER = 4 * 2 * ND;
    memset(got_p, 0, sizeof(int32_t) * PER * k), memset(got_q, 0, sizeof(int32_t) * PER * k);
    memset(want_p, 0, sizeof(int32_t) * PER * k), memset(want_q, 0, sizeof(int32_t) * PER * k);
    for (long j = 0; j < k; j++) {
        Planes P, Q;
        if (!load(P, ip[j], reads, read_off, refs, ref_off) || !load(Q, iq[j], reads, read_off, refs, ref_off)) return -2;
        int a = -1, b = -1;
        const BlockState sink{got_p + PER * j, got_q + PER * j};
        nw_band2x16<ND, ND + 2, BlockState>(P.a0, P.a1, P.b0, P.b1, P.m, P.n, Q.a0, Q.a1, Q.b0, Q.b1, Q.m, Q.n, a, b, sink);
        band16_blocks(P, want_p + PER * j);
        band16_blocks(Q, want_q + PER * j);
    }
    return 0;
}

// The last stage of the cascade on the device is the full-height bit-parallel sweep (nw_unit_full, GPU only); the host
// check closes its cascade with the plain dynamic programme instead.
extern "C" int nw_host_full(long n, const unsigned char* reads, const uint32_t* read_off, const unsigned char* refs,
                            const uint32_t* ref_off, int32_t* out) {
    std::vector<int> row;
    for (long i = 0; i < n; i++) {
        const unsigned char* a = reads + read_off[i];
        const unsigned char* b = refs + ref_off[i];
        const int m = (int)(read_off[i + 1] - read_off[i]), nn = (int)(ref_off[i + 1] - ref_off[i]);
        row.assign((size_t)m + 1, 0);
        for (int r = 0; r <= m; r++) row[r] = r;
        for (int j = 1; j <= nn; j++) {
            int diag = row[0];
            row[0] = j;
            for (int r = 1; r <= m; r++) {
                const int sub = diag + (a[r - 1] != b[j - 1]);
                diag = row[r];
                int best = sub < row[r] + 1 ? sub : row[r] + 1;
                row[r] = best < row[r - 1] + 1 ? best : row[r - 1] + 1;
            }
        }
        out[i] = row[m];
    }
    return 0;
}
