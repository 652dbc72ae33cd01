// The MD:Z tag of a SAM line (contract: docs/design/mapper.md, "MD tag"): the rule, written once, with no HIP in it.  hipcc compiles
// it into map_md_kernel (asm_map.h), plain g++ into asm_md_format (the C ABI's host helper) and into host/md_host_check.cpp, which
// tests/test_md_host.py runs under ASan + UBSan.
//
// md_format walks a CIGAR row forward (entry = count << 3 | op; 0 M, 1 I, 2 D) over q_s, the read on the alignment's strand in
// upper case, against the reference window T_r[pos, end):
//   M column  the bases are equal under the mapper's byte rule (A, C, G, T match only themselves; every other byte mismatches
//             everything, N against N included): the run counter goes up; else the counter (0 included), then the reference byte,
//             and the counter starts again
//   I         skips its read bases and writes nothing
//   D run     the counter, '^', the deleted reference bytes; the counter starts again, so a mismatch right behind a deletion reads
//             ^AC0T, as the SAM specification wants
//   end       the counter, always
// A reference byte is written as the text holds it (upper case); a byte outside A-Z ('*', '-', a digit) as 'N', so the tag always
// matches [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*.
//
// Size.  A record of the mapper has d <= MD_MAX_EDITS = 15 edits (MAP_MAX_ERRORS; asm_map.h checks that they agree).  Mismatch
// letters plus deleted letters are at most d; carets are at most the deletion runs, which are at most the deleted letters; numbers
// are at most mismatches + deletion runs + 1 <= 16, each of at most MD_NUM_DIGITS = 3 digits (m <= MAP_MAX_READ = 511).  The worst
// case is 15 single-base deletions: 3 * 16 + 15 + 15 = 78 bytes, MD_MAX_TAG; a row has MD_ROW_CAP = 80, which the C ABI publishes
// as ASM_MAP_MD_CAP (asm_map_host.h checks that they agree).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MD_HD __host__ __device__ inline
#else
#define MD_HD inline
#endif

#define MD_MAX_EDITS 15  /* the mapper's MAP_MAX_ERRORS */
#define MD_NUM_DIGITS 3  /* of a run counter: at most MAP_MAX_READ = 511 */
#define MD_MAX_TAG (MD_NUM_DIGITS * (MD_MAX_EDITS + 1) + 2 * MD_MAX_EDITS) /* 78: the longest tag (above) */
#define MD_ROW_CAP (MD_MAX_TAG + 2) /* 80: bytes of an item's MD row, the tag and, on the host, its NUL; the ABI's ASM_MAP_MD_CAP */
static_assert(MD_MAX_TAG == 78 && MD_ROW_CAP == 80 && MD_ROW_CAP <= 255, "an MD row holds the longest tag and its length fits a byte");

MD_HD bool md_is_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
MD_HD char md_ref_letter(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (char)c : 'N'; }

/* A sink over a row of `cap` < 2^32 - 1 bytes that never stores outside it: cur counts the tag's bytes, stored or not, and stops at
 * cap + 1, so cur > cap tells that the tag did not fit and no length can wrap.  Byte stores only. */
struct MdRowSink {
    char* out;
    uint32_t cap;
    uint32_t cur = 0;
    MD_HD void ch(char c) {
        if (cur < cap) out[cur] = c;
        if (cur <= cap) cur++;
    }
    MD_HD void num(uint32_t v) {
        uint32_t w = 1;
        for (uint32_t t = v; t >= 10u; t /= 10u) w++;
        for (uint32_t idx = w; idx-- > 0; v /= 10u)
            if (idx < cap - (cur < cap ? cur : cap)) out[cur + idx] = (char)('0' + v % 10u);
        cur = w > cap - (cur < cap ? cur : cap) ? cap + 1u : cur + w;
    }
};

/* The tag of the row ops[0, nops) into o (ch and num).  qbyte(p) is byte p of q_s, m its length; rbyte(p) byte p of the window, n
 * its length.
 * false, with o left anywhere, when an entry is no M, I or D or the row does not consume exactly m read and n reference bytes;
 * nothing outside [0, m) and [0, n) is read either way. */
template <class Q, class R, class Sink>
MD_HD bool md_format(const uint16_t* ops, uint32_t nops, Q&& qbyte, uint32_t m, R&& rbyte, uint32_t n, Sink& o) {
    uint32_t a = 0, b = 0, run = 0; /* read bases and reference bases consumed, matches since the last letter */
    for (uint32_t i = 0; i < nops; i++) {
        const uint32_t cnt = (uint32_t)(ops[i] >> 3), op = ops[i] & 7u;
        if (op > 2u) return false;
        if (op != 2u && cnt > m - a) return false;
        if (op != 1u && cnt > n - b) return false;
        if (op == 0u) {
            for (uint32_t t = 0; t < cnt; t++, a++, b++) {
                const uint8_t q = (uint8_t)qbyte(a), r = (uint8_t)rbyte(b);
                if (q == r && md_is_base(q)) {
                    run++;
                } else {
                    o.num(run), o.ch(md_ref_letter(r));
                    run = 0;
                }
            }
        } else if (op == 1u) {
            a += cnt;
        } else if (cnt) {
            o.num(run), o.ch('^');
            for (uint32_t t = 0; t < cnt; t++, b++) o.ch(md_ref_letter((uint8_t)rbyte(b)));
            run = 0;
        }
    }
    o.num(run);
    return a == m && b == n;
}
