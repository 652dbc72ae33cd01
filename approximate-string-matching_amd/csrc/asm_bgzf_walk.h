// The BGZF container walked on the host, without decoding (contract: docs/design/mapper.md, "Compressed input"): a member's header
// (magic, CM 8, FLG 4, the XLEN walk to the BC subfield of 2 bytes), BSIZE, and CRC-32 and ISIZE of its trailer.  No HIP and nothing
// of the library: asm_host.h (the file calls' BGZF fill policy) and asm_inflate.h (the decoder) both include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#define INF_MAX_ISIZE 65536u

/* a member of the chunk, as the host's walk found it; the kernel reads src[src_off, src_off + csize) and writes
 * dst[out_off, out_off + isize) */
struct InfMember {
    unsigned long long src_off, out_off;
    uint32_t csize;  /* BSIZE + 1 */
    uint32_t dstart; /* where the deflate stream begins in the member: 12 + XLEN; it ends at csize - 8 */
    uint32_t isize, crc;
};

/* ---- the container ------------------------------------------------------------------------------------------------------------ */
enum {
    BGZF_IN_OK = 0,
    BGZF_IN_MAGIC = 1,   /* not 1f 8b 08 with FLG 4 */
    BGZF_IN_NO_BC = 2,   /* no BC subfield of 2 bytes in the extra field */
    BGZF_IN_BSIZE = 3,   /* BSIZE + 1 below the member's own header and trailer */
    BGZF_IN_PAST_END = 4, /* the header or the member reaches past the end */
    BGZF_IN_ISIZE = 5,   /* ISIZE above 65 536 */
    BGZF_IN_CLASSES = 6
};
inline const char* bgzf_in_text(uint32_t s) {
    static const char* const text[BGZF_IN_CLASSES] = {"no error",
                                                      "not a BGZF member header (1f 8b 08 04)",
                                                      "no BC subfield in the gzip extra field",
                                                      "BSIZE is smaller than the member's header and trailer",
                                                      "the member reaches past the end of the file",
                                                      "ISIZE is above 65536"};
    return s < BGZF_IN_CLASSES ? text[s] : "unknown status";
}
/* The member header at p[0, have), have < 18 included.  BGZF_IN_OK: *csize = BSIZE + 1 and *dstart are set, and csize >= dstart + 8 (an
 * empty member has a deflate stream of two bytes, but that is the decoder's to say).  BGZF_IN_PAST_END: `have` ends inside the header. */
inline uint32_t bgzf_member_header(const uint8_t* p, size_t have, uint32_t* csize, uint32_t* dstart) {
    static const uint8_t magic[4] = {0x1f, 0x8b, 0x08, 0x04};
    for (size_t i = 0; i < 4u && i < have; i++)
        if (p[i] != magic[i]) return BGZF_IN_MAGIC;
    if (have < 12u) return BGZF_IN_PAST_END;
    const uint32_t xlen = p[10] | (uint32_t)p[11] << 8;
    if (have < 12u + (size_t)xlen) return BGZF_IN_PAST_END;
    uint32_t bsize = 0u;
    bool found = false;
    for (uint32_t at = 0; at + 4u <= xlen;) {
        const uint8_t* f = p + 12u + at;
        const uint32_t slen = f[2] | (uint32_t)f[3] << 8;
        if (at + 4u + slen > xlen) break;
        if (f[0] == 'B' && f[1] == 'C' && slen == 2u && !found) found = true, bsize = f[4] | (uint32_t)f[5] << 8;
        at += 4u + slen;
    }
    if (!found) return BGZF_IN_NO_BC;
    *csize = bsize + 1u;
    *dstart = 12u + xlen;
    if (*csize < 26u || *csize < *dstart + 8u) return BGZF_IN_BSIZE;
    return BGZF_IN_OK;
}
/* is p[0, have) the start of a gzip file that is not BGZF?  (for the refusal of plain gzip) */
inline bool bgzf_is_plain_gzip(const uint8_t* p, size_t have) {
    uint32_t csize = 0u, dstart = 0u;
    if (have < 2u || p[0] != 0x1fu || p[1] != 0x8bu) return false;
    const uint32_t s = bgzf_member_header(p, have, &csize, &dstart);
    return s == BGZF_IN_MAGIC || s == BGZF_IN_NO_BC;
}
/* The members of src[0, n), their output offsets the exclusive sum of ISIZE.  BGZF_IN_OK, or the first bad member's status with its
 * index and offset. */
struct BgzfWalkError {
    uint32_t status = BGZF_IN_OK;
    size_t member = 0, offset = 0;
};
inline BgzfWalkError bgzf_walk(const uint8_t* src, size_t n, std::vector<InfMember>* members, size_t* total) {
    BgzfWalkError err;
    size_t at = 0, out = 0, k = 0;
    while (at < n) {
        uint32_t csize = 0u, dstart = 0u;
        uint32_t s = bgzf_member_header(src + at, n - at, &csize, &dstart);
        if (s == BGZF_IN_OK && csize > n - at) s = BGZF_IN_PAST_END;
        uint32_t isize = 0u, crc = 0u;
        if (s == BGZF_IN_OK) {
            const uint8_t* t = src + at + csize - 8u;
            crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
            if (isize > INF_MAX_ISIZE) s = BGZF_IN_ISIZE;
        }
        if (s != BGZF_IN_OK) {
            err.status = s, err.member = k, err.offset = at;
            return err;
        }
        if (members) members->push_back(InfMember{(unsigned long long)at, (unsigned long long)out, csize, dstart, isize, crc});
        at += csize, out += isize, k++;
    }
    if (total) *total = out;
    return err;
}
