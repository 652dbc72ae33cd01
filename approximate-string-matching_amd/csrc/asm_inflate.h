// The BGZF container read back (contract: docs/design/mapper.md, "Compressed input"): a deflate decoder (RFC 1951, complete) for one
// member at a time, the container's walk, and bgzf_inflate_kernel, one wavefront per member.
//
// A member's symbols are a serial chain, so the decoding is wave-uniform: bit buffer, position and every table entry are the same
// value in all 64 lanes (INF_UNIFORM: v_readfirstlane on the device), and the wave's width goes into the bytes.  Tokens are collected
// in batches of up to 64, lane t keeping token t and the output position it starts at; a batch's literals are stored at once, its
// matches then resolved in order, lane l copying out[p + l] = out[p - dist + l % dist] for l, l + 64, ... below the length, which reads
// only bytes in front of the match.  The member's whole output (at most 64 KiB) is an image in LDS; it starts at the 16-byte phase of
// its place in the text buffer, so that it is flushed in aligned 16-byte pieces.  The CRC is folded over the image in 64-byte slices
// with the tables and the slice code of asm_bgzf.h.
//
// Everything above the kernel holds no HIP: inf_member runs the same code on the host with the 64 lanes as a loop (INF_FOR_LANES),
// host/inflate_host_check.cpp compiles it with plain g++ under ASan + UBSan (tests/test_inflate_host.py).
//
// Totality.  Every bit comes out of InfBits, which loads no byte at or behind the member's compressed end and counts the bits it gave
// out against the bits there are (`avail`; below zero: INF_E_EOF).  A token's output position and its distance are checked where the
// token is decoded, before any lane stores: pos + len <= ISIZE <= 65 536 and dist <= pos.  A block's header consumes 3 bits, a token
// at least 1, a stored block 32 and its bytes, so every loop ends.
//
// Table sizes.  A decode table is a root of 2^R entries indexed by the next R bits and, for every root index that longer codes share,
// a subtable of 2^s entries, s = (the longest code under that index) - R.  Only complete codes are built (the two incomplete distance
// codes that are allowed have no code above 1 bit).  Under a complete code the subtree below a root index is a full binary tree; one
// of height s has at least s + 1 leaves.  So subtables of s_1, s_2, ... bits need sum(s_i + 1) <= N symbols, and their entries,
// sum(2^s_i), are largest when all but one have s = 15 - R: inf_sub_bound works the maximum out as a knapsack.
//   literal/length: N = 286, R = 10: 47 subtables of 32 and 8 more, 1 512; with the root 2 536 entries
//   distance:       N = 30,  R = 8:  3 of 128 and 32 more, 416; with the root 672 entries
// (zlib's exhaustive search gives less; this bound is what is proved here.)  The builder checks the room again before it places a
// subtable: an assert in the host build, INF_E_TABLE everywhere.
#pragma once
#include <assert.h>

#include "asm_bgzf.h"
#include "asm_bgzf_walk.h"

extern "C++" {

#define INF_IMG (INF_MAX_ISIZE + 16u) /* the image: up to 15 bytes of phase in front */
#define INF_LL_ROOT 10u
#define INF_D_ROOT 8u
#define INF_CL_ROOT 7u
#define INF_LL_MAX 286u
#define INF_D_MAX 30u
#define INF_LANES 64u

/* the status of a member: 0, or what is wrong with it */
enum {
    INF_OK = 0,
    INF_E_EOF = 1,      /* the stream runs past the member's compressed end */
    INF_E_BTYPE = 2,    /* BTYPE 3 */
    INF_E_STORED = 3,   /* a stored block's LEN is not ~NLEN */
    INF_E_HEADER = 4,   /* HLIT > 286 or HDIST > 30 */
    INF_E_CODELEN = 5,  /* the code-length code is over-subscribed or incomplete, or an unused code of it is read */
    INF_E_REPEAT = 6,   /* symbol 16 with no previous length, or a repeat past HLIT + HDIST */
    INF_E_LITLEN = 7,   /* the literal/length code is over-subscribed or incomplete, or has no end-of-block code */
    INF_E_DISTCODE = 8, /* the distance code is over-subscribed, or incomplete with more than one code or with one longer than a bit */
    INF_E_SYMBOL = 9,   /* length symbol 286 / 287, distance symbol 30 / 31, or an unused code */
    INF_E_DIST = 10,    /* a distance that reaches in front of the member's first byte */
    INF_E_OVERRUN = 11, /* more output than ISIZE */
    INF_E_ISIZE = 12,   /* less output than ISIZE */
    INF_E_CRC = 13,     /* the CRC-32 of the output is not the trailer's */
    INF_E_SLACK = 14,   /* whole bytes between the final block and the trailer */
    INF_E_TABLE = 15,   /* a decode table out of room: never, by the argument above */
    INF_E_CLASSES = 16
};
inline const char* inf_status_text(uint32_t s) {
    static const char* const text[INF_E_CLASSES] = {"no error",
                                                    "the deflate stream runs past the member's end",
                                                    "block type 3",
                                                    "a stored block's LEN is not ~NLEN",
                                                    "more than 286 literal/length or 30 distance codes",
                                                    "bad code-length code",
                                                    "bad code-length repeat",
                                                    "bad literal/length code",
                                                    "bad distance code",
                                                    "invalid symbol",
                                                    "distance reaches before the member's first byte",
                                                    "more output than ISIZE",
                                                    "less output than ISIZE",
                                                    "CRC-32 mismatch",
                                                    "bytes between the final block and the trailer",
                                                    "decode table out of room"};
    return s < INF_E_CLASSES ? text[s] : "unknown status";
}

/* the most subtable entries of a complete code of n symbols and at most 15 bits under a root of `root` bits (header comment) */
constexpr uint32_t inf_sub_bound(uint32_t n, uint32_t root) {
    uint32_t best[289] = {};
    for (uint32_t m = 0; m <= n; m++)
        for (uint32_t s = 1; s <= 15u - root; s++)
            if (m >= s + 1u && best[m - s - 1u] + (1u << s) > best[m]) best[m] = best[m - s - 1u] + (1u << s);
    uint32_t top = 0;
    for (uint32_t m = 0; m <= n; m++) top = best[m] > top ? best[m] : top;
    return top;
}
#define INF_LL_ENTRIES 2536u
#define INF_D_ENTRIES 672u
static_assert((1u << INF_LL_ROOT) + inf_sub_bound(INF_LL_MAX, INF_LL_ROOT) == INF_LL_ENTRIES, "the literal/length table's size is its bound");
static_assert((1u << INF_D_ROOT) + inf_sub_bound(INF_D_MAX, INF_D_ROOT) == INF_D_ENTRIES, "the distance table's size is its bound");
static_assert(INF_LL_ROOT >= 9u && INF_D_ROOT >= 5u, "the fixed codes (at most 9 and 5 bits) stay in the roots");

/* An entry, 16 bits: bits 0-3 the code bits this level takes (0: no such code), bit 4 set: a link, whose bits 5-15 are the subtable's
 * start / 2 and whose bits 0-3 are the subtable's index bits; else bits 5-15 are the symbol.  16-bit entries keep tables, image and CRC
 * table of a wave under 80 KiB, two waves to a CU; a lookup is one ds_read_u16 at a uniform address either way. */
#define INF_LINK 16u
#define INF_NOSYM 0xffffu

struct InfWork {
    uint16_t ll[INF_LL_ENTRIES];
    uint16_t d[INF_D_ENTRIES];
    uint16_t cl[1u << INF_CL_ROOT];
    uint16_t count[16], next[16];
    uint8_t lens[320]; /* HLIT + HDIST <= 316 code lengths; the fixed code's 288 + 32 */
};

/* one wave's LDS: the image, the CRC's slice-by-4 table, the work area */
#define INF_LDS_TABLE INF_IMG
#define INF_LDS_WORK (INF_LDS_TABLE + (uint32_t)sizeof(BgzfCrcTable))
#define INF_LDS_BYTES ((INF_LDS_WORK + (uint32_t)sizeof(InfWork) + 15u) & ~15u)

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define INF_FOR_LANES(l) for (uint32_t l = threadIdx.x & 63u, once_ = 1u; once_; once_ = 0u)
#define INF_SLOTS 1u
#define INF_ONE_LANE if ((threadIdx.x & 63u) == 0u)
#define INF_WAVE_ORDER()                                    \
    do {                                                    \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                    \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
#else
#define INF_UNIFORM(x) ((uint32_t)(x))
#define INF_FOR_LANES(l) for (uint32_t l = 0; l < INF_LANES; l++)
#define INF_SLOTS INF_LANES
#define INF_ONE_LANE
#define INF_WAVE_ORDER() ((void)0)
#endif

SAM_HD unsigned long long inf_uniform64(unsigned long long x) {
    return (unsigned long long)INF_UNIFORM((uint32_t)(x >> 32)) << 32 | INF_UNIFORM((uint32_t)x);
}

/* ---- bits --------------------------------------------------------------------------------------------------------------------- */
/* The stream of p[beg, end): dwords at 4-byte aligned addresses, clipped to `end` (a byte at or behind it is never loaded and reads
 * as zero; up to 3 bytes in front of beg, the member's own header, are loaded and dropped).  `avail`: the stream's bits not yet
 * given out; below zero once more were asked for than there are. */
struct InfBits {
    const uint8_t* b; /* p rounded down to 4 bytes */
    uint32_t next, end;
    uint64_t bb;
    uint32_t bc;
    int32_t avail;
};
SAM_HD uint32_t inf_load(const InfBits& r, uint32_t off) {
    uint32_t v = 0u;
    if (off + 4u <= r.end) __builtin_memcpy(&v, (const uint8_t*)__builtin_assume_aligned(r.b + off, 4), 4);
    else
        for (uint32_t k = 0; k < 3u; k++)
            if (off + k < r.end) v |= (uint32_t)r.b[off + k] << (8u * k);
    return INF_UNIFORM(v);
}
SAM_HD void inf_bits_at(InfBits& r, uint32_t at) { /* at <= end, both counted from b */
    r.next = (at & ~3u) + 4u;
    r.bb = (uint64_t)(inf_load(r, at & ~3u) >> (8u * (at & 3u)));
    r.bc = 32u - 8u * (at & 3u);
    r.avail = (int32_t)(8u * (r.end - at));
}
SAM_HD void inf_bits_open(InfBits& r, const uint8_t* p, uint32_t beg, uint32_t end) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    r.b = p - mis;
    r.end = end + mis;
    inf_bits_at(r, beg + mis);
}
/* at least 33 bits in the buffer afterwards */
SAM_HD void inf_refill(InfBits& r) {
    if (r.bc <= 32u) {
        r.bb |= (uint64_t)inf_load(r, r.next) << r.bc;
        r.next += 4u;
        r.bc += 32u;
    }
}
SAM_HD uint32_t inf_take(InfBits& r, uint32_t n) { /* n <= 16, and no more than 32 between two refills */
    const uint32_t v = (uint32_t)r.bb & ((1u << n) - 1u);
    r.bb >>= n;
    r.bc -= n;
    r.avail -= (int32_t)n;
    return v;
}

/* ---- tables ------------------------------------------------------------------------------------------------------------------- */
SAM_HD uint32_t inf_reverse(uint32_t code, uint32_t len) {
    uint32_t r = 0u;
    for (uint32_t k = 0; k < len; k++) r |= ((code >> k) & 1u) << (len - 1u - k);
    return r;
}
enum { INF_CODE_COMPLETE = 0, INF_CODE_OVER = 1, INF_CODE_INCOMPLETE = 2, INF_CODE_ONE = 3, INF_CODE_NONE = 4, INF_CODE_ROOM = 5 };
/* The table of the canonical code with lengths lens[0, n), each <= 15, in tab[0, cap).  INF_CODE_COMPLETE: built.  INF_CODE_ONE (one code,
 * of 1 bit) and INF_CODE_NONE: built too, the unused indexes holding no code.  Every other result leaves the table undefined.
 * inf_build clears the root with all lanes and runs the rest, inf_build_one, in one lane (it is a chain of read-modify-writes on
 * count, next and the table); the wave meets again behind it and every lane gets the result. */
SAM_HD uint32_t inf_build_one(uint16_t* tab, uint32_t root, uint32_t cap, const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* next) {
    for (uint32_t k = 0; k < 16u; k++) count[k] = 0u;
    for (uint32_t i = 0; i < n; i++) count[lens[i]] = (uint16_t)(count[lens[i]] + 1u);
    uint32_t used = n - count[0], left = 1u, code = 0u, longest = 0u;
    for (uint32_t k = 1; k < 16u; k++) {
        left <<= 1;
        if (count[k] > left) return INF_CODE_OVER;
        left -= count[k];
        code = (code + count[k - 1u] * (k > 1u)) << 1;
        next[k] = (uint16_t)code;
        if (count[k]) longest = k;
    }
    uint32_t kind = INF_CODE_COMPLETE;
    if (used == 0u) kind = INF_CODE_NONE;
    else if (left != 0u) {
        if (used != 1u || longest != 1u) return INF_CODE_INCOMPLETE;
        kind = INF_CODE_ONE;
    }
    const uint32_t nroot = 1u << root, rmask = nroot - 1u;
    /* the longest code under every root index that codes above the root share */
    if (longest > root) {
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t len = lens[i];
            if (len == 0u) continue;
            const uint32_t c = next[len];
            next[len] = (uint16_t)(c + 1u);
            if (len <= root) continue;
            const uint32_t at = inf_reverse(c, len) & rmask, had = INF_UNIFORM(tab[at]) & 15u;
            if (len - root > had) tab[at] = (uint16_t)(INF_LINK | (len - root));
        }
        uint32_t room = nroot;
        for (uint32_t i = 0; i < nroot; i++) {
            const uint32_t e = INF_UNIFORM(tab[i]);
            if (!(e & INF_LINK)) continue;
            const uint32_t size = 1u << (e & 15u);
#if !defined(__HIP_DEVICE_COMPILE__)
            assert(room + size <= cap && "a decode table above its bound");
#endif
            if (room + size > cap) return INF_CODE_ROOM;
            tab[i] = (uint16_t)(e | ((room >> 1) << 5));
            room += size;
        }
        for (uint32_t k = 1; k < 16u; k++) next[k] = (uint16_t)(next[k] - count[k]);
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = lens[i];
        if (len == 0u) continue;
        const uint32_t c = next[len];
        next[len] = (uint16_t)(c + 1u);
        const uint32_t rev = inf_reverse(c, len);
        if (len <= root) {
            for (uint32_t at = rev; at < nroot; at += 1u << len) tab[at] = (uint16_t)(len | (i << 5));
        } else {
            const uint32_t e = INF_UNIFORM(tab[rev & rmask]), sub = (e >> 5) << 1, size = 1u << (e & 15u), sl = len - root;
            for (uint32_t at = rev >> root; at < size; at += 1u << sl) tab[sub + at] = (uint16_t)(sl | (i << 5));
        }
    }
    return kind;
}
SAM_HD uint32_t inf_build(uint16_t* tab, uint32_t root, uint32_t cap, const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* next) {
    INF_FOR_LANES(l)
    for (uint32_t i = l; i < (1u << root); i += INF_LANES) tab[i] = 0u;
    INF_WAVE_ORDER();
    uint32_t kind = 0u;
    INF_ONE_LANE kind = inf_build_one(tab, root, cap, lens, n, count, next);
    INF_WAVE_ORDER();
    return INF_UNIFORM(kind);
}
/* the symbol that the buffer's next bits are the code of, and the code's length; INF_NOSYM: no code */
SAM_HD uint32_t inf_lookup(const uint16_t* tab, uint32_t root, uint32_t bits, uint32_t* used) {
    uint32_t e = INF_UNIFORM(tab[bits & ((1u << root) - 1u)]);
    *used = 0u;
    if (e & INF_LINK) {
        *used = root;
        e = INF_UNIFORM(tab[((e >> 5) << 1) + ((bits >> root) & ((1u << (e & 15u)) - 1u))]);
    }
    *used += e & 15u;
    return (e & 15u) ? e >> 5 : INF_NOSYM;
}

/* ---- tokens ------------------------------------------------------------------------------------------------------------------- */
/* lane t's token of the batch: a = position | length << 17; b = distance, or 0 for a literal, whose byte is in bits 16-23 */
struct InfTokens {
    uint32_t a[INF_SLOTS], b[INF_SLOTS];
};
#if defined(__HIP_DEVICE_COMPILE__)
#define INF_TOKEN(arr, m) ((uint32_t)__builtin_amdgcn_readlane((int)(arr)[0], (int)(m)))
#else
#define INF_TOKEN(arr, m) ((arr)[m])
#endif
SAM_HD void inf_put(InfTokens& tk, uint32_t n, uint32_t a, uint32_t b) {
    INF_FOR_LANES(l)
    if (l == n) tk.a[l % INF_SLOTS] = a, tk.b[l % INF_SLOTS] = b;
}
/* the batch's n tokens into the image (out: the image at the member's first byte) */
SAM_HD void inf_apply(uint8_t* out, const InfTokens& tk, uint32_t n) {
    uint64_t matches = 0u;
    INF_FOR_LANES(l)
    if (l < n && (tk.b[l % INF_SLOTS] & 0xffffu) == 0u) out[tk.a[l % INF_SLOTS] & 0x1ffffu] = (uint8_t)(tk.b[l % INF_SLOTS] >> 16);
#if defined(__HIP_DEVICE_COMPILE__)
    matches = __ballot((threadIdx.x & 63u) < n && (tk.b[0] & 0xffffu) != 0u);
#else
    for (uint32_t l = 0; l < n; l++) matches |= (uint64_t)((tk.b[l] & 0xffffu) != 0u) << l;
#endif
    INF_WAVE_ORDER();
    while (matches) {
        const uint32_t m = (uint32_t)__builtin_ctzll(matches);
        matches &= matches - 1u;
        const uint32_t a = INF_TOKEN(tk.a, m), dist = INF_TOKEN(tk.b, m) & 0xffffu, p = a & 0x1ffffu, len = a >> 17;
        INF_FOR_LANES(l)
        for (uint32_t i = l; i < len; i += INF_LANES) out[p + i] = out[p - dist + (dist >= len ? i : i % dist)];
        INF_WAVE_ORDER();
    }
}

/* ---- one member --------------------------------------------------------------------------------------------------------------- */
/* the code lengths of a dynamic block's header into w.lens, and its two tables; 0 or the status */
SAM_HD uint32_t inf_dynamic(InfBits& r, InfWork& w) {
    inf_refill(r);
    const uint32_t hlit = inf_take(r, 5) + 257u, hdist = inf_take(r, 5) + 1u, hclen = inf_take(r, 4) + 4u;
    if (r.avail < 0) return INF_E_EOF;
    if (hlit > INF_LL_MAX || hdist > INF_D_MAX) return INF_E_HEADER;
    /* 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each */
    const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                              11ull << 50 | 4ull << 55;
    const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    for (uint32_t i = 0; i < 19u; i++) {
        inf_refill(r);
        const uint32_t sym = (uint32_t)((i < 12u ? order_lo >> (5u * i) : order_hi >> (5u * (i - 12u))) & 31u);
        w.lens[sym] = (uint8_t)(i < hclen ? inf_take(r, 3) : 0u);
    }
    if (r.avail < 0) return INF_E_EOF;
    INF_WAVE_ORDER();
    if (inf_build(w.cl, INF_CL_ROOT, 1u << INF_CL_ROOT, w.lens, 19u, w.count, w.next) != INF_CODE_COMPLETE) return INF_E_CODELEN;
    const uint32_t total = hlit + hdist;
    for (uint32_t n = 0; n < total;) {
        inf_refill(r);
        uint32_t used = 0u;
        const uint32_t sym = inf_lookup(w.cl, INF_CL_ROOT, (uint32_t)r.bb, &used);
        if (sym == INF_NOSYM) return INF_E_CODELEN;
        (void)inf_take(r, used);
        uint32_t rep = 1u, val = sym;
        if (sym == 16u) {
            if (n == 0u) return INF_E_REPEAT;
            rep = 3u + inf_take(r, 2), val = INF_UNIFORM(w.lens[n - 1u]);
        } else if (sym == 17u) rep = 3u + inf_take(r, 3), val = 0u;
        else if (sym == 18u) rep = 11u + inf_take(r, 7), val = 0u;
        if (r.avail < 0) return INF_E_EOF;
        if (n + rep > total) return INF_E_REPEAT;
        for (uint32_t k = 0; k < rep; k++) w.lens[n + k] = (uint8_t)val;
        INF_WAVE_ORDER();
        n += rep;
    }
    if (INF_UNIFORM(w.lens[256]) == 0u) return INF_E_LITLEN;
    const uint32_t ll = inf_build(w.ll, INF_LL_ROOT, INF_LL_ENTRIES, w.lens, hlit, w.count, w.next);
    if (ll != INF_CODE_COMPLETE) return ll == INF_CODE_ROOM ? INF_E_TABLE : INF_E_LITLEN;
    const uint32_t d = inf_build(w.d, INF_D_ROOT, INF_D_ENTRIES, w.lens + hlit, hdist, w.count, w.next);
    if (d == INF_CODE_ROOM) return INF_E_TABLE;
    if (d != INF_CODE_COMPLETE && d != INF_CODE_ONE && d != INF_CODE_NONE) return INF_E_DISTCODE;
    return INF_OK;
}
SAM_HD uint32_t inf_fixed(InfWork& w) {
    INF_FOR_LANES(l)
    for (uint32_t i = l; i < 320u; i += INF_LANES) w.lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
    INF_WAVE_ORDER();
    if (inf_build(w.ll, INF_LL_ROOT, INF_LL_ENTRIES, w.lens, 288u, w.count, w.next) != INF_CODE_COMPLETE) return INF_E_TABLE;
    if (inf_build(w.d, INF_D_ROOT, INF_D_ENTRIES, w.lens + 288u, 32u, w.count, w.next) != INF_CODE_COMPLETE) return INF_E_TABLE;
    return INF_OK;
}

/* the tokens of one Huffman block, from behind its header up to its end-of-block code, into the image; *opos: the output position */
SAM_HD uint32_t inf_tokens(InfBits& r, const InfWork& w, uint8_t* out, uint32_t isize, uint32_t* opos) {
    InfTokens tk = {};
    uint32_t n = 0u, pos = *opos;
    for (;;) {
        if (r.avail < 0) return INF_E_EOF;
        inf_refill(r);
        uint32_t used = 0u;
        const uint32_t sym = inf_lookup(w.ll, INF_LL_ROOT, (uint32_t)r.bb, &used);
        if (sym == INF_NOSYM) return INF_E_SYMBOL;
        (void)inf_take(r, used);
        if (sym < 256u) {
            if (pos >= isize) return INF_E_OVERRUN;
            inf_put(tk, n++, pos | 1u << 17, sym << 16);
            pos++;
        } else if (sym == 256u) {
            if (r.avail < 0) return INF_E_EOF;
            inf_apply(out, tk, n);
            *opos = pos;
            return INF_OK;
        } else {
            if (sym > 285u) return INF_E_SYMBOL;
            uint32_t len = sym - 254u;
            if (sym == 285u) len = 258u;
            else if (sym >= 265u) {
                const uint32_t e = (sym - 261u) >> 2;
                len = ((4u + ((sym - 261u) & 3u)) << e) + 3u + inf_take(r, e);
            }
            inf_refill(r);
            const uint32_t dsym = inf_lookup(w.d, INF_D_ROOT, (uint32_t)r.bb, &used);
            if (dsym == INF_NOSYM || dsym >= INF_D_MAX) return INF_E_SYMBOL;
            (void)inf_take(r, used);
            uint32_t dist = dsym + 1u;
            if (dsym >= 4u) {
                const uint32_t e = (dsym >> 1) - 1u;
                dist = ((2u + (dsym & 1u)) << e) + 1u + inf_take(r, e);
            }
            if (r.avail < 0) return INF_E_EOF;
            if (dist > pos) return INF_E_DIST;
            if (pos + len > isize) return INF_E_OVERRUN;
            inf_put(tk, n++, pos | len << 17, dist);
            pos += len;
        }
        if (n == INF_LANES) inf_apply(out, tk, n), n = 0u;
    }
}

/* the image's CRC-32: out[0, len) with `phase` zero bytes in front, which start at a 16-byte boundary and leave a register of zero as
 * it is; the register's initial ones are brought behind the len bytes by x^(8 len).  Lane t folds slices t, t + 64, ... */
SAM_HD uint32_t inf_crc(const uint8_t* img, uint32_t phase, uint32_t len, const BgzfCrcTable& T, const BgzfTables& G) {
    if (len == 0u) return 0u;
    const BgzfCut c = bgzf_cut(phase + len);
    uint32_t front = 0u, last_state = 0u;
    INF_FOR_LANES(l) {
        uint32_t acc = 0u, mine = 0u, j = l;
        bool any = false, holds_last = false;
        for (; j <= c.last; j += INF_LANES) {
            const uint32_t nbytes = bgzf_slice_bytes(c, j);
            const uint32_t s = bgzf_crc_slice(T, 0u, bgzf_load_slice(img + BGZF_SLICE * j, nbytes), nbytes);
            if (j == c.last) {
                holds_last = true, mine = s;
                if (any) acc = bgzf_mul(acc, G.pow_slices[INF_LANES - 1u]); /* from slice last - 64 to slice last - 1 */
            } else {
                acc = any ? bgzf_mul(acc, G.pow_slices[INF_LANES]) ^ s : s;
            }
            any = true;
        }
        /* acc stands at the end of this lane's last slice in front of `last`: j - 64, or j - 128 for the lane that holds `last` */
        if (holds_last) last_state ^= mine;
        else if (any) acc = bgzf_mul(acc, G.pow_slices[c.last - 1u - (j - INF_LANES)]);
        if (any) front ^= acc;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    for (int off = 32; off > 0; off >>= 1) front ^= __shfl_xor(front, off), last_state ^= __shfl_xor(last_state, off);
#endif
    const uint32_t q = len / BGZF_SLICE, ones = bgzf_mul(bgzf_mul(G.pow_slices[q / 2u], G.pow_slices[q - q / 2u]), G.pow_bytes[len % BGZF_SLICE]);
    return ~(bgzf_mul(front, G.pow_bytes[c.last_len]) ^ last_state ^ bgzf_mul(0xffffffffu, ones));
}

/* One member: the deflate stream p[beg, end) into the image (img: 16-byte aligned, INF_IMG bytes, the output from img + phase on,
 * phase < 16), its length against isize <= INF_MAX_ISIZE and its CRC against crc.  The status; the image is whole only under INF_OK. */
SAM_HD uint32_t inf_member(const uint8_t* p, uint32_t beg, uint32_t end, uint32_t isize, uint32_t crc, uint8_t* img, uint32_t phase, InfWork& w,
                           const BgzfCrcTable& T, const BgzfTables& G) {
    INF_FOR_LANES(l)
    if (l < 16u) img[l] = 0u;
    uint8_t* const out = img + phase;
    InfBits r;
    inf_bits_open(r, p, beg, end);
    uint32_t opos = 0u;
    for (;;) {
        inf_refill(r);
        const uint32_t bfinal = inf_take(r, 1), btype = inf_take(r, 2);
        if (r.avail < 0) return INF_E_EOF;
        if (btype == 0u) {
            (void)inf_take(r, (uint32_t)r.avail & 7u);
            inf_refill(r);
            const uint32_t len = inf_take(r, 16), nlen = inf_take(r, 16);
            if (r.avail < 0) return INF_E_EOF;
            if (len != (~nlen & 0xffffu)) return INF_E_STORED;
            if (len > (uint32_t)r.avail >> 3) return INF_E_EOF;
            if (opos + len > isize) return INF_E_OVERRUN;
            const uint32_t at = r.end - ((uint32_t)r.avail >> 3);
            INF_FOR_LANES(l)
            for (uint32_t i = l; i < len; i += INF_LANES) out[opos + i] = r.b[at + i];
            INF_WAVE_ORDER();
            opos += len;
            inf_bits_at(r, at + len);
        } else if (btype == 3u) {
            return INF_E_BTYPE;
        } else {
            if (const uint32_t s = btype == 1u ? inf_fixed(w) : inf_dynamic(r, w)) return s;
            if (const uint32_t s = inf_tokens(r, w, out, isize, &opos)) return s;
        }
        if (bfinal) break;
    }
    if (opos != isize) return INF_E_ISIZE;
    if (r.avail >= 8) return INF_E_SLACK;
    INF_WAVE_ORDER();
    return inf_crc(img, phase, isize, T, G) == crc ? INF_OK : INF_E_CRC;
}

/* the image's len bytes to d, whose address has the image's phase: 16 bytes at a time, single bytes at the two ends */
SAM_HD void inf_flush(const uint8_t* img, uint32_t phase, uint32_t len, uint8_t* d) {
    uint8_t* const d0 = d - phase; /* 16-byte aligned */
    const uint32_t pieces = (phase + len + 15u) / 16u;
    INF_FOR_LANES(l)
    for (uint32_t g = l; g < pieces; g += INF_LANES) {
        if (16u * g >= phase && 16u * g + 16u <= phase + len) {
            __builtin_memcpy(__builtin_assume_aligned(d0 + 16u * g, 16), (const uint8_t*)__builtin_assume_aligned(img + 16u * g, 16), 16);
        } else {
            for (uint32_t k = 0; k < 16u; k++)
                if (16u * g + k >= phase && 16u * g + k < phase + len) d0[16u * g + k] = img[16u * g + k];
        }
    }
}

/* the first failed member of a launch: member << 8 | status, the smallest wins; ~0: none */
#define INF_NONE_BAD 0xffffffffffffffffull

/* the members decoded serially by the code the kernel runs, into dst[0, total); the first failed member as the kernel reports it */
inline unsigned long long bgzf_inflate_host(const uint8_t* src, const std::vector<InfMember>& members, uint8_t* dst) {
    std::vector<uint32_t> aligned(INF_IMG / 4u + 8u);
    uint8_t* const img = (uint8_t*)(((uintptr_t)aligned.data() + 15u) & ~(uintptr_t)15u);
    std::vector<InfWork> w(1);
    unsigned long long bad = INF_NONE_BAD;
    for (size_t k = 0; k < members.size(); k++) {
        const InfMember& m = members[k];
        uint8_t* const d = dst + m.out_off;
        const uint32_t phase = (uint32_t)((uintptr_t)d & 15u);
        const uint32_t s = inf_member(src + m.src_off, m.dstart, m.csize - 8u, m.isize, m.crc, img, phase, w[0], bgzf_host_tables().t, bgzf_host_tables());
        if (s == INF_OK) {
            inf_flush(img, phase, m.isize, d);
        } else if (((unsigned long long)k << 8 | s) < bad) {
            bad = (unsigned long long)k << 8 | s;
        }
    }
    return bad;
}

#if defined(__HIPCC__)

/* One wavefront per member, the grid striding over the launch's members: member m's deflate stream out of src, its output to
 * dst[out_off, out_off + isize) when it is sound; a failed member leaves its place in dst as it was and brings m << 8 | status into
 * *first_bad (atomicMin).  Reads only the bytes of the members' entries, which the host has checked against the chunk; dst: 16-byte
 * aligned.  LDS: INF_LDS_BYTES of dynamic LDS. */
__global__ __launch_bounds__(INF_LANES) void bgzf_inflate_kernel(const uint8_t* __restrict__ src, const InfMember* __restrict__ members,
                                                                 uint32_t nmembers, uint8_t* __restrict__ dst,
                                                                 unsigned long long* __restrict__ first_bad) {
    extern __shared__ uint4 inf_lds[];
    uint8_t* const img = (uint8_t*)inf_lds;
    BgzfCrcTable& table = *(BgzfCrcTable*)(img + INF_LDS_TABLE);
    InfWork& w = *(InfWork*)(img + INF_LDS_WORK);
    for (uint32_t i = threadIdx.x; i < 1024u; i += INF_LANES) (&table[0][0])[i] = (&bgzf_device_tables.t[0][0])[i];
    INF_WAVE_ORDER();
    for (uint32_t m = blockIdx.x; m < nmembers; m += gridDim.x) {
        const unsigned long long src_off = inf_uniform64(members[m].src_off), out_off = inf_uniform64(members[m].out_off);
        const uint32_t csize = INF_UNIFORM(members[m].csize), dstart = INF_UNIFORM(members[m].dstart), isize = INF_UNIFORM(members[m].isize),
                       crc = INF_UNIFORM(members[m].crc);
        uint8_t* const d = dst + out_off;
        const uint32_t phase = INF_UNIFORM((uint32_t)((uintptr_t)d & 15u));
        const uint32_t s = inf_member(src + src_off, dstart, csize - 8u, isize, crc, img, phase, w, table, bgzf_device_tables);
        if (s == INF_OK) inf_flush(img, phase, isize, d);
        else if (threadIdx.x == 0u) atomicMin(first_bad, (unsigned long long)m << 8 | s);
        INF_WAVE_ORDER();
    }
}

/* the members (a host table, checked by bgzf_walk against the n bytes at d_src) decoded into d_dst, 16-byte aligned; *d_bad: set to
 * INF_NONE_BAD here, the first failed member afterwards.  On the handle's stream; no members launch nothing. */
static hipError_t bgzf_inflate_device(asm_handle* h, const uint8_t* d_src, const InfMember* d_members, size_t nmembers, uint8_t* d_dst,
                                      unsigned long long* d_bad) {
    if (const hipError_t e = hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), h->stream)) return e;
    if (nmembers == 0) return hipSuccess;
    const unsigned grid = (unsigned)(nmembers < 512u ? nmembers : 512u); /* two waves' LDS to a CU, 256 CUs */
    return launch_lds(h, bgzf_inflate_kernel, grid, INF_LANES, INF_LDS_BYTES, d_src, d_members, (uint32_t)nmembers, d_dst, d_bad);
}

#endif /* __HIPCC__ */

} /* extern "C++" */

#if defined(__HIPCC__)
/* ---- C entry points: asm_bgzf_decompressed_size, asm_bgzf_decompress, asm_bgzf_decompress_host ------------------------------------- */
/* a container the walk refused: plain gzip in front is ASM_EUNSUPPORTED, everything else ASM_EINVAL, naming member and offset */
static int bgzf_in_fail(asm_handle* h, const std::string& who, const uint8_t* src, size_t n, const BgzfWalkError& err) {
    if (err.member == 0 && bgzf_is_plain_gzip(src, n))
        return fail(h, ASM_EUNSUPPORTED, who + ": the input is plain gzip, not BGZF (no BC subfield in its first member): recompress it with bgzip");
    return fail(h, ASM_EINVAL, who + ": BGZF member " + std::to_string(err.member) + " at offset " + std::to_string(err.offset) + ": " + bgzf_in_text(err.status));
}
/* a member the decoder refused; bad: member << 8 | status */
static int bgzf_member_fail(asm_handle* h, const std::string& who, const std::vector<InfMember>& members, unsigned long long bad) {
    const size_t k = (size_t)(bad >> 8);
    return fail(h, ASM_EINVAL, who + ": BGZF member " + std::to_string(k) + " at offset " + std::to_string(k < members.size() ? members[k].src_off : 0ull) +
                                   ": " + inf_status_text((uint32_t)(bad & 0xffu)));
}
/* the walk and the argument checks the two decompress calls share */
static int bgzf_decompress_open(asm_handle* h, const std::string& who, const void* src, size_t n, void* dst, size_t dst_cap, size_t* dst_len,
                                std::vector<InfMember>& members, size_t* total) {
    if ((n && !src) || !dst_len) return fail(h, ASM_EINVAL, who + ": NULL argument");
    const BgzfWalkError err = bgzf_walk((const uint8_t*)src, n, &members, total);
    if (err.status != BGZF_IN_OK) return bgzf_in_fail(h, who, (const uint8_t*)src, n, err);
    if (dst_cap < *total || (*total && !dst))
        return fail(h, ASM_EINVAL, who + ": dst_cap is below asm_bgzf_decompressed_size (" + std::to_string(*total) + " bytes)");
    if (members.size() >= 0xffffffffull) return fail(h, ASM_EUNSUPPORTED, who + ": 2^32 members or more");
    return ASM_OK;
}
int asm_bgzf_decompressed_size(const void* src, size_t n, size_t* out_len) {
    const std::string who = "asm_bgzf_decompressed_size";
    if ((n && !src) || !out_len) return fail(nullptr, ASM_EINVAL, who + ": NULL argument");
    size_t total = 0;
    const BgzfWalkError err = bgzf_walk((const uint8_t*)src, n, nullptr, &total);
    if (err.status != BGZF_IN_OK) return bgzf_in_fail(nullptr, who, (const uint8_t*)src, n, err);
    *out_len = total;
    return ASM_OK;
}
int asm_bgzf_decompress_host(const void* src, size_t n, void* dst, size_t dst_cap, size_t* dst_len) {
    const std::string who = "asm_bgzf_decompress_host";
    std::vector<InfMember> members;
    size_t total = 0;
    if (const int rc = bgzf_decompress_open(nullptr, who, src, n, dst, dst_cap, dst_len, members, &total)) return rc;
    *dst_len = 0;
    /* into a buffer of the call's own, so that dst stays as it was when a member fails */
    std::vector<uint8_t> out(total);
    const unsigned long long bad = bgzf_inflate_host((const uint8_t*)src, members, out.data());
    if (bad != INF_NONE_BAD) return bgzf_member_fail(nullptr, who, members, bad);
    if (total) memcpy(dst, out.data(), total);
    *dst_len = total;
    return ASM_OK;
}
int asm_bgzf_decompress(asm_handle* h, const void* src, size_t n, void* dst, size_t dst_cap, size_t* dst_len) {
    const char* who = "asm_bgzf_decompress";
    const std::string call = who;
    if (!h) return fail(h, ASM_EINVAL, call + ": NULL argument");
    std::vector<InfMember> members;
    size_t total = 0;
    if (const int rc = bgzf_decompress_open(h, call, src, n, dst, dst_cap, dst_len, members, &total)) return rc;
    *dst_len = 0;
    if (members.empty()) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    Scratch<uint8_t> d_src(h), d_dst(h);
    Scratch<InfMember> d_members(h);
    Scratch<unsigned long long> d_bad(h);
    STREAM_TRY(who, d_src.alloc(n + 16));
    STREAM_TRY(who, d_dst.alloc(total + 16));
    STREAM_TRY(who, d_members.alloc(sizeof(InfMember) * members.size()));
    STREAM_TRY(who, d_bad.alloc(sizeof(unsigned long long)));
    STREAM_TRY(who, hipMemcpyAsync(d_src.p, src, n, hipMemcpyHostToDevice, h->stream));
    STREAM_TRY(who, hipMemcpyAsync(d_members.p, members.data(), sizeof(InfMember) * members.size(), hipMemcpyHostToDevice, h->stream));
    STREAM_TRY(who, bgzf_inflate_device(h, d_src.p, d_members.p, members.size(), d_dst.p, d_bad.p));
    unsigned long long bad = INF_NONE_BAD;
    STREAM_TRY(who, fetch(h, {fetched(&bad, (const unsigned long long*)d_bad.p)}));
    if (bad != INF_NONE_BAD) return bgzf_member_fail(h, call, members, bad);
    if (total) STREAM_TRY(who, hipMemcpyAsync(dst, d_dst.p, total, hipMemcpyDeviceToHost, h->stream));
    STREAM_TRY(who, hipStreamSynchronize(h->stream));
    *dst_len = total;
    return ASM_OK;
}
#endif /* __HIPCC__ */
