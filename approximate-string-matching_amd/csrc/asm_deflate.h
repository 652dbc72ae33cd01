// The deflate encoder of the BGZF container at ASM_BGZF_DEFLATE (contract: docs/design/mapper.md, "Deflate").  Included by asm_bgzf.h,
// behind its host-buildable part, whose slices, CRC and fixed bytes it uses.  One BGZF block is one deflate block with BFINAL = 1:
// stored, fixed Huffman or dynamic Huffman, whichever has the fewest bits (a tie goes to the lower BTYPE), so no block is longer
// than its stored form.
//
// bgzf_deflate_kernel, one workgroup of 1024 threads per block, everything in LDS (DeflateLds: 157 984 bytes, one workgroup per CU):
//   matches   the block is walked in windows of 1024 positions, thread i at position 1024 w + i.  A position hashes its four bytes
//             into `wfirst` (the window's earliest position per hash, atomicMin) and, a window later, into `prev` (the latest position
//             of the earlier windows per hash, atomicMax); barriers separate the inserts from the lookups, so what a lookup reads is
//             a function of the payload alone.  Both candidates lie in front of the position; each is verified against the payload,
//             dropped beyond a distance of 32 768 and clipped at the end of the 64-byte slice that holds the position.
//   parse     a wave holds exactly one slice of a window.  The greedy parse is a wave-uniform walk over the lanes' match lengths; it
//             gives the mask of lanes that start a token.  Pass 1 counts the tokens' symbols (atomicAdd), pass 2 emits them.
//   codes     lengths limited to 15 (7 for the code-length alphabet): the used symbols ranked by (count, symbol) in parallel, then
//             by one thread per alphabet Moffat and Katajainen's in-place minimum-redundancy lengths, the Kraft repair of the
//             overlong ones and the canonical codes.  An alphabet with fewer than two used symbols gets zlib's dummies, so every
//             code is complete.
//   emit      pass 2 finds the matches again (keeping them would take more LDS than a CU has), scans the tokens' bit counts across
//             the wave and the window's 16 waves, and ORs the bits into the bit buffer (atomicOr on dwords).
// Every table's content is defined by min, max, add and or, and nothing depends on which thread comes first: the bytes are a pure
// function of the payload, and dfl_block_host, which runs the same per-position code serially, gives the same ones.
//
// Not built: matches across slices (so none is longer than 64, although the symbol mapping covers 258), lazy or optimal parsing,
// further levels.
#pragma once

#define DFL_WIN 1024u                   /* positions per window: one per thread */
#define DFL_PREV (1u << 12)             /* entries of `prev` */
#define DFL_WTAB (1u << 11)             /* entries of `wfirst` */
#define DFL_PAYW (BGZF_PAYLOAD / 4u + 4u) /* dwords of the payload and of the bit buffer: four behind the last byte */
#define DFL_NLL 288u                    /* slots of the literal/length alphabet (286 in use); the distance alphabet follows it */
#define DFL_ND 32u                      /* slots of the distance alphabet (30 in use) */
#define DFL_SYMS (DFL_NLL + DFL_ND)
#define DFL_NCL 19u
#define DFL_STRIDE 65312u               /* where the kernel leaves block b for the compaction: BGZF_BLOCK rounded up to 16 */
#define DFL_NONE 0xffffffffu
#define DFL_TOO_FAR 4096u               /* a match of three bytes further back than this costs more than its literals (zlib's rule) */

struct DeflateLds {
    uint32_t pay[DFL_PAYW];  /* the payload, little endian */
    uint32_t bits[DFL_PAYW]; /* the deflate stream; before that, the CRC table of the first step */
    uint32_t prev[DFL_PREV]; /* position + 1 of the latest earlier-window position per hash, 0: none; between the passes, the builder's */
    uint32_t wfirst[DFL_WTAB]; /* the earliest position of the current window per hash, DFL_NONE: none */
    uint32_t hist[DFL_SYMS];
    uint32_t code[DFL_SYMS]; /* the bit-reversed code, its length << 16 */
    uint32_t misc[64];
};
enum { DFL_M_FRONT = 0, DFL_M_LAST = 16, DFL_M_CRC, DFL_M_TYPE, DFL_M_HEAD, DFL_M_BITS, DFL_M_FIXED, DFL_M_DYN, DFL_M_WAVE = 32 };
/* the builder's arrays inside prev */
enum { DFL_B_W = 0, DFL_B_ORDER = DFL_SYMS, DFL_B_LEN = 2 * DFL_SYMS, DFL_B_A = 3 * DFL_SYMS, DFL_B_USED = 4 * DFL_SYMS, DFL_B_END = 4 * DFL_SYMS + 2 };
static_assert(DFL_WTAB == 2u * BGZF_THREADS, "a thread clears two entries of wfirst");
static_assert(DFL_B_END <= DFL_PREV, "the builder's arrays fit into prev");
static_assert(sizeof(DeflateLds) <= 160u * 1024u, "one CU's LDS");
static_assert(sizeof(BgzfCrcTable) <= sizeof(uint32_t) * DFL_PAYW, "the CRC table fits into the bit buffer");
static_assert(DFL_STRIDE >= BGZF_BLOCK && DFL_STRIDE % 16u == 0, "the compaction loads whole 16-byte pieces");

/* min, max, add and or on a table entry: atomic among the workgroup's threads, plain in the serial host build */
SAM_HD void dfl_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
SAM_HD void dfl_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
SAM_HD void dfl_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
SAM_HD void dfl_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

SAM_HD uint32_t dfl_get4(const uint32_t* pay, uint32_t p) { return sam_funnel(pay[(p >> 2) + 1u], pay[p >> 2], p & 3u); }
SAM_HD uint32_t dfl_hash(uint32_t x, uint32_t entries_log2) { return (x * 0x9e3779b1u) >> (32u - entries_log2); }
SAM_HD uint32_t dfl_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

/* the symbol of a length in [3, 258] or of a distance in [1, 32 768], with its extra bits */
struct DflSym {
    uint32_t sym, nextra, extra;
};
SAM_HD DflSym dfl_len_sym(uint32_t len) {
    const uint32_t l = len - 3u;
    if (len == 258u) return {285u, 0u, 0u};
    if (l < 8u) return {257u + l, 0u, 0u};
    const uint32_t eb = dfl_log2(l) - 2u;
    return {257u + 4u * (eb + 1u) + ((l >> eb) & 3u), eb, l & ((1u << eb) - 1u)};
}
SAM_HD DflSym dfl_dist_sym(uint32_t dist) {
    const uint32_t d = dist - 1u;
    if (d < 4u) return {d, 0u, 0u};
    const uint32_t k = dfl_log2(d);
    return {2u * k + ((d >> (k - 1u)) & 1u), k - 1u, d & ((1u << (k - 1u)) - 1u)};
}
/* the extra bits of a symbol of the two alphabets in one numbering (s < DFL_NLL: literal/length) */
SAM_HD uint32_t dfl_sym_extra(uint32_t s) {
    if (s < DFL_NLL) return s < 265u || s >= 285u ? 0u : (s - 261u) >> 2;
    const uint32_t d = s - DFL_NLL;
    return d < 4u ? 0u : (d >> 1) - 1u;
}
SAM_HD uint32_t dfl_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : s < DFL_NLL ? 8u : 5u; }
SAM_HD uint32_t dfl_rev(uint32_t v, uint32_t n) {
    uint32_t r = 0u;
    for (uint32_t i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1u - i);
    return r;
}

/* where the slice of position p ends in a block of len bytes */
SAM_HD uint32_t dfl_slice_end(uint32_t p, uint32_t len) {
    const uint32_t e = (p / BGZF_SLICE + 1u) * BGZF_SLICE;
    return e < len ? e : len;
}
/* does position p of a block of len bytes have four bytes to hash? */
SAM_HD bool dfl_hashed(uint32_t p, uint32_t len) { return p + 4u <= len; }

/* how many bytes agree at c < p and p, at most cap */
SAM_HD uint32_t dfl_agree(const uint32_t* pay, uint32_t c, uint32_t p, uint32_t cap) {
    uint32_t k = 0u;
    while (k < cap) {
        const uint32_t x = dfl_get4(pay, c + k) ^ dfl_get4(pay, p + k);
        if (x) {
            k += (uint32_t)__builtin_ctz(x) >> 3;
            break;
        }
        k += 4u;
    }
    return k < cap ? k : cap;
}
/* The match of position p, whose four bytes are x: the longer of the two candidates, the nearer one when they tie.  Length 0: none. */
struct DflMatch {
    uint32_t len, dist;
};
SAM_HD DflMatch dfl_lookup(const DeflateLds& L, uint32_t p, uint32_t len, uint32_t x) {
    DflMatch m = {0u, 0u};
    const uint32_t cap = dfl_slice_end(p, len) - p;
    if (!dfl_hashed(p, len) || cap < 3u) return m;
    const uint32_t far = L.prev[dfl_hash(x, 12u)], near = L.wfirst[dfl_hash(x, 11u)];
    if (far != 0u && p - (far - 1u) <= 32768u) m = {dfl_agree(L.pay, far - 1u, p, cap < 258u ? cap : 258u), p - (far - 1u)};
    if (near < p) {
        const uint32_t n = dfl_agree(L.pay, near, p, cap < 258u ? cap : 258u);
        if (n >= m.len) m = {n, p - near};
    }
    if (m.len < 3u || (m.len == 3u && m.dist > DFL_TOO_FAR)) m = {0u, 0u};
    return m;
}
/* the token that starts at a position: the literal byte b, or the match m; counted, or as bits (at most 48) */
SAM_HD void dfl_count(uint32_t* hist, uint32_t b, const DflMatch& m) {
    if (m.len == 0u) {
        dfl_add(&hist[b], 1u);
        return;
    }
    dfl_add(&hist[dfl_len_sym(m.len).sym], 1u);
    dfl_add(&hist[DFL_NLL + dfl_dist_sym(m.dist).sym], 1u);
}
struct DflBits {
    uint64_t v;
    uint32_t n;
};
SAM_HD void dfl_append(DflBits& o, uint32_t v, uint32_t n) { o.v |= (uint64_t)v << o.n, o.n += n; }
SAM_HD DflBits dfl_token(const uint32_t* code, uint32_t b, const DflMatch& m) {
    DflBits o = {0u, 0u};
    if (m.len == 0u) {
        dfl_append(o, code[b] & 0xffffu, code[b] >> 16);
        return o;
    }
    const DflSym l = dfl_len_sym(m.len), d = dfl_dist_sym(m.dist);
    dfl_append(o, code[l.sym] & 0xffffu, code[l.sym] >> 16);
    dfl_append(o, l.extra, l.nextra);
    dfl_append(o, code[DFL_NLL + d.sym] & 0xffffu, code[DFL_NLL + d.sym] >> 16);
    dfl_append(o, d.extra, d.nextra);
    return o;
}
/* n <= 48 bits of v into the bit buffer at bit `at` */
SAM_HD void dfl_put(uint32_t* bits, uint32_t at, uint64_t v, uint32_t n) {
    if (n == 0u) return;
    const uint32_t i = at >> 5, s = at & 31u;
    const uint64_t lo = v << s;
    const uint32_t hi = s ? (uint32_t)(v >> (64u - s)) : 0u;
    if ((uint32_t)lo) dfl_or(&bits[i], (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) dfl_or(&bits[i + 1u], (uint32_t)(lo >> 32));
    if (hi) dfl_or(&bits[i + 2u], hi);
}

/* ---- the codes ------------------------------------------------------------------------------------------------------------------- */
/* zlib's dummies: an alphabet w[0, n) with fewer than two used symbols gets symbols of weight 1 until it has two */
SAM_HD void dfl_two_symbols(uint32_t* w, uint32_t n) {
    uint32_t used = 0u;
    int top = -1;
    for (uint32_t i = 0; i < n; i++)
        if (w[i]) used++, top = (int)i;
    while (used < 2u) {
        const uint32_t s = top < 2 ? (uint32_t)++top : 0u;
        w[s] = 1u, used++;
    }
}
/* the place of symbol i among the used ones of w[0, n) in the order of (weight, symbol); DFL_NONE for an unused one */
SAM_HD uint32_t dfl_rank(const uint32_t* w, uint32_t n, uint32_t i) {
    const uint32_t wi = w[i];
    if (wi == 0u) return DFL_NONE;
    uint32_t r = 0u;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t wj = w[j];
        r += (wj != 0u && (wj < wi || (wj == wi && j < i))) ? 1u : 0u;
    }
    return r;
}
/* The code lengths of the `used` symbols order[0, used) (in the order of dfl_rank, weights w), at most `limit` bits, into len[0, n);
 * a: `used` dwords of scratch.  Moffat and Katajainen's in-place lengths, then the overlong codes folded into `limit` and the Kraft
 * sum repaired from the longest codes up, then the lengths handed out from the rarest symbol down. */
SAM_HD void dfl_lengths(const uint32_t* w, const uint32_t* order, uint32_t used, uint32_t limit, uint32_t* a, uint32_t* len, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) len[i] = 0u;
    if (used == 0u) return;
    if (used == 1u) {
        len[order[0]] = 1u;
        return;
    }
    const int m = (int)used;
    for (int i = 0; i < m; i++) a[i] = w[order[i]];
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; next++) {
        if (leaf >= m || a[root] < a[leaf]) a[next] = a[root], a[root++] = (uint32_t)next;
        else a[next] = a[leaf++];
        if (leaf >= m || (root < next && a[root] < a[leaf])) a[next] += a[root], a[root++] = (uint32_t)next;
        else a[next] += a[leaf++];
    }
    a[m - 2] = 0u;
    for (int next = m - 3; next >= 0; next--) a[next] = a[a[next]] + 1u;
    int avbl = 1, inner = 0, next = m - 1;
    uint32_t depth = 0u;
    root = m - 2;
    while (avbl > 0) {
        while (root >= 0 && a[root] == depth) inner++, root--;
        while (avbl > inner) a[next--] = depth, avbl--;
        avbl = 2 * inner, depth++, inner = 0;
    }
    uint32_t num[16] = {0u};
    for (int i = 0; i < m; i++) num[a[i] < limit ? a[i] : limit]++;
    uint32_t total = 0u;
    for (uint32_t l = limit; l > 0u; l--) total += num[l] << (limit - l);
    while (total != (1u << limit)) {
        num[limit]--;
        for (uint32_t l = limit - 1u; l > 0u; l--)
            if (num[l]) {
                num[l]--, num[l + 1u] += 2u;
                break;
            }
        total--;
    }
    uint32_t j = used;
    for (uint32_t l = 1u; l <= limit; l++)
        for (uint32_t c = num[l]; c > 0u; c--) len[order[--j]] = l;
}
/* the canonical codes of len[0, n), bit-reversed, with the length << 16 */
SAM_HD void dfl_codes(const uint32_t* len, uint32_t n, uint32_t* code) {
    uint32_t count[16] = {0u}, next[16] = {0u};
    for (uint32_t i = 0; i < n; i++) count[len[i]]++;
    count[0] = 0u;
    for (uint32_t l = 1u; l < 16u; l++) next[l] = (next[l - 1u] + count[l - 1u]) << 1;
    for (uint32_t i = 0; i < n; i++) code[i] = len[i] ? dfl_rev(next[len[i]]++, len[i]) | (len[i] << 16) : 0u;
}

/* the header of a dynamic block behind its three type bits: counted (bits == NULL) or written at bit `at`.  ll, d: the two
 * alphabets' lengths; gives the bits it takes. */
struct DflHeadSink {
    uint32_t* bits;
    uint32_t at, n;
    uint32_t* cl_hist;        /* counting: the code-length alphabet's histogram */
    const uint32_t* cl_code;  /* writing: its codes */
    SAM_HD void put(uint32_t v, uint32_t nb) {
        if (bits) dfl_put(bits, at + n, v, nb);
        n += nb;
    }
    SAM_HD void sym(uint32_t s, uint32_t extra, uint32_t nextra) {
        if (cl_hist) {
            cl_hist[s]++;
            return;
        }
        put(cl_code[s] & 0xffffu, cl_code[s] >> 16);
        put(extra, nextra);
    }
};
SAM_HD uint32_t dfl_head_len(const uint32_t* ll, const uint32_t* d, uint32_t hlit, uint32_t i) { return i < hlit ? ll[i] : d[i - hlit]; }
/* the two alphabets' lengths as symbols of the code-length alphabet: 16 repeats the last length 3 to 6 times, 17 and 18 are 3 to 10
 * and 11 to 138 zeros */
SAM_HD void dfl_head_runs(DflHeadSink& s, const uint32_t* ll, const uint32_t* d, uint32_t hlit, uint32_t hdist) {
    const uint32_t n = hlit + hdist;
    uint32_t i = 0u;
    while (i < n) {
        const uint32_t v = dfl_head_len(ll, d, hlit, i);
        uint32_t run = 1u;
        while (i + run < n && dfl_head_len(ll, d, hlit, i + run) == v) run++;
        i += run;
        if (v == 0u) {
            while (run >= 11u) {
                const uint32_t r = run < 138u ? run : 138u;
                s.sym(18u, r - 11u, 7u), run -= r;
            }
            if (run >= 3u) s.sym(17u, run - 3u, 3u), run = 0u;
        } else {
            s.sym(v, 0u, 0u), run--;
            while (run >= 3u) {
                const uint32_t r = run < 6u ? run : 6u;
                s.sym(16u, r - 3u, 2u), run -= r;
            }
        }
        while (run > 0u) s.sym(v, 0u, 0u), run--;
    }
}
SAM_HD uint32_t dfl_cl_order(uint32_t i) {
    const uint64_t lo = 0x0b050a0609070800ull, hi = 0x0f010e020d030c04ull; /* 0 8 7 9 6 10 5 11, 4 12 3 13 2 14 1 15 */
    return i < 3u ? 16u + i : i < 11u ? (uint32_t)(lo >> (8u * (i - 3u))) & 0xffu : (uint32_t)(hi >> (8u * (i - 11u))) & 0xffu;
}

/* One thread, behind both alphabets' lengths (b + DFL_B_LEN) and the histogram: the code-length alphabet, the three types' bit
 * counts and the choice; the chosen type's codes into L.code and its header into the bit buffer.  misc: DFL_M_TYPE, DFL_M_HEAD (the
 * bits in front of the first token), DFL_M_BITS (the whole block's); in the host build also DFL_M_FIXED and DFL_M_DYN, the counts
 * of the two Huffman types, for host/deflate_host_check.cpp. */
SAM_HD void dfl_choose(DeflateLds& L, uint32_t len) {
    uint32_t* const b = L.prev;
    const uint32_t *ll = b + DFL_B_LEN, *d = b + DFL_B_LEN + DFL_NLL;
    uint32_t fixed = 3u, dyn = 0u;
    for (uint32_t s = 0; s < DFL_SYMS; s++) {
        fixed += L.hist[s] * (dfl_fixed_len(s) + dfl_sym_extra(s));
        dyn += L.hist[s] * (b[DFL_B_LEN + s] + dfl_sym_extra(s));
    }
    uint32_t hlit = 286u, hdist = 30u;
    while (hlit > 257u && ll[hlit - 1u] == 0u) hlit--;
    while (hdist > 1u && d[hdist - 1u] == 0u) hdist--;
    uint32_t cl_w[DFL_NCL] = {0u}, cl_order[DFL_NCL], cl_a[DFL_NCL], cl_len[DFL_NCL], cl_code[DFL_NCL];
    DflHeadSink count = {nullptr, 0u, 0u, cl_w, nullptr};
    dfl_head_runs(count, ll, d, hlit, hdist);
    uint32_t cl_hist[DFL_NCL];
    for (uint32_t i = 0; i < DFL_NCL; i++) cl_hist[i] = cl_w[i];
    dfl_two_symbols(cl_w, DFL_NCL);
    uint32_t used = 0u;
    for (uint32_t i = 0; i < DFL_NCL; i++) {
        const uint32_t r = dfl_rank(cl_w, DFL_NCL, i);
        if (r != DFL_NONE) cl_order[r] = i, used++;
    }
    dfl_lengths(cl_w, cl_order, used, 7u, cl_a, cl_len, DFL_NCL);
    dfl_codes(cl_len, DFL_NCL, cl_code);
    uint32_t hclen = DFL_NCL;
    while (hclen > 4u && cl_len[dfl_cl_order(hclen - 1u)] == 0u) hclen--;
    uint32_t head = 3u + 14u + 3u * hclen;
    for (uint32_t i = 0; i < DFL_NCL; i++) head += cl_hist[i] * (cl_len[i] + (i == 16u ? 2u : i == 17u ? 3u : i == 18u ? 7u : 0u));
    dyn += head;
    const uint32_t stored = 40u + 8u * len;
    const uint32_t type = stored <= fixed && stored <= dyn ? 0u : fixed <= dyn ? 1u : 2u;
    L.misc[DFL_M_TYPE] = type, L.misc[DFL_M_HEAD] = type == 2u ? head : 3u, L.misc[DFL_M_BITS] = type == 0u ? stored : type == 1u ? fixed : dyn;
#if !defined(__HIP_DEVICE_COMPILE__)
    L.misc[DFL_M_FIXED] = fixed, L.misc[DFL_M_DYN] = dyn;
#endif
    if (type == 0u) return;
    dfl_put(L.bits, 0u, 1u | (type << 1), 3u);
    if (type == 1u) {
        uint32_t* const fl = b + DFL_B_A; /* free by now */
        for (uint32_t s = 0; s < DFL_SYMS; s++) fl[s] = dfl_fixed_len(s);
        dfl_codes(fl, DFL_NLL, L.code);
        dfl_codes(fl + DFL_NLL, DFL_ND, L.code + DFL_NLL);
        return;
    }
    dfl_codes(ll, DFL_NLL, L.code);
    dfl_codes(d, DFL_ND, L.code + DFL_NLL);
    DflHeadSink out = {L.bits, 3u, 0u, nullptr, cl_code};
    out.put(hlit - 257u, 5u), out.put(hdist - 1u, 5u), out.put(hclen - 4u, 4u);
    for (uint32_t i = 0; i < hclen; i++) out.put(cl_len[dfl_cl_order(i)], 3u);
    dfl_head_runs(out, ll, d, hlit, hdist);
}

/* the 18 bytes in front of a block's deflate stream; `block`: the whole block's bytes */
SAM_HD uint8_t dfl_head_byte(uint32_t i, uint32_t block) { return i < 16u ? bgzf_front_byte(i, 0u) : (uint8_t)((block - 1u) >> (8u * (i - 16u))); }
#define DFL_HEAD 18u

/* ---- the serial host build -------------------------------------------------------------------------------------------------------- */
/* one pass over the windows, as the kernel's threads make it: emit == false counts the symbols, emit == true writes the tokens' bits
 * from bit `at` on and gives the bit behind the last one */
inline uint32_t dfl_pass_host(DeflateLds& L, uint32_t len, bool emit, uint32_t at) {
    for (uint32_t i = 0; i < DFL_PREV; i++) L.prev[i] = 0u;
    for (uint32_t i = 0; i < DFL_WTAB; i++) L.wfirst[i] = DFL_NONE;
    DflMatch m[DFL_WIN];
    for (uint32_t w = 0; DFL_WIN * w < len; w++) {
        for (uint32_t t = 0; t < DFL_WIN; t++) {
            const uint32_t p = DFL_WIN * w + t;
            if (dfl_hashed(p, len)) dfl_min(&L.wfirst[dfl_hash(dfl_get4(L.pay, p), 11u)], p);
            if (w > 0u && dfl_hashed(p - DFL_WIN, len)) dfl_max(&L.prev[dfl_hash(dfl_get4(L.pay, p - DFL_WIN), 12u)], p - DFL_WIN + 1u);
        }
        for (uint32_t t = 0; t < DFL_WIN; t++) {
            const uint32_t p = DFL_WIN * w + t;
            m[t] = p < len ? dfl_lookup(L, p, len, dfl_hashed(p, len) ? dfl_get4(L.pay, p) : 0u) : DflMatch{0u, 0u};
        }
        for (uint32_t t = 0; t < DFL_WTAB; t++) L.wfirst[t] = DFL_NONE;
        for (uint32_t s = 0; s < DFL_WIN / BGZF_SLICE; s++) /* a slice's greedy parse */
            for (uint32_t t = BGZF_SLICE * s; t < BGZF_SLICE * (s + 1u) && DFL_WIN * w + t < len; t += m[t].len ? m[t].len : 1u) {
                const uint32_t b = (L.pay[(DFL_WIN * w + t) >> 2] >> (8u * (t & 3u))) & 0xffu;
                if (!emit) {
                    dfl_count(L.hist, b, m[t]);
                    continue;
                }
                const DflBits o = dfl_token(L.code, b, m[t]);
                dfl_put(L.bits, at, o.v, o.n);
                at += o.n;
            }
    }
    return at;
}
/* both alphabets' lengths from the histogram, into the builder's arrays inside prev */
inline void dfl_build_host(DeflateLds& L) {
    uint32_t* const b = L.prev;
    for (uint32_t s = 0; s < DFL_SYMS; s++) b[DFL_B_W + s] = L.hist[s];
    dfl_two_symbols(b + DFL_B_W + DFL_NLL, DFL_ND);
    for (uint32_t k = 0; k < 2u; k++) {
        const uint32_t base = k ? DFL_NLL : 0u, n = k ? DFL_ND : DFL_NLL;
        uint32_t used = 0u;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t r = dfl_rank(b + DFL_B_W + base, n, i);
            if (r != DFL_NONE) b[DFL_B_ORDER + base + r] = i, used++;
        }
        dfl_lengths(b + DFL_B_W + base, b + DFL_B_ORDER + base, used, 15u, b + DFL_B_A + base, b + DFL_B_LEN + base, n);
    }
}
/* The block of p[0, len), len in [1, BGZF_PAYLOAD], onto the end of out, as bgzf_deflate_kernel writes it; p as in bgzf_block_host.
 * type: the block's BTYPE; counts: the bits dfl_choose counted for the fixed and for the dynamic form, or NULL. */
inline void dfl_block_host(DeflateLds& L, const uint8_t* p, uint32_t len, std::vector<uint8_t>& out, uint32_t* type, uint32_t* counts = nullptr) {
    memset(&L, 0, sizeof L);
    memcpy(L.pay, p, len);
    const uint32_t crc = bgzf_block_host(p, len, nullptr);
    L.hist[256] = 1u;
    dfl_pass_host(L, len, false, 0u);
    dfl_build_host(L);
    dfl_choose(L, len);
    *type = L.misc[DFL_M_TYPE];
    if (counts) counts[0] = L.misc[DFL_M_FIXED], counts[1] = L.misc[DFL_M_DYN];
    const size_t blk = out.size();
    if (*type == 0u) {
        out.resize(blk + BGZF_FRONT + len + BGZF_BACK);
        for (uint32_t i = 0; i < BGZF_FRONT; i++) out[blk + i] = bgzf_front_byte(i, len);
        (void)bgzf_block_host(p, len, out.data() + blk + BGZF_FRONT);
        for (uint32_t i = 0; i < BGZF_BACK; i++) out[blk + BGZF_FRONT + len + i] = bgzf_back_byte(i, crc, len);
        return;
    }
    const uint32_t at = dfl_pass_host(L, len, true, L.misc[DFL_M_HEAD]);
    dfl_put(L.bits, at, L.code[256] & 0xffffu, L.code[256] >> 16);
    const uint32_t nbytes = (L.misc[DFL_M_BITS] + 7u) / 8u, block = DFL_HEAD + nbytes + BGZF_BACK;
    out.resize(blk + block);
    for (uint32_t i = 0; i < DFL_HEAD; i++) out[blk + i] = dfl_head_byte(i, block);
    memcpy(out.data() + blk + DFL_HEAD, L.bits, nbytes);
    for (uint32_t i = 0; i < BGZF_BACK; i++) out[blk + DFL_HEAD + nbytes + i] = bgzf_back_byte(i, crc, len);
}
/* src[0, n) in blocks at `level` onto the end of out, the EOF block behind them when with_eof; types: every block's BTYPE, or NULL;
 * counts: at level 1 every block's fixed and dynamic bit counts, two entries per block, or NULL */
inline void bgzf_compress_host(const void* src, size_t n, int with_eof, int level, std::vector<uint8_t>& out, std::vector<uint32_t>* types,
                               std::vector<uint32_t>* counts = nullptr) {
    if (level == 0) {
        bgzf_frame_host(src, n, with_eof, out);
        if (types) types->assign(bgzf_blocks(n), 0u);
        return;
    }
    std::vector<uint32_t> aligned((BGZF_PAYLOAD + BGZF_SRC_PAD) / 4u + 4u);
    uint8_t* const stage = (uint8_t*)(((uintptr_t)aligned.data() + 15u) & ~(uintptr_t)15u);
    std::vector<DeflateLds> lds(1);
    for (size_t at = 0; at < n; at += BGZF_PAYLOAD) {
        const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD ? n - at : BGZF_PAYLOAD);
        memcpy(stage, (const uint8_t*)src + at, len);
        uint32_t type = 0u, bits[2] = {0u, 0u};
        dfl_block_host(lds[0], stage, len, out, &type, bits);
        if (types) types->push_back(type);
        if (counts) counts->push_back(bits[0]), counts->push_back(bits[1]);
    }
    if (with_eof)
        for (uint32_t i = 0; i < BGZF_EOF; i++) out.push_back(bgzf_eof_byte(i));
}

#if defined(__HIPCC__)

/* One pass of the workgroup over the block's windows (EMIT: pass 2).  `at`: the bit of the first token; gives the bit behind the
 * last one, the same in every thread.  Every thread of the workgroup calls it. */
template <bool EMIT>
__device__ uint32_t dfl_pass(DeflateLds& L, uint32_t len, uint32_t at) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t i = t; i < DFL_PREV; i += BGZF_THREADS) L.prev[i] = 0u;
    L.wfirst[t] = DFL_NONE, L.wfirst[t + BGZF_THREADS] = DFL_NONE;
    __syncthreads();
    uint32_t x_before = 0u;
    bool hashed_before = false;
    for (uint32_t w = 0; DFL_WIN * w < len; w++) {
        const uint32_t p = DFL_WIN * w + t;
        const bool hashed = dfl_hashed(p, len);
        const uint32_t x = hashed ? dfl_get4(L.pay, p) : 0u;
        if (hashed) dfl_min(&L.wfirst[dfl_hash(x, 11u)], p);
        if (hashed_before) dfl_max(&L.prev[dfl_hash(x_before, 12u)], p - DFL_WIN + 1u);
        x_before = x, hashed_before = hashed;
        __syncthreads();
        const DflMatch m = p < len ? dfl_lookup(L, p, len, x) : DflMatch{0u, 0u};
        /* the slice's greedy parse: the wave walks its 64 positions; `at_lane` is uniform */
        bool starts = false;
        for (uint32_t at_lane = 0; at_lane < BGZF_SLICE;) {
            starts = starts || at_lane == lane;
            const uint32_t l = (uint32_t)__shfl((int)m.len, (int)at_lane);
            at_lane += l ? l : 1u;
        }
        starts = starts && p < len;
        const uint32_t b = p < len ? (L.pay[p >> 2] >> (8u * (p & 3u))) & 0xffu : 0u;
        if (!EMIT) {
            if (starts) dfl_count(L.hist, b, m);
            __syncthreads();
            L.wfirst[t] = DFL_NONE, L.wfirst[t + BGZF_THREADS] = DFL_NONE;
            __syncthreads();
            continue;
        }
        const DflBits o = starts ? dfl_token(L.code, b, m) : DflBits{0u, 0u};
        uint32_t sum = o.n; /* inclusive over the wave */
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)sum, off);
            if (lane >= (uint32_t)off) sum += up;
        }
        if (lane == 63u) L.misc[DFL_M_WAVE + wave] = sum;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t k = 0; k < BGZF_THREADS / 64u; k++) {
            const uint32_t s = L.misc[DFL_M_WAVE + k];
            before += k < wave ? s : 0u, all += s;
        }
        dfl_put(L.bits, at + before + sum - o.n, o.v, o.n);
        at += all;
        L.wfirst[t] = DFL_NONE, L.wfirst[t + BGZF_THREADS] = DFL_NONE;
        __syncthreads();
    }
    return at;
}

/* Workgroup b < nblocks encodes src[b * BGZF_PAYLOAD, ...) (the last block: what is left of n) into tmp + b * DFL_STRIDE and
 * gives the block's bytes in size[b]; src as in bgzf_frame_kernel.  Writes tmp[b * DFL_STRIDE, + size[b]) and nothing else. */
__global__ __launch_bounds__(BGZF_THREADS) void bgzf_deflate_kernel(const uint8_t* __restrict__ src, unsigned long long n, uint32_t nblocks,
                                                                   uint8_t* __restrict__ tmp, unsigned long long* __restrict__ size) {
    __shared__ DeflateLds L;
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    uint8_t* const blk = tmp + (size_t)b * DFL_STRIDE;
    const unsigned long long at = (unsigned long long)b * BGZF_PAYLOAD;
    const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD ? n - at : BGZF_PAYLOAD);
    const BgzfCut c = bgzf_cut(len);
    const uint32_t nbytes = bgzf_slice_bytes(c, t);
    /* the payload into LDS and its CRC, as bgzf_frame_kernel computes it; the table lies in the bit buffer */
    BgzfCrcTable& table = *reinterpret_cast<BgzfCrcTable*>(L.bits);
    (&table[0][0])[t] = (&bgzf_device_tables.t[0][0])[t];
    {
        const BgzfSlice v = bgzf_load_slice(src + at + BGZF_SLICE * t, nbytes);
        if (t < BGZF_SLICES) {
#pragma unroll
            for (uint32_t j = 0; j < BGZF_SLICE / 4u; j++) L.pay[BGZF_SLICE / 4u * t + j] = v.w[j];
        } else {
            L.pay[BGZF_PAYLOAD / 4u + (t - BGZF_SLICES)] = 0u;
        }
        if (t < DFL_SYMS) L.hist[t] = t == 256u ? 1u : 0u;
        __syncthreads();
        const uint32_t s = bgzf_crc_slice(table, bgzf_slice_init(t), v, nbytes);
        uint32_t front = t < c.last ? bgzf_mul(s, bgzf_device_tables.pow_slices[c.last - 1u - t]) : 0u;
        if (t == c.last) L.misc[DFL_M_LAST] = s;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) front ^= __shfl_xor(front, off);
        if ((t & 63u) == 0u) L.misc[DFL_M_FRONT + (t >> 6)] = front;
    }
    __syncthreads();
    if (t == 0u) {
        uint32_t all = 0u;
        for (uint32_t w = 0; w < BGZF_THREADS / 64u; w++) all ^= L.misc[DFL_M_FRONT + w];
        L.misc[DFL_M_CRC] = bgzf_crc_finish(all, bgzf_device_tables.pow_bytes[c.last_len], L.misc[DFL_M_LAST]);
    }
    for (uint32_t i = t; i < DFL_PAYW; i += BGZF_THREADS) L.bits[i] = 0u;
    (void)dfl_pass<false>(L, len, 0u); /* starts with a barrier of its own, behind its clearing */
    /* the codes: weights, dummies, ranks, lengths, choice */
    uint32_t* const bw = L.prev;
    if (t < DFL_SYMS) bw[DFL_B_W + t] = L.hist[t];
    __syncthreads();
    if (t == 0u) dfl_two_symbols(bw + DFL_B_W + DFL_NLL, DFL_ND);
    if (t < 2u) bw[DFL_B_USED + t] = 0u;
    __syncthreads();
    if (t < DFL_SYMS) {
        const uint32_t base = t < DFL_NLL ? 0u : DFL_NLL;
        const uint32_t r = dfl_rank(bw + DFL_B_W + base, base ? DFL_ND : DFL_NLL, t - base);
        if (r != DFL_NONE) bw[DFL_B_ORDER + base + r] = t - base, dfl_add(&bw[DFL_B_USED + (base ? 1u : 0u)], 1u);
    }
    __syncthreads();
    if (t == 0u || t == 64u) { /* one thread per alphabet, in two waves */
        const uint32_t base = t ? DFL_NLL : 0u;
        dfl_lengths(bw + DFL_B_W + base, bw + DFL_B_ORDER + base, bw[DFL_B_USED + (t ? 1u : 0u)], 15u, bw + DFL_B_A + base, bw + DFL_B_LEN + base,
                    t ? DFL_ND : DFL_NLL);
    }
    __syncthreads();
    if (t == 0u) dfl_choose(L, len);
    __syncthreads();
    const uint32_t type = L.misc[DFL_M_TYPE], crc = L.misc[DFL_M_CRC];
    if (type == 0u) { /* what bgzf_frame_kernel writes */
        BgzfSlice v = {};
        if (t < BGZF_SLICES) {
#pragma unroll
            for (uint32_t j = 0; j < BGZF_SLICE / 4u; j++) v.w[j] = L.pay[BGZF_SLICE / 4u * t + j];
        }
        if (t < BGZF_FRONT) blk[t] = bgzf_front_byte(t, len);
        bgzf_store_slice(blk + BGZF_FRONT + BGZF_SLICE * t, v, nbytes);
        if (t < BGZF_BACK) blk[BGZF_FRONT + len + t] = bgzf_back_byte(t, crc, len);
        if (t == 0u) size[b] = BGZF_FRONT + len + BGZF_BACK;
        return;
    }
    const uint32_t end = dfl_pass<true>(L, len, L.misc[DFL_M_HEAD]);
    if (t == 0u) dfl_put(L.bits, end, L.code[256] & 0xffffu, L.code[256] >> 16);
    __syncthreads();
    const uint32_t total = (L.misc[DFL_M_BITS] + 7u) / 8u, block = DFL_HEAD + total + BGZF_BACK;
    const uint32_t first = BGZF_SLICE * t, mine = first >= total ? 0u : total - first < BGZF_SLICE ? total - first : BGZF_SLICE;
    BgzfSlice v = {};
#pragma unroll
    for (uint32_t j = 0; j < BGZF_SLICE / 4u; j++)
        if (4u * j < mine) v.w[j] = L.bits[BGZF_SLICE / 4u * t + j];
    if (t < DFL_HEAD) blk[t] = dfl_head_byte(t, block);
    bgzf_store_slice(blk + DFL_HEAD + first, v, mine);
    if (t < BGZF_BACK) blk[DFL_HEAD + total + t] = bgzf_back_byte(t, crc, len);
    if (t == 0u) size[b] = block;
}

/* Workgroup b < nblocks moves block b (size[b] bytes at tmp + b * DFL_STRIDE, tmp 16-byte aligned) to dst + off[b]; workgroup
 * nblocks, when the grid has one, writes the EOF block at dst + off[nblocks].  Unaligned dwords go through sam_funnel
 * (bgzf_store_slice). */
__global__ __launch_bounds__(BGZF_THREADS) void bgzf_compact_kernel(const uint8_t* __restrict__ tmp, const unsigned long long* __restrict__ size,
                                                                   const unsigned long long* __restrict__ off, uint32_t nblocks,
                                                                   uint8_t* __restrict__ dst) {
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    if (b >= nblocks) {
        if (t < BGZF_EOF) dst[off[nblocks] + t] = bgzf_eof_byte(t);
        return;
    }
    const uint32_t total = (uint32_t)size[b];
    for (uint32_t first = BGZF_SLICE * t; first < total; first += BGZF_SLICE * BGZF_THREADS) { /* one round: a block has at most 1021 slices */
        const uint32_t mine = total - first < BGZF_SLICE ? total - first : BGZF_SLICE;
        const BgzfSlice v = bgzf_load_slice(tmp + (size_t)b * DFL_STRIDE + first, mine);
        bgzf_store_slice(dst + off[b] + first, v, mine);
    }
}

#endif /* __HIPCC__ */
