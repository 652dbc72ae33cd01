// The pair cut of two FASTQ texts whose line counts are known (docs/design/mapper.md, "Compressed input for pairs"): how many whole
// pairs the two texts hold together, which newline ends the last of them in each text, and what each text says of its file's end.
// The rule only: no HIP and nothing of the library, so that the kernel (pair_cut_kernel, asm_map_pairs_file.h) and the host check
// (host/bgzf_pair_fill_host_check.cpp) run the same code; finding the byte behind a newline is the caller's (bisection and ballots
// on the device, a scan on the host).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define PCUT_HD __host__ __device__ __forceinline__
#else
#define PCUT_HD static inline
#endif

struct PairCutText {
    unsigned long long counted; /* the newlines of text[0, nbytes) */
    unsigned long long nbytes;
    uint32_t open_end; /* the text reaches its file's end and does not end in a newline: it gets one at text[nbytes] */
    uint32_t pad;
};
struct PairCutFile {
    unsigned long long lines; /* the text's newlines, an appended one included */
    unsigned long long cut;   /* the bytes of its first `pairs` records */
    uint32_t appended;        /* a newline was appended behind the text */
    uint32_t extra_lines;     /* the lines behind the text's last whole record: at the file's end, a truncated record */
    uint32_t more;            /* the text holds whole records beyond `pairs` */
    uint32_t pad;
};
struct PairCutOut {
    unsigned long long pairs; /* R = min(lines1 / 4, lines2 / 4) */
    PairCutFile f[2];
};

enum { PAIR_CUT_SET = 0, PAIR_CUT_FIND = 1 };
/* Everything of *o but the cuts that have to be looked for: how[x] == PAIR_CUT_SET: o->f[x].cut is set (0 for no pair, nbytes + 1
 * when the appended newline closes the last pair's record); PAIR_CUT_FIND: it is the byte behind newline 4 * pairs - 1 (from 0) of
 * text x, which is one of its `counted`. */
PCUT_HD void pair_cut_plan(const PairCutText t[2], PairCutOut* o, uint32_t how[2]) {
    for (int x = 0; x < 2; x++) {
        o->f[x].appended = t[x].open_end && t[x].nbytes > 0 ? 1u : 0u;
        o->f[x].lines = t[x].counted + o->f[x].appended;
        o->f[x].extra_lines = (uint32_t)(o->f[x].lines & 3u);
        o->f[x].pad = 0u;
    }
    const unsigned long long r0 = o->f[0].lines / 4u, r1 = o->f[1].lines / 4u, pairs = r0 < r1 ? r0 : r1;
    o->pairs = pairs;
    for (int x = 0; x < 2; x++) {
        o->f[x].more = o->f[x].lines / 4u > pairs ? 1u : 0u;
        how[x] = PAIR_CUT_SET;
        if (pairs == 0u) o->f[x].cut = 0u;
        else if (4u * pairs > t[x].counted) o->f[x].cut = t[x].nbytes + 1u;
        else o->f[x].cut = 0u, how[x] = PAIR_CUT_FIND;
    }
}
