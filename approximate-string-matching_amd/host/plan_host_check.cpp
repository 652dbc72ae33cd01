// Stand-alone driver of the aligner and filter dispatch (csrc/asm_plan.h) on the CPU: reads one query per line from standard input and
// prints every field of the plan it gets, one line per query (tests/test_plan_host.py).  Plain g++, no HIP.
//   A aligner k x o e alignment_type leap_mode n maxlen w4 mixed hint switches   -> align_plan; switches: bit q = the q-th of AlignSwitches
//   C aligner k x o e alignment_type leap_mode p_match p_mismatch p_indel maxlen -> check_params_rule: code and message
//   E T ed_mode n maxlen                                                         -> simd_ed_plan
//   F gap x o e n maxlen                                                         -> simd_ed_affine_plan
#include <stdio.h>
#include <string.h>

#include "../../include/asm_mi355x.h"
#include "../csrc/asm_affine.h"
#include "../csrc/asm_plan.h"

static const char* const FAMILY[ALIGN_FAMILIES] = {"GREEDY_FAST", "GREEDY_PERSIST", "GREEDY_GROUP", "GREEDY_WAVE", "GREEDY_WAVE2", "GREEDY_WIDE",
                                                   "LEAP_UNIT", "LEAP_GENERAL", "LEAP_QUAD", "LEAP_WIDE", "NW_UNIT_FULL", "NW_BANDED",
                                                   "NW_BANDED_BYLEN", "NW_PAIR2", "NW_WFA", "NW_AFFINE_FULL"};

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        asm_params p;
        memset(&p, 0, sizeof p);
        p.p_match = 0.80, p.p_mismatch = 0.20 / 3, p.p_indel = 0.40 / 3;
        int aligner, k, x, o, e, at, lm, maxlen, w4, mixed, hint, T, mode, gap;
        long long n;
        unsigned sw;
        if (sscanf(line, "A %d %d %d %d %d %d %d %lld %d %d %d %d %u", &aligner, &k, &x, &o, &e, &at, &lm, &n, &maxlen, &w4, &mixed, &hint, &sw) == 13) {
            p.k = k, p.x = x, p.o = o, p.e = e, p.alignment_type = at, p.leap_mode = lm;
            const AlignSwitches s = {(sw & 1) != 0, (sw & 2) != 0, (sw & 4) != 0, (sw & 8) != 0, (sw & 16) != 0, (sw & 32) != 0, (sw & 64) != 0, (sw & 128) != 0};
            const AlignPlan pl = align_plan(aligner, p, AlignShape{(int64_t)n, maxlen, w4, mixed != 0}, s, hint != 0);
            if (pl.family < 0 || pl.family >= ALIGN_FAMILIES) return 2;
            printf("%s k=%d words=%d window=%d entry=%d gm=%d gi=%d unit=%d hinted=%d waves=%d sort=%d sort_div=%d oct_entry=%d oct_lds=%zu block=%u "
                   "grid=%lld grid_rule=%d grid_arg=%d lds=%zu\n",
                   FAMILY[pl.family], pl.k, pl.words, pl.window, pl.entry, pl.gm, pl.gi, (int)pl.unit, (int)pl.hinted, pl.waves, (int)pl.sort,
                   pl.sort_div, pl.oct_entry, pl.oct_lds, pl.block, (long long)pl.grid, pl.grid_rule, pl.grid_arg, pl.lds);
        } else if (sscanf(line, "C %d %d %d %d %d %d %d %lf %lf %lf %d", &aligner, &k, &x, &o, &e, &at, &lm, &p.p_match, &p.p_mismatch, &p.p_indel,
                          &maxlen) == 11) {
            p.k = k, p.x = x, p.o = o, p.e = e, p.alignment_type = at, p.leap_mode = lm;
            const ParamVerdict v = check_params_rule(aligner, &p, maxlen);
            printf("%d %s\n", v.code, v.msg ? v.msg : "");
        } else if (sscanf(line, "E %d %d %lld %d", &T, &mode, &n, &maxlen) == 4) {
            const SimdEdPlan pl = simd_ed_plan(T, mode, (int64_t)n, maxlen);
            printf("reg_t=%d words=%d block=%u grid=%lld lds=%zu\n", pl.reg_t, pl.words, pl.block, (long long)pl.grid, pl.lds);
        } else if (sscanf(line, "F %d %d %d %d %lld %d", &gap, &x, &o, &e, &n, &maxlen) == 6) {
            const SimdEdAffinePlan pl = simd_ed_affine_plan(gap, x, o, e, (int64_t)n, maxlen);
            printf("refused=%d quad=%d block=%u grid=%lld lds=%zu gm=%d gi=%d\n", (int)pl.refused, (int)pl.quad, pl.block, (long long)pl.grid, pl.lds,
                   pl.gm, pl.gi);
        } else {
            fprintf(stderr, "plan_host_check: bad query: %s", line);
            return 1;
        }
    }
    return 0;
}
