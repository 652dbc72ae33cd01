// Test-only brute force of asm_map_pairs' mate rescue (docs/design/mapper.md, "Paired-end reads"): over the ends j in
// [jlo, jhi] of one sequence T (clipped to [1, len]), a plain semi-global DP under the mapper's byte rule gives
// D(j) = min_i Lev(q_s, T[i, j)); the rescued locus is the smallest (D(j), j) with D(j) <= R and D(j) < m, and its i is the
// largest start with Lev(q_s, T[i, j)) = D(j) (reversed DP).  Starts before jlo - m - R are left out: an alignment of m read
// bytes with at most R edits spans at least m - R text bytes, so no such start reaches D <= R at an end >= jlo.
//   map_bf_rescue(t, len, read, m, s, jlo, jhi, R, out) -> 1 and out = {s, i, j, d}, or 0 when nothing qualifies.
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

static bool is_base(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
static char upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
static char comp(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
static int sub(char a, char b) { return (a == b && is_base(a)) ? 0 : 1; }

/* the largest start i with Lev(q, T[i, j)) = d: a plain DP over the reversed strings, the first length reaching d */
static int64_t start_of(const std::string& q, const char* t, int64_t j, int d) {
    const int m = (int)q.size();
    const int64_t lo = std::max<int64_t>(0, j - m - d);
    std::vector<int> P(m + 1), Q(m + 1);
    for (int i = 0; i <= m; i++) P[i] = i;
    for (int64_t L = 1; L <= j - lo; L++) {
        const char tc = upper(t[j - L]);
        Q[0] = (int)L;
        for (int i = 1; i <= m; i++) Q[i] = std::min({P[i - 1] + sub(q[m - i], tc), P[i] + 1, Q[i - 1] + 1});
        std::swap(P, Q);
        if (P[m] == d) return j - L;
    }
    return -1;
}

extern "C" int map_bf_rescue(const char* t, int64_t len, const char* read, int m, int s, int64_t jlo, int64_t jhi, int R, int32_t* out) {
    std::string q(read, read + m);
    for (char& c : q) c = upper(c);
    if (s) {
        std::reverse(q.begin(), q.end());
        for (char& c : q) c = comp(c);
    }
    jlo = std::max<int64_t>(jlo, 1), jhi = std::min<int64_t>(jhi, len);
    if (jlo > jhi) return 0;
    const int64_t c0 = std::max<int64_t>(0, jlo - m - R);
    std::vector<int> C(m + 1), N(m + 1);
    for (int i = 0; i <= m; i++) C[i] = i;
    int best = R + 1;
    int64_t best_j = 0;
    for (int64_t c = c0; c < jhi; c++) {
        const char tc = upper(t[c]);
        N[0] = 0;
        for (int i = 1; i <= m; i++) N[i] = std::min({C[i - 1] + sub(q[i - 1], tc), C[i] + 1, N[i - 1] + 1});
        std::swap(C, N);
        const int64_t j = c + 1;
        if (j >= jlo && C[m] < best && C[m] < m) best = C[m], best_j = j;
    }
    if (best > R) return 0;
    out[0] = s, out[1] = (int32_t)start_of(q, t, best_j, best), out[2] = (int32_t)best_j, out[3] = best;
    return 1;
}
