// Closed forms of a group's matrix element (host side, no device code): the class of a group from its masks alone, and
// the sign tables eloc_kernel2's drain reads instead of walking the group's terms.
//
// A group is the terms that share one flip mask xy; its matrix element for a key is  h = sum_t c_t (-1)^popc(key & yz_t).
// With one of the group's own masks as reference R,  parity(key & yz_t) = parity(key & R) ^ parity(key & (yz_t ^ R)), and
//   class D (4 flipped bits, every yz_t ^ R inside xy):  h = (-1)^popc(key & R) * T[the key's 4 bits at the flipped positions]
//   class S (2 flipped bits, every yz_t ^ R has at most one bit outside xy, its "spectator"):
//            h = (-1)^popc(key & R) * sum_s B[s][the key's 2 bits at the flipped positions][the key's bits SEG_BITS*s ...]
//            a term belongs to the segment s its spectator lies in (segment 0 without one)
//   class L: anything else — the term loop.
// Every table entry is the sum of its terms in ascending t, from 0.0, in plain double adds: a D element is the very double
// the loop produces (times +-1, exactly); an S element is the same terms in another association.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace naqs {
namespace closed {

constexpr int SEG_BITS = 6;                    // key bits per S segment: 64 entries per (pattern, segment)
constexpr int SEG_SIZE = 1 << SEG_BITS;
constexpr int MAX_UNITS = 1 << 12;             // the word's table-unit field: an S table begins at a multiple of SEG_SIZE doubles
constexpr int MAX_CLASSIFY_TERMS = 4096;       // the choice of R is quadratic in a group's terms; longer groups stay class L
enum { CLASS_L = 0, CLASS_D = 1, CLASS_S = 2 };

struct Group {
    int cls = CLASS_L;
    uint64_t R = 0;
    int pos[4] = {0, 0, 0, 0};                 // flipped positions, ascending
};

inline int popc64(uint64_t v) { return __builtin_popcountll(v); }
inline int n_segments(int n_qubits) { return (n_qubits + SEG_BITS - 1) / SEG_BITS; }
inline size_t d_table_doubles() { return 16; }
inline size_t s_table_doubles(int nseg) { return (size_t)4 * (size_t)nseg * SEG_SIZE; }

// the pattern's bits put back at the flipped positions
inline uint64_t deposit(const Group &g, int pattern, int nflip) {
    uint64_t m = 0;
    for (int i = 0; i < nflip; ++i)
        if ((pattern >> i) & 1) m |= 1ull << g.pos[i];
    return m;
}

// R = the first term that minimises the largest popc((yz_t ^ R) & ~xy); D: 4 flipped bits and that maximum 0, S: 2 and <= 1
inline Group classify(uint64_t xy, const uint64_t *yz, int n) {
    Group g;
    const int nflip = popc64(xy);
    if ((nflip != 2 && nflip != 4) || n <= 0 || n > MAX_CLASSIFY_TERMS) return g;
    int best = 1 << 30, ref = 0;
    for (int r = 0; r < n; ++r) {
        int worst = 0;
        for (int t = 0; t < n; ++t) worst = std::max(worst, popc64((yz[t] ^ yz[r]) & ~xy));
        if (worst < best) { best = worst; ref = r; }
    }
    if (!((nflip == 4 && best == 0) || (nflip == 2 && best <= 1))) return g;
    g.cls = nflip == 4 ? CLASS_D : CLASS_S;
    g.R = yz[ref];
    for (int q = 0, k = 0; q < 64; ++q)
        if ((xy >> q) & 1) g.pos[k++] = q;
    return g;
}

inline uint32_t d_word(const Group &g) {
    return (uint32_t)g.pos[0] | (uint32_t)g.pos[1] << 6 | (uint32_t)g.pos[2] << 12 | (uint32_t)g.pos[3] << 18;
}
inline uint32_t s_word(const Group &g, int unit) {
    return (uint32_t)g.pos[0] | (uint32_t)g.pos[1] << 6 | (uint32_t)unit << 12;
}

// T[16]
inline void build_d(const Group &g, const uint64_t *yz, const double *c, int n, double *T) {
    for (int p = 0; p < 16; ++p) {
        const uint64_t dep = deposit(g, p, 4);
        double acc = 0.0;
        for (int t = 0; t < n; ++t) acc += (popc64(dep & (yz[t] ^ g.R)) & 1) ? -c[t] : c[t];
        T[p] = acc;
    }
}

// B[nseg][4][SEG_SIZE]
inline void build_s(const Group &g, uint64_t xy, const uint64_t *yz, const double *c, int n, int nseg, double *B) {
    for (int p = 0; p < 4; ++p) {
        const uint64_t dep = deposit(g, p, 2);
        for (int s = 0; s < nseg; ++s)
            for (int v = 0; v < SEG_SIZE; ++v) {
                double acc = 0.0;
                for (int t = 0; t < n; ++t) {
                    const uint64_t d = yz[t] ^ g.R, sp = d & ~xy;
                    const int r = sp ? __builtin_ctzll(sp) : 0;
                    if (r / SEG_BITS != s) continue;
                    const int par = popc64(dep & d) + (sp ? (v >> (r - s * SEG_BITS)) & 1 : 0);
                    acc += (par & 1) ? -c[t] : c[t];
                }
                B[((size_t)s * 4 + p) * SEG_SIZE + v] = acc;
            }
    }
}

}  // namespace closed
}  // namespace naqs
