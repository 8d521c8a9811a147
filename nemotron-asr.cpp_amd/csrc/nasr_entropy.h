// nasr_entropy.h -- the arithmetic of the per-token entropy (engine option "token_entropy" = round(1000 alpha)), pure code without HIP so
// that the CPU suite compiles it with g++ (tests/test_entropy_math.py), like nasr_logprob.h, on whose parts it rests.  kernels_decode.hip
// includes it and runs the same functions on the device.
//
//   p = softmax of a row's 1025 RAW logits;   alpha = 1: H = -sum p ln p (Shannon);   alpha != 1: H = ln(sum p^alpha) / (1 - alpha) (Renyi), nats
//
// Beside each nasr_lp::Part (m, s) of a vocabulary slice the joint kernels keep ONE more f32, taken with the same slice maximum m:
//   alpha != 1   u = sum exp(alpha (x - m))            rescaled to a larger maximum M:  u exp(alpha (m - M))
//   alpha == 1   t = sum exp(x - m) (x - m)                                             (t + s (m - M)) exp(m - M)
// reduced in the orders of the parts: lane4, the xor-16 / xor-32 butterfly, ((w0, w1), w2), w3, and finish in ascending part index:
//   alpha != 1   H = (ln U - alpha ln S) / (1 - alpha)        alpha == 1   H = ln S - T / S
// An empty part (-inf, 0) carries 0 and contributes exactly 0 (0 * -inf is guarded).  A -inf logit inside a slice with a finite maximum
// contributes 0 as well; a lane whose four logits are all -inf is outside what nasr_lp::lane4 itself defines (its s is NaN) -- the joint's
// logits are finite.
// The 1 / (1 - alpha) of the Renyi form multiplies the rounding of ln U - alpha ln S, whose two terms come from f32 parts (relative error
// about 1e-7 each): at |1 - alpha| = 1e-3 that is 1e-4 nats (tests/test_entropy_math.py measures it), so the option refuses the band
// 900 < 1000 alpha < 1100 except 1000 itself (valid_milli), where the Shannon form has no such factor.
#pragma once
#include "nasr_logprob.h"

namespace nasr_ent {
using nasr_lp::Part;

constexpr int MILLI_MIN = 50, MILLI_MAX = 4000, MILLI_SHANNON = 1000, BAND_LO = 900, BAND_HI = 1100;
// 0 = off; 50 .. 4000 without the band around 1000 whose amplification exceeds the value's own precision (1000 itself is Shannon)
NASR_LP_HD bool valid_milli(int v) { return v == 0 || v == MILLI_SHANNON || (v >= MILLI_MIN && v <= MILLI_MAX && (v <= BAND_LO || v >= BAND_HI)); }
NASR_LP_HD float alpha_of(int milli) { return (float)milli / 1000.0f; }
NASR_LP_HD bool shannon(float alpha) { return alpha == 1.0f; }
NASR_LP_HD float ln_vocab() { return 6.93244789f; }                     // (float) ln 1025: the largest entropy of 1025 outcomes

// one logit's term against the slice maximum m (finite)
NASR_LP_HD float term(float x, float m, float alpha) {
    const float d = x - m;
    if (d == nasr_lp::neg_inf()) return 0.0f;
    return shannon(alpha) ? expf(d) * d : expf(alpha * d);
}
// the first n_valid (0 .. 4) of a lane's four logits, m = nasr_lp::lane4's maximum of them; added in ascending vocab order
NASR_LP_HD float lane4(float x0, float x1, float x2, float x3, int n_valid, float m, float alpha) {
    if (n_valid <= 0 || m == nasr_lp::neg_inf()) return 0.0f;
    float e = term(x0, m, alpha);
    if (n_valid > 1) e += term(x1, m, alpha);
    if (n_valid > 2) e += term(x2, m, alpha);
    if (n_valid > 3) e += term(x3, m, alpha);
    return e;
}
// part a with its extra ea, rescaled to the maximum m >= a.m (m finite)
NASR_LP_HD float rescaled(Part a, float ea, float m, float alpha) {
    if (a.m == nasr_lp::neg_inf()) return 0.0f;
    const float d = a.m - m;
    return shannon(alpha) ? (ea + a.s * d) * expf(d) : ea * expf(alpha * d);
}
// the extra of nasr_lp::merge(a, b), whose maximum is m; symmetric in (a, ea) / (b, eb): both lanes of a butterfly step get the same bits
NASR_LP_HD float merge(Part a, float ea, Part b, float eb, float m, float alpha) {
    if (m == nasr_lp::neg_inf()) return 0.0f;
    return rescaled(a, ea, m, alpha) + rescaled(b, eb, m, alpha);
}
// a part and its extra
struct EPart { Part p; float e; };
NASR_LP_HD EPart emerge(EPart a, EPart b, float alpha) {
    EPart r;
    r.p = nasr_lp::merge(a.p, b.p);
    r.e = merge(a.p, a.e, b.p, b.e, r.p.m, alpha);
    return r;
}
NASR_LP_HD EPart elane4(float x0, float x1, float x2, float x3, int n_valid, float alpha) {
    EPart r;
    r.p = nasr_lp::lane4(x0, x1, x2, x3, n_valid);
    r.e = lane4(x0, x1, x2, x3, n_valid, r.p.m, alpha);
    return r;
}
NASR_LP_HD EPart tile16(EPart q0, EPart q1, EPart q2, EPart q3, float alpha) { return emerge(emerge(q0, q1, alpha), emerge(q2, q3, alpha), alpha); }
NASR_LP_HD EPart wg64(EPart w0, EPart w1, EPart w2, EPart w3, float alpha) { return emerge(emerge(emerge(w0, w1, alpha), w2, alpha), w3, alpha); }

#if defined(__HIPCC__)
// nasr_lp::tile_part_wave with the extra beside it.  The part it carries serves the extra only: the kernels store the part they formed
// without this function, from code of its own (kernels_decode.hip, ent_opaque) -- the two may differ in the last bit of s where the
// compiler contracts a * b + c * d differently, which moves H by 1e-7 at most
__device__ __forceinline__ EPart tile_wave(float x0, float x1, float x2, float x3, int v0, float alpha) {
    EPart a = elane4(x0, x1, x2, x3, nasr_lp::lane_valid(v0), alpha), b;
    b.p.m = __shfl_xor(a.p.m, 16); b.p.s = __shfl_xor(a.p.s, 16); b.e = __shfl_xor(a.e, 16);
    a = emerge(a, b, alpha);
    b.p.m = __shfl_xor(a.p.m, 32); b.p.s = __shfl_xor(a.p.s, 32); b.e = __shfl_xor(a.e, 32);
    return emerge(a, b, alpha);
}
#endif

// H of a row from its parts and their extras, merged in ascending part index.  The sums, the logarithms and the division are taken in f64
// and the result is rounded to f32 once, as nasr_lp::blank_lp does and for the same reason: many parts contribute terms of the same size,
// and ln U - alpha ln S is a difference of two close numbers.  One thread does this once per emitted token, at most 65 terms
NASR_LP_HD float finish(const Part *parts, const float *ext, int n_parts, float alpha) {
    float m = nasr_lp::neg_inf();
    for (int i = 0; i < n_parts; i++) m = fmaxf(m, parts[i].m);
    double S = 0.0, E = 0.0;
    for (int i = 0; i < n_parts; i++) {
        if (parts[i].m == nasr_lp::neg_inf()) continue;
        S += (double)(parts[i].s * expf(parts[i].m - m));
        E += (double)rescaled(parts[i], ext[i], m, alpha);
    }
    const double a = (double)alpha;
    double h = shannon(alpha) ? log(S) - E / S : (log(E) - a * log(S)) / (1.0 - a);
    if (h < 0.0) h = 0.0;
    if (h > (double)ln_vocab()) h = (double)ln_vocab();
    return (float)h;
}

// host restatement of what a kernel leaves in the scratch for one row: `width` = nasr_lp::TILE_W or WG_W, parts[n] and ext[n], n = parts_of_width(width)
NASR_LP_HD EPart tile_of(const float *logits, int nt, float alpha) {
    EPart q[4];
    for (int k = 0; k < 4; k++) {
        const int v0 = nt * nasr_lp::TILE_W + k * 4, n = nasr_lp::lane_valid(v0);
        q[k] = elane4(n > 0 ? logits[v0] : 0.0f, n > 1 ? logits[v0 + 1] : 0.0f, n > 2 ? logits[v0 + 2] : 0.0f, n > 3 ? logits[v0 + 3] : 0.0f, n, alpha);
    }
    return tile16(q[0], q[1], q[2], q[3], alpha);
}
NASR_LP_HD void row_parts(const float *logits, int width, float alpha, Part *parts, float *ext) {
    const int n = nasr_lp::parts_of_width(width);
    for (int p = 0; p < n; p++) {
        const EPart r = width == nasr_lp::TILE_W ? tile_of(logits, p, alpha)
                                                 : wg64(tile_of(logits, 4 * p, alpha), tile_of(logits, 4 * p + 1, alpha), tile_of(logits, 4 * p + 2, alpha), tile_of(logits, 4 * p + 3, alpha), alpha);
        parts[p] = r.p; ext[p] = r.e;
    }
}

}  // namespace nasr_ent
