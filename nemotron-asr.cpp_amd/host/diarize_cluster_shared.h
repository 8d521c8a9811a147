// diarize_cluster_shared.h -- what the two NME-SC paths must agree on bit for bit: the host path (diarize_cluster_amd.cpp) and
// the device path (csrc/nasr_diar_cluster.hip) differ in who computes the affinity, the neighbour graphs and the Laplacians'
// eigen-pairs; the candidate p values, the gap-ratio rule, the connectivity check, the early return and k-means are this one
// text.  Host-only, header-only (the line numbers cite the reference's src/diarize_cluster.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "diarize_cluster_amd.h"

namespace nmesc_shared {

constexpr float  AFF_EPS = 3.5e-4f;      // src/diarize_cluster.cpp:31
constexpr double EIG_EPS = 1e-10;        // :32
constexpr int    MIN_P   = 2;            // :33

// inputs this small are one cluster (:325-331)
inline bool early_return(int N, const nmesc_cfg &cfg, nmesc_result &res) {
    if (N > cfg.min_samples_for_nmesc) return false;
    res.est_num_speakers = cfg.oracle_num_speakers > 0 ? cfg.oracle_num_speakers : 1;
    res.labels.assign(N, 0);
    res.p_hat = N - 1;
    return true;
}

// the NME analysis runs on every ratio-th row / column when N exceeds nme_mat_size (:150-166)
inline int subsample_ratio(int N, const nmesc_cfg &cfg) { return std::max(1, (int)std::ceil((double)N / (double)cfg.nme_mat_size)); }

// candidate p values: `steps` points from 1 to max(2, floor(N * max_rp_threshold)), truncated to int, duplicates removed (:168-190)
inline std::vector<int> candidate_p(int N, float max_rp_threshold, int sparse_search_volume) {
    const int max_p = std::max(MIN_P, (int)std::floor((double)N * (double)max_rp_threshold));
    const int steps = std::min(max_p, std::max(2, sparse_search_volume));
    std::vector<int> out;
    for (int i = 0; i < steps; i++) {
        const int p = (int)(1.0 + (double)i * ((double)max_p - 1.0) / (double)std::max(1, steps - 1));
        if (std::find(out.begin(), out.end(), p) == out.end()) out.push_back(p);
    }
    return out;
}

// the p values the analysis of an Ns x Ns (sub)matrix tries
inline std::vector<int> analysis_candidates(int Ns, const nmesc_cfg &cfg) {
    return cfg.fixed_thres > 0.0f ? std::vector<int>(1, std::max(MIN_P, (int)std::floor((double)Ns * (double)cfg.fixed_thres)))
                                  : candidate_p(Ns, cfg.max_rp_threshold, cfg.sparse_search_volume);
}

// how many of the smallest Laplacian eigenvalues the gap rule reads (besides the largest)
inline int gap_values(int N, int max_num_speakers) { return std::min(N - 1, max_num_speakers) + 1; }

// g_p = (p / N) / (largest gap among the first K eigenvalues, normalised by the largest eigenvalue) (:199-214).
// lam_low: the gap_values(N, max_num_speakers) smallest eigenvalues, ascending
struct GapRatio { double g_p; int n_spk; };
inline GapRatio gap_rule(const double *lam_low, double lam_max, int N, int p, int max_num_speakers) {
    const int K = std::min(N - 1, max_num_speakers);
    int best = 0;
    for (int i = 1; i < K; i++)
        if (lam_low[i + 1] - lam_low[i] > lam_low[best + 1] - lam_low[best]) best = i;
    const double gap = K > 0 ? (lam_low[best + 1] - lam_low[best]) / (lam_max + EIG_EPS) : 0.0;
    return {((double)p / (double)N) / (gap + EIG_EPS), best + 1};
}

// the analysis' choice among the candidates: the first p with the smallest ratio
struct Choice { double g = std::numeric_limits<double>::infinity(); int p = 0, est = 1; };
inline void consider(Choice &c, const GapRatio &gr, int p) {
    if (gr.g_p < c.g) { c.g = gr.g_p; c.p = p; c.est = gr.n_spk; }
}

// is the graph one component?  each(v, f) calls f(j) for every neighbour j of v (either direction of the symmetrised graph)
template <class Each>
inline bool connected(int N, Each &&each) {
    if (N == 0) return true;
    std::vector<char> seen(N, 0);
    std::vector<int> stack(1, 0);
    seen[0] = 1;
    int reached = 1;
    while (!stack.empty()) {
        const int v = stack.back();
        stack.pop_back();
        each(v, [&](int j) { if (!seen[j]) { seen[j] = 1; reached++; stack.push_back(j); } });
    }
    return reached == N;
}

inline int cluster_count(int est, const nmesc_cfg &cfg) {
    const int n = cfg.oracle_num_speakers > 0 ? cfg.oracle_num_speakers : est;
    return std::max(1, std::min(n, cfg.max_num_speakers));
}

struct Rng {                              // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// k-means++ seeding, Lloyd iterations until the inertia moves by less than 1e-4 (:221-307)
inline double kmeans(const std::vector<float> &X, int N, int D, int K, Rng &rng, std::vector<int> &labels) {
    labels.assign(N, 0);
    if (K <= 1) return 0.0;
    auto dist2 = [&](const float *a, const float *b) { double s = 0.0; for (int d = 0; d < D; d++) { const double t = (double)a[d] - b[d]; s += t * t; } return s; };
    std::vector<float> centre((size_t)K * D);
    std::vector<double> near(N, std::numeric_limits<double>::infinity());
    int pick = (int)(rng.next() % (uint64_t)N);
    for (int k = 0; k < K; k++) {
        std::copy_n(&X[(size_t)pick * D], D, &centre[(size_t)k * D]);
        if (k + 1 == K) break;
        double total = 0.0;
        for (int i = 0; i < N; i++) { near[i] = std::min(near[i], dist2(&X[(size_t)i * D], &centre[(size_t)k * D])); total += near[i]; }
        if (total <= 0.0) { pick = (int)(rng.next() % (uint64_t)N); continue; }
        double target = rng.uniform() * total, cum = 0.0;
        pick = N - 1;
        for (int i = 0; i < N; i++) { cum += near[i]; if (cum >= target) { pick = i; break; } }
    }
    std::vector<double> sum((size_t)K * D);
    std::vector<int> count(K);
    double prev = std::numeric_limits<double>::infinity();
    for (int it = 0; it < 300; it++) {
        std::fill(sum.begin(), sum.end(), 0.0);
        std::fill(count.begin(), count.end(), 0);
        double inertia = 0.0;
        for (int i = 0; i < N; i++) {
            int best = 0;
            double bd = std::numeric_limits<double>::infinity();
            for (int k = 0; k < K; k++) { const double dd = dist2(&X[(size_t)i * D], &centre[(size_t)k * D]); if (dd < bd) { bd = dd; best = k; } }
            labels[i] = best;
            inertia += bd;
            count[best]++;
            for (int d = 0; d < D; d++) sum[(size_t)best * D + d] += X[(size_t)i * D + d];
        }
        for (int k = 0; k < K; k++)
            if (count[k] > 0) for (int d = 0; d < D; d++) centre[(size_t)k * D + d] = (float)(sum[(size_t)k * D + d] / count[k]);
        if (std::fabs(prev - inertia) < 1e-4) break;
        prev = inertia;
    }
    return prev;
}

// the spectral embedding (row i = the n_clusters eigenvector entries of sample i) -> labels of the best of the k-means trials
inline std::vector<int> kmeans_trials(const std::vector<float> &se, int N, int n_clusters, const nmesc_cfg &cfg) {
    Rng rng{cfg.kmeans_seed};
    double best_inertia = std::numeric_limits<double>::infinity();
    std::vector<int> labels, best;
    for (int t = 0; t < std::max(1, cfg.kmeans_random_trials); t++) {
        const double inertia = kmeans(se, N, n_clusters, n_clusters, rng, labels);
        if (inertia < best_inertia) { best_inertia = inertia; best = labels; }
    }
    return best;
}

}  // namespace nmesc_shared
