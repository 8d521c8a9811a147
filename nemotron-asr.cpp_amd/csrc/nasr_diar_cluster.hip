// nasr_diar_cluster.hip -- NME-SC speaker clustering of the diarization side-car on the device: scratch, launch sequences and the host
// decisions between them.  Replaces the compute of host/diarize_cluster_amd.cpp (the reference's src/diarize_cluster.cpp): affinity,
// neighbour graphs, Laplacians and their eigen-pairs are kernels (kernels_cluster.hip); the candidate p values, the gap rule, the
// connectivity check and k-means are the host path's own text (host/diarize_cluster_shared.h).
#include "nasr_internal.h"
#include "nasr_diar_cluster.h"
#include "../host/diarize_cluster_shared.h"

#include <cstdarg>
#include <cstdio>
#include <vector>

namespace nasr {
namespace {

int failf(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return set_error(buf);
}
#define CCHK(x)                                                                                                  \
    do {                                                                                                         \
        hipError_t e_ = (x);                                                                                     \
        if (e_ != hipSuccess) return failf("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// grow-on-demand scratch: whatever the stream still does with the old buffer finishes before it is freed
int ensure(hipStream_t st, ClBuf &b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    CCHK(hipStreamSynchronize(st));
    if (b.p) CCHK(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    CCHK(hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return 0;
}
int prepare(ClusterState &cs) {
    if (cs.ready) return 0;
    init_cluster_kernel_attributes();
    for (auto &e : cs.ev) CCHK(hipEventCreate(&e));
    cs.ready = true;
    return 0;
}
int stage_begin(ClusterState &cs, hipStream_t st) {
    CCHK(hipEventRecord(cs.ev[0], st));
    return 0;
}
// the stage's launches are done when this returns; its device time is added to the call's
int stage_end(ClusterState &cs, hipStream_t st, int stage) {
    CCHK(hipEventRecord(cs.ev[1], st));
    CCHK(hipStreamSynchronize(st));
    CCHK(hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, cs.ev[0], cs.ev[1]) == hipSuccess) cs.ms[stage] += ms;
    return 0;
}
template <typename Tp>
int download(hipStream_t st, Tp *host, const void *dev, size_t n) {
    CCHK(hipMemcpyAsync(host, dev, n * sizeof(Tp), hipMemcpyDeviceToHost, st));
    CCHK(hipStreamSynchronize(st));
    return 0;
}

// emb (host) -> cs.aff [N][N] on the device
int affinity_device(ClusterState &cs, hipStream_t st, const float *emb, int N, int D) {
    const size_t nd = (size_t)N * D;
    if (ensure(st, cs.emb, nd * sizeof(float)) || ensure(st, cs.unit, (size_t)N * cl_pad4(D) * sizeof(float)) ||
        ensure(st, cs.aff, (size_t)N * N * sizeof(float)) || ensure(st, cs.minmax, 2 * sizeof(unsigned)))
        return -1;
    CCHK(hipMemcpyAsync(cs.emb.p, emb, nd * sizeof(float), hipMemcpyHostToDevice, st));
    if (stage_begin(cs, st)) return -1;
    launch_cl_affinity((const float *)cs.emb.p, N, D, (float *)cs.unit.p, (unsigned *)cs.minmax.p, (float *)cs.aff.p, st);
    return stage_end(cs, st, CL_AFFINITY);
}

// the neighbour bitmaps of the C candidates ps of the n x n matrix that is every stride-th row / column of cs.aff [ld][ld] -> cs.keep,
// then (lap) their Laplacians -> cs.mat and / or (graph) the graphs -> cs.graph
int graphs_device(ClusterState &cs, hipStream_t st, int ld, int stride, int n, const int *ps, int C, bool lap, bool graph) {
    const size_t nn = (size_t)n * n;
    if (ensure(st, cs.plist, (size_t)C * sizeof(int)) || ensure(st, cs.keep, (size_t)C * n * cl_keep_words(n) * sizeof(unsigned)) ||
        (lap && ensure(st, cs.mat, (size_t)C * nn * sizeof(double))) || (graph && ensure(st, cs.graph, (size_t)C * nn * sizeof(float))))
        return -1;
    CCHK(hipMemcpyAsync(cs.plist.p, ps, (size_t)C * sizeof(int), hipMemcpyHostToDevice, st));
    if (stage_begin(cs, st)) return -1;
    launch_cl_select((const float *)cs.aff.p, ld, stride, n, (const int *)cs.plist.p, C, (unsigned *)cs.keep.p, st);
    if (lap || graph) launch_cl_laplacian((const unsigned *)cs.keep.p, n, C, lap ? (double *)cs.mat.p : nullptr, graph ? (float *)cs.graph.p : nullptr, st);
    return stage_end(cs, st, CL_GRAPH);           // also: ps may go out of scope
}

// cs.mat [batch][n][n] (destroyed) -> vals [batch][k_low + 1]: the k_low smallest eigenvalues and the largest of every matrix;
// k_vec > 0: the eigenvectors of the k_vec smallest of matrix 0 -> vectors [n][k_vec] (host)
int eigen_device(ClusterState &cs, hipStream_t st, int n, int batch, int k_low, std::vector<double> &vals, int k_vec, double *vectors) {
    const size_t tri = cl_tri_work(n, batch), vec = k_vec > 0 ? cl_vec_work(n, k_vec) : 0, nv = (size_t)batch * (k_low + 1);
    if (ensure(st, cs.work, (tri + vec) * sizeof(double)) || ensure(st, cs.vals, nv * sizeof(double)) ||
        (k_vec > 0 && ensure(st, cs.vecs, (size_t)n * k_vec * sizeof(double))))
        return -1;
    const ClTri t = cl_tri_split((double *)cs.work.p, n, batch);
    if (stage_begin(cs, st)) return -1;
    launch_cl_tridiag((double *)cs.mat.p, n, batch, t, st);
    if (stage_end(cs, st, CL_TRIDIAG) || stage_begin(cs, st)) return -1;
    launch_cl_bisect(t, n, batch, k_low, (double *)cs.vals.p, st);
    if (stage_end(cs, st, CL_VALUES)) return -1;
    vals.resize(nv);
    if (download(st, vals.data(), cs.vals.p, nv)) return -1;
    if (k_vec <= 0) return 0;
    if (stage_begin(cs, st)) return -1;
    launch_cl_vectors((const double *)cs.mat.p, t, n, (const double *)cs.vals.p, k_vec, (double *)cs.work.p + tri, (double *)cs.vecs.p, st);
    if (stage_end(cs, st, CL_VECTORS)) return -1;
    return download(st, vectors, cs.vecs.p, (size_t)n * k_vec);
}

// is the symmetrised graph of the bitmap cs.keep (one candidate, n rows) one component?  O(n p) on the neighbour lists
int bitmap_connected(ClusterState &cs, hipStream_t st, int n, bool &out) {
    const size_t W = cl_keep_words(n);
    std::vector<unsigned> bits((size_t)n * W);
    if (download(st, bits.data(), cs.keep.p, bits.size())) return -1;
    std::vector<std::vector<int>> adj(n);
    for (int i = 0; i < n; i++)
        for (size_t w = 0; w < W; w++)
            for (unsigned m = bits[(size_t)i * W + w]; m; m &= m - 1) {
                const int j = (int)w * 32 + __builtin_ctz(m);
                if (j != i) { adj[i].push_back(j); adj[j].push_back(i); }
            }
    out = nmesc_shared::connected(n, [&](int v, auto &&visit) { for (int j : adj[v]) visit(j); });
    return 0;
}
void reset_times(ClusterState &cs) { for (float &m : cs.ms) m = 0.f; }

}  // namespace

void cluster_free(ClusterState &cs) {
    for (ClBuf *b : {&cs.emb, &cs.unit, &cs.aff, &cs.minmax, &cs.plist, &cs.keep, &cs.graph, &cs.mat, &cs.work, &cs.vals, &cs.vecs})
        if (b->p) { hipFree(b->p); b->p = nullptr; b->cap = 0; }
    for (auto &e : cs.ev) if (e) { hipEventDestroy(e); e = nullptr; }
    cs.ready = false;
}

int cluster_affinity(ClusterState &cs, hipStream_t st, const float *emb, int N, int D, float *out) {
    if (!emb || !out || N < 1 || D < 1) return failf("nasr_diar_cluster_affinity: null argument, N < 1 or D < 1");
    if (N > CL_MAX_N) return failf("nasr_diar_cluster_affinity: N = %d is above the device path's cap of %d", N, CL_MAX_N);
    if (N == 1) { out[0] = 1.0f; return 0; }
    reset_times(cs);
    if (prepare(cs) || affinity_device(cs, st, emb, N, D)) return -1;
    return download(st, out, cs.aff.p, (size_t)N * N);
}

int cluster_graph(ClusterState &cs, hipStream_t st, const float *aff, int N, int p, float *graph_out) {
    if (!aff || !graph_out || N < 1 || p < 1) return failf("nasr_diar_cluster_graph: null argument, N < 1 or p < 1");
    if (N > CL_MAX_N) return failf("nasr_diar_cluster_graph: N = %d is above the device path's cap of %d", N, CL_MAX_N);
    reset_times(cs);
    const size_t nn = (size_t)N * N;
    if (prepare(cs) || ensure(st, cs.aff, nn * sizeof(float))) return -1;
    CCHK(hipMemcpyAsync(cs.aff.p, aff, nn * sizeof(float), hipMemcpyHostToDevice, st));
    if (graphs_device(cs, st, N, 1, N, &p, 1, false, true)) return -1;
    return download(st, graph_out, cs.graph.p, nn);
}

int cluster_sym_eigen(ClusterState &cs, hipStream_t st, const double *a, int n, int batch, int k_low, double *values_low, double *value_max,
                      double *vectors) {
    if (!a || !values_low || !value_max || n < 1 || batch < 1) return failf("nasr_diar_sym_eigen: null argument, n < 1 or batch < 1");
    if (k_low < 1 || k_low > n || k_low > CL_MAX_VALUES) return failf("nasr_diar_sym_eigen: k_low = %d outside 1 .. min(n, %d)", k_low, CL_MAX_VALUES);
    const size_t bytes = (size_t)batch * n * n * sizeof(double);
    if (n > CL_MAX_N || (batch > 1 && bytes > CL_BATCH_BYTES))
        return failf("nasr_diar_sym_eigen: n = %d above %d, or %d matrices above %zu bytes", n, CL_MAX_N, batch, CL_BATCH_BYTES);
    reset_times(cs);
    if (prepare(cs) || ensure(st, cs.mat, bytes)) return -1;
    CCHK(hipMemcpyAsync(cs.mat.p, a, bytes, hipMemcpyHostToDevice, st));
    std::vector<double> vals;
    if (eigen_device(cs, st, n, batch, k_low, vals, vectors ? k_low : 0, vectors)) return -1;
    for (int b = 0; b < batch; b++) {
        std::copy_n(&vals[(size_t)b * (k_low + 1)], k_low, values_low + (size_t)b * k_low);
        value_max[b] = vals[(size_t)b * (k_low + 1) + k_low];
    }
    return 0;
}

// nmesc_cluster (host/diarize_cluster_amd.cpp) step for step
int cluster_run(ClusterState &cs, hipStream_t st, const float *emb, int N, int D, const nmesc_cfg &cfg, nmesc_result &res) {
    using namespace nmesc_shared;
    if (!emb || N < 1 || D < 1) return failf("nasr_diar_cluster: null argument, N < 1 or D < 1");
    if (cfg.max_num_speakers < 1 || cfg.max_num_speakers >= CL_MAX_VALUES || cfg.nme_mat_size < 1)
        return failf("nasr_diar_cluster: max_num_speakers outside 1 .. %d or nme_mat_size < 1", CL_MAX_VALUES - 1);
    res = nmesc_result();
    reset_times(cs);
    if (early_return(N, cfg, res)) return 0;
    if (N > CL_MAX_N) return failf("nasr_diar_cluster: N = %d is above the device path's cap of %d (the host path has none)", N, CL_MAX_N);
    if (prepare(cs) || affinity_device(cs, st, emb, N, D)) return -1;
    // the NME analysis: every candidate's Laplacian of the (subsampled) affinity, batched
    const int ratio = subsample_ratio(N, cfg), Ns = (N + ratio - 1) / ratio;
    const std::vector<int> ps = analysis_candidates(Ns, cfg);
    const int k_low = gap_values(Ns, cfg.max_num_speakers);
    const size_t chunk = std::max<size_t>(1, std::min(ps.size(), CL_BATCH_BYTES / ((size_t)Ns * Ns * sizeof(double))));
    Choice best;
    best.p = ps[0];
    std::vector<double> vals;
    for (size_t c0 = 0; c0 < ps.size(); c0 += chunk) {
        const int C = (int)std::min(chunk, ps.size() - c0);
        if (graphs_device(cs, st, N, ratio, Ns, &ps[c0], C, true, false) || eigen_device(cs, st, Ns, C, k_low, vals, 0, nullptr)) return -1;
        for (int c = 0; c < C; c++) {
            const double *lam = &vals[(size_t)c * (k_low + 1)];
            consider(best, gap_rule(lam, lam[k_low], Ns, ps[c0 + c], cfg.max_num_speakers), ps[c0 + c]);
        }
    }
    // the graph of the chosen p on the full matrix; grow p until it is connected (:367-381)
    int p_hat = ratio * best.p;
    bool whole = false;
    if (graphs_device(cs, st, N, 1, N, &p_hat, 1, false, false) || bitmap_connected(cs, st, N, whole)) return -1;
    for (size_t c = 0; !whole && c < ps.size(); c++) {
        p_hat = ratio * ps[c];
        if (graphs_device(cs, st, N, 1, N, &p_hat, 1, false, false) || bitmap_connected(cs, st, N, whole)) return -1;
    }
    const int n_clusters = cluster_count(best.est, cfg);
    if (n_clusters > N) return failf("nasr_diar_cluster: %d clusters of %d embeddings", n_clusters, N);
    res.est_num_speakers = n_clusters;
    res.p_hat = p_hat;
    if (n_clusters == 1) { res.labels.assign(N, 0); return 0; }
    // spectral embedding = the eigenvectors of the n_clusters smallest Laplacian eigenvalues (:309-319), then k-means++ on the host
    if (ensure(st, cs.mat, (size_t)N * N * sizeof(double)) || stage_begin(cs, st)) return -1;
    launch_cl_laplacian((const unsigned *)cs.keep.p, N, 1, (double *)cs.mat.p, nullptr, st);
    if (stage_end(cs, st, CL_GRAPH)) return -1;
    std::vector<double> vec((size_t)N * n_clusters);
    if (eigen_device(cs, st, N, 1, n_clusters, vals, n_clusters, vec.data())) return -1;
    std::vector<float> se((size_t)N * n_clusters);
    for (int i = 0; i < N; i++)
        for (int k = 0; k < n_clusters; k++) se[(size_t)i * n_clusters + k] = (float)vec[(size_t)i * n_clusters + (n_clusters - 1 - k)];
    res.labels = kmeans_trials(se, N, n_clusters, cfg);
    return 0;
}

}  // namespace nasr
