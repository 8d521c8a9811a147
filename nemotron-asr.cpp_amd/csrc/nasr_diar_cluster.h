// nasr_diar_cluster.h -- NME-SC speaker clustering on the device (kernels_cluster.hip, nasr_diar_cluster.hip): the scratch the
// side-car keeps for it, the kernels' launchers and the four operations behind the C ABI (nasr_diar_cluster*, nasr_diar_sym_eigen).
// Include after nasr_internal.h.
#pragma once
#include <cstddef>
#include <cstdint>

struct nmesc_cfg;
struct nmesc_result;

namespace nasr {

constexpr int CL_MAX_N = 8192;           // order of the largest matrix: the Householder step keeps two vectors of that many doubles in LDS (128 KiB of 160)
constexpr int CL_MAX_VALUES = 64;        // eigenvalues per matrix the bisection kernel finds (one thread each), eigenvectors the iteration carries
constexpr size_t CL_BATCH_BYTES = (size_t)1 << 29;     // f64 matrices of one batched eigen-solve: the sweep's candidates go through in chunks of this

enum { CL_AFFINITY = 0, CL_GRAPH, CL_TRIDIAG, CL_VALUES, CL_VECTORS, CL_STAGES };

struct ClBuf { void *p = nullptr; size_t cap = 0; };
struct ClusterState {                    // allocated on first use, grown on demand, freed by cluster_free (nasr_diar_destroy)
    ClBuf emb, unit, aff, minmax, plist, keep, graph, mat, work, vals, vecs;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms[CL_STAGES] = {0.f, 0.f, 0.f, 0.f, 0.f};   // device time per stage of the last call
    bool ready = false;
};
void cluster_free(ClusterState &cs);

// every function: 0, or -1 with nasr_last_error set; all device work on `st`; host pointers in and out
int cluster_affinity(ClusterState &cs, hipStream_t st, const float *emb, int N, int D, float *out);
int cluster_graph(ClusterState &cs, hipStream_t st, const float *aff, int N, int p, float *graph_out);
int cluster_sym_eigen(ClusterState &cs, hipStream_t st, const double *a, int n, int batch, int k_low, double *values_low, double *value_max,
                      double *vectors);
int cluster_run(ClusterState &cs, hipStream_t st, const float *emb, int N, int D, const nmesc_cfg &cfg, nmesc_result &res);

// ---- kernels_cluster.hip -----------------------------------------------------------------------------------------------------
void init_cluster_kernel_attributes();
inline int cl_pad4(int D) { return (D + 3) & ~3; }
// rows of emb [N][D] to unit length (norm + 3.5e-4) -> unit [N][cl_pad4(D)], X X^T on the f64 MFMA, min-max scaling -> aff [N][N], symmetric
void launch_cl_affinity(const float *emb, int N, int D, float *unit, unsigned *minmax, float *aff, hipStream_t st);
inline size_t cl_keep_words(int n) { return (size_t)(n + 31) / 32; }
// keep[c][i] = bitmap of the min(p_list[c], n) largest entries of row i (value descending, lower index first) of the n x n matrix
// whose entry (i, j) is aff[(i * stride) * ld + j * stride]
void launch_cl_select(const float *aff, int ld, int stride, int n, const int *p_list, int C, unsigned *keep, hipStream_t st);
// g = 0.5 (keep + keep^T): graph [C][n][n] f32 (or null) and the Laplacian lap [C][n][n] f64 (or null): off-diagonal -g, diagonal = sum of the off-diagonal g
void launch_cl_laplacian(const unsigned *keep, int n, int C, double *lap, float *graph, hipStream_t st);
inline size_t cl_tri_work(int n, int batch) { return (size_t)9 * n * batch; }       // doubles: v, A v and the pivot row twice each, d, e, beta
struct ClTri { double *v, *s, *piv, *d, *e, *beta; };                               // v, s, piv: [2][batch][n]; d, e, beta: [batch][n]
inline ClTri cl_tri_split(double *work, int n, int batch) {
    const size_t bn = (size_t)n * batch;
    return {work, work + 2 * bn, work + 4 * bn, work + 6 * bn, work + 7 * bn, work + 8 * bn};
}
// Householder tridiagonalisation of `batch` symmetric matrices a [batch][n][n] in place: T = (d, e); the reflector of step k stays in
// the tail of row k, its beta in t.beta.  n - 1 launches
void launch_cl_tridiag(double *a, int n, int batch, const ClTri &t, hipStream_t st);
// the k_low smallest eigenvalues (ascending) and the largest of every tridiagonal: out [batch][k_low + 1]
void launch_cl_bisect(const ClTri &t, int n, int batch, int k_low, double *out, hipStream_t st);
inline size_t cl_vec_work(int n, int k) { return (size_t)5 * n * k; }               // doubles: the LU factors and right-hand side per vector, the vectors
// eigenvectors of matrix 0 for the k eigenvalues lam (device, ascending): inverse iteration on T, re-orthogonalised, then back through
// the reflectors in a -> out [n][k]
void launch_cl_vectors(const double *a, const ClTri &t, int n, const double *lam, int k, double *work, double *out, hipStream_t st);

}  // namespace nasr
