// kernels_cluster.hip -- NME-SC speaker clustering on the device (host/diarize_cluster_amd.cpp is the definition): cosine affinity on
// the f64 MFMA, p-nearest-neighbour graphs by radix select, their Laplacians, and a batched symmetric eigen-solver in f64 (Householder
// tridiagonalisation with one launch per step, Sturm-count bisection, inverse iteration, back-transform).  gfx950, wave64.
#include "nasr_internal.h"
#include "nasr_diar_cluster.h"

#include <algorithm>
#include <cfloat>

namespace nasr {
namespace {

constexpr int CL_T = 256;                 // threads of every workgroup here but the affinity's row kernel
constexpr float AFF_EPS = 3.5e-4f;        // host/diarize_cluster_shared.h

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over the 256 threads, the same order of additions in every workgroup (workgroups that recompute a scalar get the same bits);
// red: 4 doubles of LDS
__device__ inline double block_sum(double v, double *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// floats as unsigned keys of the same order (-0 counts as +0, as the host's comparisons do)
__device__ inline unsigned f32_key(float f) {
    const unsigned u = f == 0.0f ? 0u : __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key_f32(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- 1. affinity --------------------------------------------------------------------------------------------------------------
// one wave per row: unit[i] = emb[i] * (1 / (|emb[i]| + eps)), the squared norm summed in double, columns D .. Dp zero
__global__ __launch_bounds__(64) void k_cl_unit(const float *__restrict__ emb, int D, int Dp, float *__restrict__ unit, unsigned *minmax) {
    const size_t i = blockIdx.x;
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) { const double e = emb[i * D + d]; s += e * e; }
    s = wave_sum(s);
    const float inv = 1.0f / (sqrtf((float)s) + AFF_EPS);
    for (int d = lane; d < Dp; d += 64) unit[i * Dp + d] = d < D ? emb[i * D + d] * inv : 0.0f;
    if (i == 0 && lane == 0) minmax[0] = minmax[1] = f32_key(1.0f);       // the diagonal takes part in the minimum and the maximum
}

// X X^T above the diagonal, 32 x 32 entries per workgroup: the two 32-row panels go through LDS in chunks of 64 columns, each of the
// four waves owns a 16 x 16 tile and feeds v_mfma_f64_16x16x4_f64 (A: lane l holds row l % 16, column l / 16 of a 16 x 4 slice; the
// accumulator: register r of lane l = row 4 r + l / 16, column l % 16).  Products of two floats are exact in double, so the rounded
// sums equal the host's double dots but for double rounding.  Writes both triangles, 1 on the diagonal, and reduces min / max
constexpr int GK = 64, GLD = GK + 4;
__global__ __launch_bounds__(CL_T) void k_cl_gram(const float *__restrict__ unit, int N, int Dp, float *__restrict__ raw, unsigned *minmax) {
    if (blockIdx.x < blockIdx.y) return;                                  // below the diagonal: mirrored from above
    __shared__ float sA[32 * GLD], sB[32 * GLD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = blockIdx.y * 32, col0 = blockIdx.x * 32, tr = wave >> 1, tc = wave & 1;
    const bool dead = blockIdx.x == blockIdx.y && tr > tc;                // this wave's tile lies below the diagonal
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < Dp; k0 += GK) {
        __syncthreads();
        for (int x = t; x < 32 * GK; x += CL_T) {
            const int rr = x / GK, cc = x % GK;
            const bool in = k0 + cc < Dp;
            sA[rr * GLD + cc] = in && row0 + rr < N ? unit[(size_t)(row0 + rr) * Dp + k0 + cc] : 0.0f;
            sB[rr * GLD + cc] = in && col0 + rr < N ? unit[(size_t)(col0 + rr) * Dp + k0 + cc] : 0.0f;
        }
        __syncthreads();
        if (dead) continue;
        const int kn = min(GK, Dp - k0);                                  // a multiple of 4
        for (int kk = 0; kk < kn; kk += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)sA[(tr * 16 + r) * GLD + kk + q], (double)sB[(tc * 16 + r) * GLD + kk + q], acc, 0, 0, 0);
    }
    if (dead) return;
    float lo = INFINITY, hi = -INFINITY;
    const int gj = col0 + tc * 16 + r;
    for (int x = 0; x < 4; x++) {
        const int gi = row0 + tr * 16 + 4 * x + q;
        if (gi >= N || gj >= N || gi > gj) continue;
        if (gi == gj) { raw[(size_t)gi * N + gj] = 1.0f; continue; }
        const float v = (float)acc[x];
        raw[(size_t)gi * N + gj] = raw[(size_t)gj * N + gi] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if (lane == 0 && lo <= hi) { atomicMin(&minmax[0], f32_key(lo)); atomicMax(&minmax[1], f32_key(hi)); }
}

// (v - lo) / range, a float division like the host's: the largest entry scales to exactly 1
__global__ __launch_bounds__(CL_T) void k_cl_scale(float *aff, size_t n, const unsigned *minmax) {
    const float lo = key_f32(minmax[0]), hi = key_f32(minmax[1]);
    if (!(hi > lo)) return;
    const float range = hi - lo;
    for (size_t i = (size_t)blockIdx.x * CL_T + threadIdx.x; i < n; i += (size_t)gridDim.x * CL_T) aff[i] = (aff[i] - lo) / range;
}

// ---- 2. neighbour graph and Laplacian -----------------------------------------------------------------------------------------
// One workgroup per (row, candidate): the row's keys in LDS, the k-th largest key by an 8-bit radix select (four histogram passes),
// everything above it kept, the tie band at it filled by ascending index.  LDS: n keys, the bitmap, 256 bins, 3 words
__global__ __launch_bounds__(CL_T) void k_cl_select(const float *__restrict__ aff, int ld, int stride, int n, const int *__restrict__ p_list,
                                                   unsigned *__restrict__ keep) {
    extern __shared__ unsigned sm_u[];
    const int W = (n + 31) / 32, t = threadIdx.x;
    unsigned *keys = sm_u, *bits = keys + n, *hist = bits + W, *pick = hist + 256;     // pick: the digit chosen, how many still to take below it
    const int row = blockIdx.x, k = min(p_list[blockIdx.y], n);
    const float *src = aff + (size_t)row * stride * ld;
    for (int j = t; j < n; j += CL_T) keys[j] = f32_key(src[(size_t)j * stride]);
    for (int w = t; w < W; w += CL_T) bits[w] = 0u;
    unsigned prefix = 0u, mask = 0u;
    int need = k;                                   // the threshold is the need-th largest of the keys that match prefix under mask
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[t] = 0u;
        __syncthreads();
        for (int j = t; j < n; j += CL_T)
            if ((keys[j] & mask) == prefix) atomicAdd(&hist[(keys[j] >> shift) & 255u], 1u);
        __syncthreads();
        if (t == 0) {
            int above = 0, b = 255;
            for (; b > 0 && above + (int)hist[b] < need; b--) above += (int)hist[b];
            pick[0] = (unsigned)b;
            pick[1] = (unsigned)(need - above);
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        mask |= 255u << shift;
        need = (int)pick[1];
        __syncthreads();
    }
    // prefix = the k-th largest key; `need` of the entries equal to it are kept, lowest index first: every thread ranks a contiguous run
    const int run = (n + CL_T - 1) / CL_T, j0 = min(t * run, n), j1 = min(j0 + run, n);
    int ties = 0;
    for (int j = j0; j < j1; j++) ties += keys[j] == prefix;
    hist[t] = (unsigned)ties;
    __syncthreads();
    int rank = 0;
    for (int u = 0; u < t; u++) rank += (int)hist[u];
    for (int j = j0; j < j1; j++) {
        const unsigned key = keys[j];
        if (key > prefix || (key == prefix && rank++ < need)) atomicOr(&bits[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    unsigned *out = keep + ((size_t)blockIdx.y * n + row) * W;
    for (int w = t; w < W; w += CL_T) out[w] = bits[w];
}

// one workgroup per (row, candidate): g = 0.5 (keep + keep^T) as f32 and / or the Laplacian row in f64
__global__ __launch_bounds__(CL_T) void k_cl_laplacian(const unsigned *__restrict__ keep, int n, double *__restrict__ lap, float *__restrict__ graph) {
    __shared__ double red[4];
    const int W = (n + 31) / 32, i = blockIdx.x, t = threadIdx.x;
    const unsigned *kb = keep + (size_t)blockIdx.y * n * W;
    const size_t base = ((size_t)blockIdx.y * n + i) * n;
    double deg = 0.0;
    for (int j = t; j < n; j += CL_T) {
        const unsigned kij = (kb[(size_t)i * W + (j >> 5)] >> (j & 31)) & 1u, kji = (kb[(size_t)j * W + (i >> 5)] >> (i & 31)) & 1u;
        const float g = 0.5f * (float)(kij + kji);
        if (graph) graph[base + j] = g;
        if (lap && j != i) { lap[base + j] = -(double)g; deg += (double)g; }
    }
    if (!lap) return;
    deg = block_sum(deg, red);
    if (t == 0) lap[base + i] = deg;
}

// ---- 3. tridiagonalisation ----------------------------------------------------------------------------------------------------
// Householder, H = I - beta v v^T per step, the two-sided update A22 -= v w^T + w v^T one launch LATE: launch k
//   (a) every workgroup: w' of step k-1 from v' and s' = A v' (the previous launch's products), then row k as step k-1 leaves it from the
//       side copy its owner wrote in the previous launch, then v, beta, alpha of step k.  O(n) work, the same bits everywhere;
//   (b) its own rows i > k: apply step k-1's update to columns > k, form s_i = A[i] . v in the same pass, and, as the owner of row
//       k + 1, write the next launch's side copy.
// Nobody reads a row of A another workgroup writes; v, s and the side copy alternate between two buffers.  Workgroup 0 records d[k],
// e[k], beta[k] and v (into the buffer and, as the stored reflector, into the tail of row k, which nothing reads again).
// LDS: w' (n - k doubles), v (n - k - 1), 4 for the sums
constexpr int TRI_ROWS = 8;               // rows per workgroup, two per wave
__global__ __launch_bounds__(CL_T) void k_cl_tri_init(const double *__restrict__ a, int n, ClTri w, int batch) {
    const size_t b = blockIdx.y, bn = (size_t)n * batch;
    const int j = blockIdx.x * CL_T + threadIdx.x;
    if (j >= n) return;
    const size_t o = b * n + j;
    w.v[o] = w.v[bn + o] = w.s[o] = w.s[bn + o] = w.piv[bn + o] = 0.0;
    w.piv[o] = a[b * n * n + j];                                          // row 0 is launch 0's pivot row
    w.beta[o] = w.e[o] = 0.0;
    w.d[o] = j == 0 ? a[b * n * n] : 0.0;                                 // n == 1: no launch follows
}

__global__ __launch_bounds__(CL_T) void k_cl_tri_step(double *__restrict__ a, int n, int k, ClTri w, int batch) {
    extern __shared__ double sm_d[];
    const int m = n - k - 1, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double *wp = sm_d, *v = wp + m + 1, *red = v + m;                     // wp[j - k], v[j - k - 1]
    const size_t b = blockIdx.y, bn = (size_t)n * batch, cur = (size_t)(k & 1) * bn + b * n, prv = (size_t)((k & 1) ^ 1) * bn + b * n;
    const double *vp = w.v + prv, *sp = w.s + prv, *piv = w.piv + cur;
    double *A = a + b * n * n;
    const double betap = k > 0 ? w.beta[b * n + k - 1] : 0.0;
    // (a) w' = p' - (beta' / 2)(v' . p') v',  p' = beta' s'
    double part = 0.0;
    for (int j = k + t; j < n; j += CL_T) part += vp[j] * (betap * sp[j]);
    const double half = 0.5 * betap * block_sum(part, red);
    for (int j = k + t; j < n; j += CL_T) wp[j - k] = betap * sp[j] - half * vp[j];
    __syncthreads();
    // row k after step k-1: d[k] at column k, the new column x to its right
    const double vk = vp[k], wk = wp[0];
    part = 0.0;
    for (int j = k + 1 + t; j < n; j += CL_T) {
        const double x = piv[j] - (vk * wp[j - k] + wk * vp[j]);
        v[j - k - 1] = x;
        if (j > k + 1) part += x * x;
    }
    const double below = block_sum(part, red);                            // also orders the writes of v before the reads below
    const double dk = piv[k] - 2.0 * vk * wk, x0 = v[0];
    double alpha = x0, beta = 0.0;
    __syncthreads();
    if (below != 0.0) {                                                   // else: the column is tridiagonal already (m == 1 included): no reflection
        alpha = x0 > 0.0 ? -sqrt(x0 * x0 + below) : sqrt(x0 * x0 + below);
        if (t == 0) v[0] = x0 - alpha;
        beta = 2.0 / ((x0 - alpha) * (x0 - alpha) + below);
    } else {
        for (int j = t; j < m; j += CL_T) v[j] = 0.0;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (t == 0) { w.d[b * n + k] = dk; w.e[b * n + k] = alpha; w.beta[b * n + k] = beta; }
        for (int j = t; j < m; j += CL_T) A[(size_t)k * n + k + 1 + j] = w.v[cur + k + 1 + j] = v[j];
    }
    // (b) own rows
    for (int r = wave; r < TRI_ROWS; r += CL_T / 64) {
        const int i = k + 1 + blockIdx.x * TRI_ROWS + r;
        if (i >= n) break;
        double *row = A + (size_t)i * n;
        const double vi = vp[i], wi = wp[i - k];
        double s = 0.0;
        for (int j = k + 1 + lane; j < n; j += 64) {
            const double x = row[j] - (vi * wp[j - k] + wi * vp[j]);
            row[j] = x;
            s += x * v[j - k - 1];
            if (i == k + 1) w.piv[prv + j] = x;
        }
        s = wave_sum(s);
        if (lane == 0) {
            w.s[cur + i] = s;
            if (m == 1) w.d[b * n + i] = row[i];                          // the last launch: the last diagonal entry
        }
    }
}

// ---- 4. eigenvalues by bisection ----------------------------------------------------------------------------------------------
// how many eigenvalues of T lie below x (the signs of the pivots of T - x I, LAPACK dstebz's recurrence: a vanishing pivot becomes
// -pivmin, so exact splits e[i] == 0 need no special case)
__device__ inline int sturm_count(const double *__restrict__ d, const double *__restrict__ e, int n, double x, double pivmin) {
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int cnt = q < 0.0;
    for (int i = 1; i < n; i++) {
        q = d[i] - x - e[i - 1] * e[i - 1] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0;
    }
    return cnt;
}
// one workgroup per matrix, one thread per wanted eigenvalue: thread t < k_low finds eigenvalue t, thread k_low the largest
__global__ void k_cl_bisect(ClTri w, int n, int k_low, double *__restrict__ out) {
    const size_t b = blockIdx.x;
    const int t = threadIdx.x;
    if (t > k_low) return;
    const double *d = w.d + b * n, *e = w.e + b * n;
    double gl = INFINITY, gu = -INFINITY, emax = 0.0;
    for (int i = 0; i < n; i++) {                                         // Gershgorin
        const double rad = (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < n ? fabs(e[i]) : 0.0);
        gl = fmin(gl, d[i] - rad);
        gu = fmax(gu, d[i] + rad);
        if (i + 1 < n) emax = fmax(emax, e[i] * e[i]);
    }
    const double tnorm = fmax(fabs(gl), fabs(gu)), pivmin = DBL_MIN * fmax(1.0, emax);
    const double abstol = fmax(DBL_EPSILON * tnorm, pivmin), margin = 2.0 * tnorm * DBL_EPSILON * n + 2.0 * pivmin;
    double lo = gl - margin, hi = gu + margin;
    const int idx = t < k_low ? t : n - 1;
    for (int it = 0; it < 1100; it++) {
        const double mid = 0.5 * (lo + hi);
        if (hi - lo <= abstol + 2.0 * DBL_EPSILON * fmax(fabs(lo), fabs(hi)) || mid <= lo || mid >= hi) break;
        if (sturm_count(d, e, n, mid, pivmin) > idx) hi = mid;
        else lo = mid;
    }
    out[b * (k_low + 1) + t] = 0.5 * (lo + hi);
}

// ---- 5. eigenvectors ----------------------------------------------------------------------------------------------------------
// x <- (T - lam I)^-1 x by Gaussian elimination with partial pivoting on the tridiagonal (LAPACK dlagtf / dlagts): one thread, the
// factor rows (u0, u1, u2) and the transformed right-hand side in f[4][n][k] (column t of each), pivots below `tiny` replaced by it
__device__ inline double guard(double p, double tiny) { return fabs(p) < tiny ? (p < 0.0 ? -tiny : tiny) : p; }
__device__ void tri_solve(const double *__restrict__ d, const double *__restrict__ e, int n, double lam, double tiny, double *f, int k, int t, double *x) {
    const size_t nk = (size_t)n * k;
    double *U0 = f + t, *U1 = U0 + nk, *U2 = U1 + nk, *Z = U2 + nk;
    double u0 = d[0] - lam, u1 = n > 1 ? e[0] : 0.0, r = x[0];
    for (int i = 0; i + 1 < n; i++) {
        const double c = e[i], a1 = d[i + 1] - lam, b1 = i + 2 < n ? e[i + 1] : 0.0, y1 = x[i + 1];
        const size_t o = (size_t)i * k;
        if (fabs(c) > fabs(u0)) {                                         // the next row is the pivot row
            const double piv = guard(c, tiny), mult = u0 / piv;
            U0[o] = piv; U1[o] = a1; U2[o] = b1; Z[o] = y1;
            u0 = u1 - mult * a1; u1 = -mult * b1; r -= mult * y1;
        } else {
            const double piv = guard(u0, tiny), mult = c / piv;
            U0[o] = piv; U1[o] = u1; U2[o] = 0.0; Z[o] = r;
            u0 = a1 - mult * u1; u1 = b1; r = y1 - mult * r;
        }
    }
    double x1 = r / guard(u0, tiny), x2 = 0.0;
    x[n - 1] = x1;
    for (int i = n - 2; i >= 0; i--) {
        const size_t o = (size_t)i * k;
        const double xi = (Z[o] - U1[o] * x1 - U2[o] * x2) / U0[o];
        x[i] = xi;
        x2 = x1;
        x1 = xi;
    }
}
// One workgroup: k threads run the solves of an iteration side by side, then all 256 orthonormalise the k vectors in ascending order
// (modified Gram-Schmidt).  Within a cluster of close eigenvalues -- the zeros of a nearly disconnected graph -- that yields an
// orthonormal basis of the cluster's invariant subspace; for a separated eigenvalue it removes O(eps) and the next solve restores the
// direction.  X [k][n]; work = f [4][n][k]
constexpr int INVIT_ROUNDS = 5;
__global__ __launch_bounds__(CL_T) void k_cl_invit(ClTri w, int n, const double *__restrict__ lam, int k, double *f, double *X) {
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double *d = w.d, *e = w.e;                                      // matrix 0
    double nrm = 0.0;
    for (int i = t; i < n; i += CL_T) nrm = fmax(nrm, fabs(d[i]) + (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < n ? fabs(e[i]) : 0.0));
    for (int o = 32; o > 0; o >>= 1) nrm = fmax(nrm, __shfl_xor(nrm, o));
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = nrm;
    __syncthreads();
    const double tiny = fmax(DBL_EPSILON * fmax(fmax(red[0], red[1]), fmax(red[2], red[3])), 1e-290);
    for (int c = 0; c < k; c++)
        for (int i = t; i < n; i += CL_T) {                               // start vectors: a hash of (entry, vector) in [-1, 1)
            unsigned h = (unsigned)i * 2654435761u ^ ((unsigned)c + 1u) * 0x9E3779B9u;
            h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
            X[(size_t)c * n + i] = (double)h * (1.0 / 2147483648.0) - 1.0;
        }
    for (int round = 0; round < INVIT_ROUNDS; round++) {
        __syncthreads();
        if (t < k) tri_solve(d, e, n, lam[t], tiny, f, k, t, X + (size_t)t * n);
        __syncthreads();
        for (int c = 0; c < k; c++) {
            double *xc = X + (size_t)c * n;
            for (int u = 0; u < c; u++) {
                const double *xu = X + (size_t)u * n;
                double part = 0.0;
                for (int i = t; i < n; i += CL_T) part += xu[i] * xc[i];
                const double dot = block_sum(part, red);
                for (int i = t; i < n; i += CL_T) xc[i] -= dot * xu[i];
            }
            double part = 0.0;
            for (int i = t; i < n; i += CL_T) part += xc[i] * xc[i];
            const double len = sqrt(block_sum(part, red));
            if (len > 0.0)
                for (int i = t; i < n; i += CL_T) xc[i] /= len;
        }
    }
}
// eigenvector of A = H_0 H_1 ... H_{n-3} y: one workgroup per vector, y in LDS (n doubles + 4), the reflectors read from the row tails
__global__ __launch_bounds__(CL_T) void k_cl_back(const double *__restrict__ a, ClTri w, int n, const double *__restrict__ X, int k, double *__restrict__ out) {
    extern __shared__ double sm_d[];
    double *y = sm_d, *red = y + n;
    const int t = threadIdx.x, c = blockIdx.x;
    for (int i = t; i < n; i += CL_T) y[i] = X[(size_t)c * n + i];
    __syncthreads();
    for (int s = n - 3; s >= 0; s--) {
        const double beta = w.beta[s];
        if (beta == 0.0) continue;
        const double *v = a + (size_t)s * n;
        double part = 0.0;
        for (int j = s + 1 + t; j < n; j += CL_T) part += v[j] * y[j];
        const double scale = beta * block_sum(part, red);
        for (int j = s + 1 + t; j < n; j += CL_T) y[j] -= scale * v[j];
        __syncthreads();
    }
    for (int i = t; i < n; i += CL_T) out[(size_t)i * k + c] = y[i];
}

size_t tri_lds(int m) { return (size_t)(2 * m + 1 + 4) * sizeof(double); }
size_t back_lds(int n) { return (size_t)(n + 4) * sizeof(double); }
}  // namespace

void init_cluster_kernel_attributes() {
    (void)hipFuncSetAttribute((const void *)k_cl_tri_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tri_lds(CL_MAX_N));
    (void)hipFuncSetAttribute((const void *)k_cl_back, hipFuncAttributeMaxDynamicSharedMemorySize, (int)back_lds(CL_MAX_N));
}

void launch_cl_affinity(const float *emb, int N, int D, float *unit, unsigned *minmax, float *aff, hipStream_t st) {
    const int nb = (N + 31) / 32;
    hipLaunchKernelGGL(k_cl_unit, dim3(N), dim3(64), 0, st, emb, D, cl_pad4(D), unit, minmax);
    hipLaunchKernelGGL(k_cl_gram, dim3(nb, nb), dim3(CL_T), 0, st, unit, N, cl_pad4(D), aff, minmax);
    hipLaunchKernelGGL(k_cl_scale, dim3((unsigned)std::min<size_t>(((size_t)N * N + CL_T - 1) / CL_T, 4096)), dim3(CL_T), 0, st, aff, (size_t)N * N, minmax);
}

void launch_cl_select(const float *aff, int ld, int stride, int n, const int *p_list, int C, unsigned *keep, hipStream_t st) {
    const size_t lds = ((size_t)n + cl_keep_words(n) + 256 + 4) * sizeof(unsigned);
    hipLaunchKernelGGL(k_cl_select, dim3(n, C), dim3(CL_T), lds, st, aff, ld, stride, n, p_list, keep);
}

void launch_cl_laplacian(const unsigned *keep, int n, int C, double *lap, float *graph, hipStream_t st) {
    hipLaunchKernelGGL(k_cl_laplacian, dim3(n, C), dim3(CL_T), 0, st, keep, n, lap, graph);
}

void launch_cl_tridiag(double *a, int n, int batch, const ClTri &t, hipStream_t st) {
    hipLaunchKernelGGL(k_cl_tri_init, dim3((n + CL_T - 1) / CL_T, batch), dim3(CL_T), 0, st, a, n, t, batch);
    for (int k = 0; k + 1 < n; k++) {
        const int m = n - k - 1;
        hipLaunchKernelGGL(k_cl_tri_step, dim3((m + TRI_ROWS - 1) / TRI_ROWS, batch), dim3(CL_T), tri_lds(m), st, a, n, k, t, batch);
    }
}

void launch_cl_bisect(const ClTri &t, int n, int batch, int k_low, double *out, hipStream_t st) {
    hipLaunchKernelGGL(k_cl_bisect, dim3(batch), dim3((k_low + 1 + 63) / 64 * 64), 0, st, t, n, k_low, out);
}

void launch_cl_vectors(const double *a, const ClTri &t, int n, const double *lam, int k, double *work, double *out, hipStream_t st) {
    double *X = work + (size_t)4 * n * k;
    hipLaunchKernelGGL(k_cl_invit, dim3(1), dim3(CL_T), 0, st, t, n, lam, k, work, X);
    hipLaunchKernelGGL(k_cl_back, dim3(k), dim3(CL_T), back_lds(n), st, a, t, n, X, k, out);
}

}  // namespace nasr
