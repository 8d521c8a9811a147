// Test helper (not product code): the planes of a packed out_w (launch_joint_weight_planes) and ONE joint-alone call of launch_decode_iter with
// DecParams::out_planes null (k_dec_joint_tiled) and one with it set (k_dec_joint_split) on the same operands, for tests/test_gpu_joint_split.py and
// tests/micro/joint_split_cost.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -I../../include -o libjoint_split_harness.so joint_split_harness.hip   (built by __graft_entry__.build())
// No kernel of its own: launchers and weight packer are the product's, resolved from libnemotron_asr_amd.so (loaded with RTLD_GLOBAL before this library).
// Joint alone: n_active = n_dirty = 0, so the candidate kernels and the commit return at their first test and touch none of their (null) buffers.
#include "nasr_internal.h"
#include "nasr_engine_priv.h"
#include <stdio.h>
#include <string.h>
#include <vector>

namespace {
using namespace nasr;
char g_err[256];
static_assert(sizeof(RowDesc) == 32 && sizeof(nasr_lp::Part) == 8, "the layouts tests/decode_kernel_cases.py builds");

struct Dev {                                    // device buffers of one call, freed together
    std::vector<void *> all;
    hipError_t e = hipSuccess;
    template <typename T> T *get(size_t bytes, const void *src, int fill = -1) {
        void *p = nullptr;
        if (e == hipSuccess) e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) all.push_back(p);
        if (e == hipSuccess && src) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && !src && fill >= 0) e = hipMemset(p, fill, bytes);
        return (T *)p;
    }
    ~Dev() { for (void *p : all) (void)hipFree(p); }
};
}  // namespace

extern "C" const char *joint_split_error() { return g_err; }

// the form launch_decode_iter takes follows the buffers, as in the engine: lp -> lp_part, boost -> boost_bonus + boost_state (+ boost_raw with lp),
// alt (with lp) -> alt_key, lmf (with boost) -> lm_row, ent (with lp) -> ent_part.  repeat > 1: the pair of launches is repeated and, with ms != null, each
// arm's launches are timed with events in alternating order (tests/micro/joint_split_cost.py); the outputs are those of the last pair
struct JsCase { int B, T, pool, n_rows, n_states, alt_k, lp, boost, alt, lmf, ent, repeat; float ent_alpha; };

// rows [B] RowDesc, encproj [B T][640], predg [pool][640], out_w [1025][640] row-major, out_b [1025], rowmap [B T], boost_bonus [n_states][1040],
// boost_state [pool], lm_row [pool][1040].  Out, run 0 = out_planes null, run 1 = set: planes [65][20][2][64][8] u16, key [2][B T], lp_part [2][B T][17][2],
// alt_key [2][B T][17][alt_k], boost_raw / ent_part [2][B T][17] (written only in the forms that have them; unwritten elements are 0xff bytes), ms [2]
extern "C" int joint_split_run(int device, const JsCase *c, const void *rows, const float *encproj, const float *predg, const float *out_w, const float *out_b,
                               const unsigned *rowmap, const float *boost_bonus, const int *boost_state, const float *lm_row, void *planes, unsigned long long *key,
                               float *lp_part, unsigned long long *alt_key, float *boost_raw, float *ent_part, float *ms) {
    g_err[0] = 0;
    const int B = c->B, T = c->T, P = nasr_lp::WG_PARTS;
    const size_t BT = (size_t)B * T;
    if (B < 1 || T < 1 || B > 65535 || T > 65535 || BT <= (size_t)nasr_lp::SMALL_ROWS || BT > (1u << 20) || c->n_rows < 0 || (size_t)c->n_rows > BT || c->pool < 1 ||
        !nasr_topk::valid_k(c->alt_k) || (c->alt && (!c->lp || c->alt_k < 1)) || (c->ent && !c->lp) || (c->lmf && !c->boost) || (c->boost && c->n_states < 1) || c->repeat < 1) {
        snprintf(g_err, sizeof(g_err), "not a case of the tiled joint");
        return -1;
    }
    const RowDesc *hr = (const RowDesc *)rows;
    for (int b = 0; b < B; b++) if (hr[b].slot < 0 || hr[b].slot >= c->pool) { snprintf(g_err, sizeof(g_err), "rows: a slot outside the pool"); return -1; }
    for (size_t i = 0; i < BT; i++) if ((int)(rowmap[i] & 0xffffu) >= B || (int)(rowmap[i] >> 16) >= T) { snprintf(g_err, sizeof(g_err), "rowmap: an entry outside the step"); return -1; }
    if (c->boost && !c->lmf) for (int s = 0; s < c->pool; s++) if (boost_state[s] < 0 || boost_state[s] >= c->n_states) { snprintf(g_err, sizeof(g_err), "boost_state: outside the table"); return -1; }
    std::vector<float> w(out_w, out_w + (size_t)VOCAB * JNT), packed;
    nasr_eng::pack_f32_mfma(w, VOCAB, JNT, false, packed);
    if (packed.size() * 4 != JOINT_PLANE_BYTES) { snprintf(g_err, sizeof(g_err), "the packer's output has another size than the planes"); return -1; }
    Dev d;
    d.e = hipSetDevice(device);
    DecParams p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.T = T;
    p.rows = d.get<RowDesc>((size_t)B * sizeof(RowDesc), rows);
    p.encproj = d.get<float>(BT * JNT * 4, encproj);
    p.predg = d.get<float>((size_t)c->pool * JNT * 4, predg);
    p.out_w = d.get<float>(packed.size() * 4, packed.data());
    p.out_b = d.get<float>(VOCAB * 4, out_b);
    p.rowmap = d.get<unsigned>(BT * 4, rowmap);
    const int counters[3] = {0, 0, c->n_rows};
    int *cnt = d.get<int>(sizeof(counters), counters);
    p.n_active = cnt; p.n_dirty = cnt + 1; p.n_rows = cnt + 2;
    if (c->boost) { p.boost_bonus = d.get<float>(nasr_boost::table_elems(c->n_states) * 4, boost_bonus); p.boost_state = d.get<int>((size_t)c->pool * 4, boost_state); }
    if (c->lmf) p.lm_row = d.get<float>((size_t)c->pool * nasr_lm::ROW_COLS * 4, lm_row);
    p.alt_k = c->alt ? c->alt_k : 0; p.ent_alpha = c->ent_alpha;
    uint16_t *dplanes = d.get<uint16_t>(JOINT_PLANE_BYTES, nullptr, 0xff);
    // the outputs of both runs
    unsigned long long *dkey[2], *dalt[2] = {nullptr, nullptr};
    nasr_lp::Part *dlp[2] = {nullptr, nullptr};
    float *draw[2] = {nullptr, nullptr}, *dent[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; i++) {
        dkey[i] = d.get<unsigned long long>(BT * 8, nullptr, 0);
        if (c->lp) dlp[i] = d.get<nasr_lp::Part>(BT * P * 8, nullptr, 0xff);
        if (c->alt) dalt[i] = d.get<unsigned long long>(BT * P * c->alt_k * 8, nullptr, 0xff);
        if (c->lp && c->boost) draw[i] = d.get<float>(BT * P * 4, nullptr, 0xff);
        if (c->ent) dent[i] = d.get<float>(BT * P * 4, nullptr, 0xff);
    }
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (d.e == hipSuccess && ms) { d.e = hipEventCreate(&ev[0]); if (d.e == hipSuccess) d.e = hipEventCreate(&ev[1]); }
    if (d.e == hipSuccess) {
        launch_joint_weight_planes(p.out_w, dplanes, 0);
        float total[2] = {0.f, 0.f};
        for (int n = 0; n < c->repeat && d.e == hipSuccess; n++)
            for (int k = 0; k < 2 && d.e == hipSuccess; k++) {
                const int i = k ^ (n & 1);              // 0: out_planes null, 1: set
                d.e = hipMemsetAsync(dkey[i], 0, BT * 8, 0);          // the keys grow by atomicMax
                p.out_planes = i ? dplanes : nullptr;
                p.key = dkey[i]; p.lp_part = dlp[i]; p.alt_key = dalt[i]; p.boost_raw = draw[i]; p.ent_part = dent[i];
                if (ms) (void)hipEventRecord(ev[0], 0);
                launch_decode_iter(p, 0);
                if (ms) {
                    float t = 0.f;
                    (void)hipEventRecord(ev[1], 0);
                    if (d.e == hipSuccess) d.e = hipEventSynchronize(ev[1]);
                    if (d.e == hipSuccess) d.e = hipEventElapsedTime(&t, ev[0], ev[1]);
                    total[i] += t;
                }
            }
        if (d.e == hipSuccess) d.e = hipDeviceSynchronize();
        if (d.e == hipSuccess) d.e = hipGetLastError();
        if (ms) { ms[0] = total[0] / c->repeat; ms[1] = total[1] / c->repeat; }
    }
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    const auto back = [&d](void *dst, const void *src, size_t bytes) { if (d.e == hipSuccess && src) d.e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
    back(planes, dplanes, JOINT_PLANE_BYTES);
    for (int i = 0; i < 2; i++) {
        back(key + i * BT, dkey[i], BT * 8);
        back(lp_part + i * BT * P * 2, dlp[i], BT * P * 8);
        back(alt_key + i * BT * P * c->alt_k, dalt[i], BT * P * c->alt_k * 8);
        back(boost_raw + i * BT * P, draw[i], BT * P * 4);
        back(ent_part + i * BT * P, dent[i], BT * P * 4);
    }
    if (d.e != hipSuccess) snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(d.e));
    return d.e == hipSuccess ? 0 : -1;
}
