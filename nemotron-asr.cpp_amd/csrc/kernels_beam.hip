// kernels_beam.hip -- frame-synchronous beam search of the offline path (nasr_engine_transcribe_beam*; the rules, the trie, the slot
// binding and the backtrace are nasr_beam.h, shared with the host and tested there).
//   k_beam_init     the root hypothesis of every utterance: fresh decoder state in slot 0, frame 0's encoder row, the first work lists
//   k_beam_select   one round of one utterance per workgroup, between two evaluations (launch_decode_rows: the decode's own LSTM / joint.pred
//                   launches over the new hypotheses, then k_dec_joint_tiled in its LP + ALT form over every live hypothesis):
//                   merges the alternatives' slices of each of the <= W rows and finishes their ln P from the softmax parts, applies the C / D
//                   rules in double, creates the trie nodes, gathers each child's committed state from its parent's candidate state, rebinds
//                   the rows' slots and lists the rows of the next evaluation
//   k_beam_final    the N best of Beam_T: tokens, frames, ln P and scores (<LM, BOOST>: by the final key)
// Shallow fusion (nasr_engine_set_lm, nasr_lm.h): the LM instantiations of k_beam_select and k_beam_final.  Between the row phase and the serial
// rule phase one thread per (live hypothesis, expansion entry), at most 64, looks its token up in the n-gram tables in HBM (plain loads; the
// loops are bounded by the table header's order and max_probe) and leaves the term and the next LM state in LDS beside ex_lp / ex_tok; the
// final adds the EOS term per hypothesis and one thread re-ranks the <= 8 entries.  No launch and no host round trip is added.
// Phrase boosting (NASR_FLAG_BEAM_BOOST, nasr_boost.h): the BOOST instantiations, with or without the LM.  The evaluation is then the tiled joint's
// BEAMB form (lists by logit + bonus of the row's automaton state; the raw logits of every row kept).  The row phase merges the boosted lists as
// before; the same (hypothesis, entry) threads then read the entry's raw logit, form the MODEL's ln P from it and read the entry's bonus and next
// automaton state from the tables -- plain loads beside the LM look-up.  Every row bound for the next evaluation gets its slot's automaton state
// from its hypothesis (boost_state [n * 3 W], the beam's own array); k_beam_init writes the root; k_beam_final<LM, true> re-ranks by the boosted key and
// writes boost and that key per hypothesis.
// The host enqueues T_max * (S + 1) rounds blind; a finished utterance's workgroup returns at once and lists nothing.  No kernel waits on
// another workgroup: the lists of the next evaluation are filled through two atomic tickets per utterance, and the counters alternate between
// two pairs -- round r's evaluation reads pair r & 1, its select zeroes that pair (one thread; nobody adds to it in this launch) and adds to
// the other.  The order inside the lists is that of the tickets; every row of the evaluation is an independent accumulation chain, so the
// order cannot change a result.  Every loop bound is a launch parameter or at most W * 8, except same_seq's walk, bounded by the length.
#include "nasr_internal.h"

namespace nasr {

using nasr_beam::Beam;
using nasr_beam::KTOP;
using nasr_beam::WMAX;

__device__ __forceinline__ void beam_fresh_ctrl(DecCtrl *ct, int prev_token) {
    DecCtrl d;
    d.t = 0; d.n_frames = 0; d.symbols = 0; d.prev_token = prev_token;
    d.cur = 0; d.n_tok = 0; d.active = 0; d.iterations = 0; d.row = 0;
    d.dirty = 1; d.frame0 = 0; d.frame_next = 0;
    *ct = d;
}

template <bool BOOST>
__global__ __launch_bounds__(256) void k_beam_init(BeamParams p) {
    const int k = blockIdx.x, W = p.W, slot0 = k * nasr_beam::n_slots(W);
    const BeamUtt ud = p.utt[k];
    for (int i = threadIdx.x; i < 4 * HID; i += 256) { p.h[(size_t)slot0 * 4 * HID + i] = 0.f; p.c[(size_t)slot0 * 4 * HID + i] = 0.f; }
    for (int i = threadIdx.x; i < W * JNT; i += 256)
        p.enc[((size_t)k * W + i / JNT) * JNT + i % JNT] = p.encproj[(size_t)ud.enc_row * JNT + i % JNT];
    if (threadIdx.x == 0) {
        Beam bm;
        nasr_beam::beam_begin<BOOST>(bm, ud.T, p.lm_on ? p.lm.start : 0);
        p.beam[k] = bm;
        if (BOOST) p.boost_state[slot0] = nasr_boost::STATE_ROOT;
        beam_fresh_ctrl(&p.ctrl[slot0], BLANK);
        p.rows[k * W].slot = slot0;
        p.dlist[atomicAdd(&p.cnt_next[0], 1)] = k * W;
        p.rowmap[atomicAdd(&p.cnt_next[1], 1)] = (unsigned)(k * W);
    }
}

template <bool LM, bool BOOST>
__global__ __launch_bounds__(256) void k_beam_select(BeamParams p) {
    __shared__ Beam bm;
    __shared__ double ex_lm[LM ? WMAX * KTOP : 1];
    __shared__ int32_t ex_state[LM ? WMAX * KTOP : 1];
    __shared__ nasr_topk::RowTop row_top[WMAX];               // the merge's 8 keys per live hypothesis, named here so that they cannot end up in scratch
    __shared__ float ex_bonus[BOOST ? WMAX * KTOP : 1], row_m[BOOST ? WMAX : 1], row_log_s[BOOST ? WMAX : 1];
    __shared__ int32_t ex_bstate[BOOST ? WMAX * KTOP : 1];
    __shared__ float lb[WMAX], ex_lp[WMAX * KTOP];
    __shared__ int32_t ex_tok[WMAX * KTOP];
    __shared__ int ex_n[WMAX];
    __shared__ nasr_beam::Child ch[WMAX];
    __shared__ nasr_beam::Hyp sel[WMAX];
    __shared__ int n_ch, adv;
    const int k = blockIdx.x, W = p.W, slot0 = k * nasr_beam::n_slots(W);
    if (k == 0 && threadIdx.x < 2) p.cnt_zero[threadIdx.x] = 0;
    const BeamUtt ud = p.utt[k];
    static_assert(sizeof(Beam) % 4 == 0, "the beam is copied word by word");
    for (int i = threadIdx.x; i < (int)(sizeof(Beam) / 4); i += 256)      // all threads copy the beam in and, after the round, out again
        reinterpret_cast<uint32_t *>(&bm)[i] = reinterpret_cast<const uint32_t *>(&p.beam[k])[i];
    __syncthreads();
    if (bm.t >= bm.T) return;                                 // finished (the same answer in every thread)
    if ((int)threadIdx.x < bm.na) {                           // one thread per live hypothesis: its row's ln P(blank) and expansion list
        const int j = threadIdx.x, row = k * W + j;
        const nasr_lp::Part *parts = p.lp_part + nasr_lp::scratch_index(row, 0, nasr_lp::WG_PARTS);
        float m, log_s;
        nasr_topk::row_softmax(parts, nasr_lp::WG_PARTS, &m, &log_s);
        lb[j] = (float)nasr_lp::blank_lp(parts, nasr_lp::WG_PARTS);
        nasr_topk::RowTop &rt = row_top[j];
        nasr_topk::row_begin(rt);
        nasr_topk::row_merge(rt, KTOP, p.alt_key + nasr_topk::scratch_index(row, 0, nasr_lp::WG_PARTS, KTOP), nasr_lp::WG_PARTS);
        if (BOOST) {                                          // the keys hold logit + bonus: only the ids come from them
            ex_n[j] = nasr_beam::expand_ids(rt.top, W, ex_tok + j * KTOP);
            row_m[j] = m; row_log_s[j] = log_s;
        } else ex_n[j] = nasr_beam::expand(rt.top, W, m, log_s, ex_tok + j * KTOP, ex_lp + j * KTOP);
    }
    __syncthreads();
    if (LM || BOOST) {                                        // one thread per (hypothesis, expansion entry)
        const int i = threadIdx.x / KTOP, j = threadIdx.x % KTOP;
        if (i < bm.na && j < ex_n[i]) {
            const int tok = ex_tok[i * KTOP + j];
            if (LM) {                                         // the LM term and the next LM state
                int32_t next = 0;
                ex_lm[i * KTOP + j] = nasr_lm::lookup(p.lm, bm.a[i].lm_state, tok, &next);
                ex_state[i * KTOP + j] = next;
            }
            if (BOOST)                                        // the model's ln P from the raw logit; the bonus and the next automaton state (tok < 1025 < COLS)
                nasr_beam::boost_entry(p.raw_logits[(size_t)(k * W + i) * nasr_boost::COLS + tok], row_m[i], row_log_s[i], p.boost_bonus, p.boost_next,
                                       bm.a[i].boost_state, tok, &ex_lp[i * KTOP + j], &ex_bonus[i * KTOP + j], &ex_bstate[i * KTOP + j]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        bool a = false;
        int n = nasr_beam::round_step_t<LM, BOOST>(bm, W, p.S, p.prune != 0, lb, ex_tok, ex_lp, ex_n, p.nodes + ud.node0, nasr_beam::node_bound(ud.T, W, p.S), ch, &a,
                                                   sel, p.lm_weight, p.lm_bonus, ex_lm, ex_state, ex_bonus, ex_bstate);
        if (n < 0) { *p.err = 1; bm.t = bm.T; n = 0; }       // cannot happen within node_bound; the utterance stops and the host reports it
        n_ch = n; adv = a ? 1 : 0;
        const int live = bm.t < bm.T ? bm.na : 0;
        if (live > 0) {
            const int base = atomicAdd(&p.cnt_next[1], live);
            for (int j = 0; j < live; j++) {
                p.rows[k * W + j].slot = slot0 + bm.a[j].slot;
                if (BOOST) p.boost_state[slot0 + bm.a[j].slot] = bm.a[j].boost_state;
                p.rowmap[base + j] = (unsigned)(k * W + j);
            }
        }
        if (n > 0) {
            const int base = atomicAdd(&p.cnt_next[0], n);
            for (int j = 0; j < n; j++) {
                p.dlist[base + j] = k * W + j;
                beam_fresh_ctrl(&p.ctrl[slot0 + ch[j].slot], ch[j].token);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (int)(sizeof(Beam) / 4); i += 256)
        reinterpret_cast<uint32_t *>(&p.beam[k])[i] = reinterpret_cast<const uint32_t *>(&bm)[i];
    // each child's committed state (version 0 of its slot) = its parent's candidate (version 1 of the parent's slot): h', c' -> h, c
    for (int i = threadIdx.x; i < n_ch * 2 * HID; i += 256) {
        const int j = i / (2 * HID), el = i % (2 * HID);
        const size_t src = ((size_t)(slot0 + ch[j].parent_slot) * 2 + 1) * 2 * HID + el, dst = ((size_t)(slot0 + ch[j].slot) * 2) * 2 * HID + el;
        p.h[dst] = p.h[src];
        p.c[dst] = p.c[src];
    }
    if (adv && bm.t < bm.T)                                   // the next frame's encoder row, once per row of the utterance
        for (int i = threadIdx.x; i < W * JNT; i += 256)
            p.enc[((size_t)k * W + i / JNT) * JNT + i % JNT] = p.encproj[(size_t)(ud.enc_row + bm.t) * JNT + i % JNT];
}

// The N best of Beam_T.  <false, false>: Beam_T's order as it stands and the scores alone (out_lm*, out_total and out_boost are null).  LM: lm_final =
// lm + the EOS term (when some n-gram ends in EOS).  LM or BOOST: one thread re-ranks the <= 8 entries by the final key (final_rank_t, stable, so
// without an LM the order is Beam_T's: it is sorted by score + boost already); the key goes out per hypothesis, with lm and lm_final (LM) and boost (BOOST)
template <bool LM, bool BOOST>
__global__ __launch_bounds__(64) void k_beam_final(BeamParams p) {
    constexpr bool RANK = LM || BOOST;
    __shared__ double lm_final[RANK ? WMAX : 1], total[RANK ? WMAX : 1];
    __shared__ int32_t rank[RANK ? WMAX : 1];
    __shared__ int n_rank;
    const int k = blockIdx.x, r = threadIdx.x;
    const BeamUtt ud = p.utt[k];
    const Beam *bm = &p.beam[k];
    int n_out = bm->na < p.N ? bm->na : p.N, src = r;
    if constexpr (RANK) {
        const int na = bm->na < WMAX ? bm->na : WMAX;
        if (r < na) {
            int32_t next = 0;
            lm_final[r] = LM && p.lm.has_eos ? bm->a[r].lm + nasr_lm::lookup(p.lm, bm->a[r].lm_state, nasr_lm::EOS, &next) : bm->a[r].lm;
        }
        __syncthreads();
        if (r == 0) n_rank = nasr_beam::final_rank_t<LM, BOOST>(bm->a, na, p.N, lm_final, p.lm_weight, p.lm_bonus, rank, total);
        __syncthreads();
        n_out = n_rank;
        if (r < n_out) src = rank[r];
    }
    if (r == 0) p.out_n[k] = bm->t >= bm->T ? n_out : -1;     // -1: the rounds enqueued did not finish the utterance
    if (r >= n_out) return;
    const long long cap = (long long)ud.T * p.S;
    const int len = bm->a[src].len;
    p.out_len[k * WMAX + r] = len;
    p.out_score[k * WMAX + r] = bm->a[src].score;
    if constexpr (LM) { p.out_lm[k * WMAX + r] = bm->a[src].lm; p.out_lm_final[k * WMAX + r] = lm_final[src]; }
    if constexpr (RANK) p.out_total[k * WMAX + r] = total[src];
    if constexpr (BOOST) p.out_boost[k * WMAX + r] = bm->a[src].boost;
    if (len > cap) return;
    const long long at = ud.out0 + (long long)r * cap;
    nasr_beam::backtrace(p.nodes + ud.node0, bm->a[src].node, len, p.out_tok + at, p.out_frame + at, p.out_lp + at);
}

void launch_beam_init(const BeamParams &p, hipStream_t st) {
    if (p.n <= 0) return;
    if (p.boost_on) hipLaunchKernelGGL(k_beam_init<true>, dim3(p.n), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_beam_init<false>, dim3(p.n), dim3(256), 0, st, p);
}
void launch_beam_select(const BeamParams &p, hipStream_t st) {
    if (p.n <= 0) return;
    if (p.boost_on) {
        if (p.lm_on) hipLaunchKernelGGL((k_beam_select<true, true>), dim3(p.n), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((k_beam_select<false, true>), dim3(p.n), dim3(256), 0, st, p);
        return;
    }
    if (p.lm_on) hipLaunchKernelGGL((k_beam_select<true, false>), dim3(p.n), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((k_beam_select<false, false>), dim3(p.n), dim3(256), 0, st, p);
}
void launch_beam_final(const BeamParams &p, hipStream_t st) {
    if (p.n <= 0) return;
    if (p.boost_on) {
        if (p.lm_on) hipLaunchKernelGGL((k_beam_final<true, true>), dim3(p.n), dim3(64), 0, st, p);
        else hipLaunchKernelGGL((k_beam_final<false, true>), dim3(p.n), dim3(64), 0, st, p);
        return;
    }
    if (p.lm_on) hipLaunchKernelGGL((k_beam_final<true, false>), dim3(p.n), dim3(64), 0, st, p);
    else hipLaunchKernelGGL((k_beam_final<false, false>), dim3(p.n), dim3(64), 0, st, p);
}

}  // namespace nasr
