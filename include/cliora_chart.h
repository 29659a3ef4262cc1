/*
 * cliora_chart.h -- C ABI of the MI355X-native DIORA/CLIORA chart engine.
 *
 * Drop-in boundary for ONE path of bobwan1995/cliora: the chart-based
 * inside-outside recursion behind DioraMLP.forward().  The reference has no
 * native code and no FFI; what a maintainer replaces is the body of
 *     cliora/net/diora.py:424-450   DioraBase.forward  (text-only DIORA)
 *     cliora/net/cliora.py:438-468  DioraBase.forward  (CLIORA, vision-language)
 * and the autograd graph torch builds under it (driven from
 *     cliora/net/trainer.py:288     self.diora(embed_span, embed_word, obj_span, obj_word)
 *     cliora/net/trainer.py:450-455 Trainer.gradient_update -> loss.backward()).
 * INTEGRATION.md shows the ctypes stub that binds these entry points.
 *
 * Conventions: plain pointers and sizes only, no torch types.  Every data
 * pointer is a DEVICE pointer to contiguous row-major fp32 unless it says
 * otherwise.  The caller owns every buffer (allocates, frees); the library only
 * reads/writes them and keeps no per-call state outside the plan and the
 * caller's workspaces.  All work is enqueued on `stream` (a hipStream_t passed
 * as void*) and returns without synchronising.  Every function returns 0 on
 * success, a negative CLIORA_E* code otherwise; it never throws.
 * cliora_last_error() gives the message for the calling thread.
 *
 * Chart layout (cliora/net/offset_cache.py:1-7): cell (level, pos) = span of
 * words [pos, pos+level]; id = C - (L-level)(L-level+1)/2 + pos, C = L(L+1)/2.
 */
#ifndef CLIORA_CHART_H
#define CLIORA_CHART_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIORA_OK 0
#define CLIORA_EINVAL (-1)   /* bad argument / unsupported shape */
#define CLIORA_EHIP (-2)     /* a HIP runtime call failed */
#define CLIORA_ENOMEM (-3)   /* workspace too small */

#define CLIORA_NORM_NONE 0   /* cliora/net/utils.py:17-27 NormalizeFunc('none') */
#define CLIORA_NORM_UNIT 1   /* NormalizeFunc('unit'): x / max(||x||, 1e-8)     */

typedef struct cliora_plan cliora_plan;

/* Parameters of DioraMLP in the reference's own shapes (cliora/net/diora.py:453-471):
 *   leaf_w (D,D), leaf_b (D)          inside_compose_func.leaf_fc.{weight,bias}
 *   w1 (D,2D), b1 (D)                 *_compose_func.h_fcs.0.{weight,bias}
 *   w2 (D,D),  b2 (D)                 *_compose_func.h_fcs.2.{weight,bias}
 *   mat (D,D)                         *_score_func.mat
 *   root_h (D)                        root_vector_out_h   (NULL with compress = True: see root_mat below)
 * With share=1 the out_* pointers are ignored (the reference aliases the modules,
 * diora.py:459-461).  The same struct carries gradients (same shapes, written,
 * not accumulated). */
typedef struct cliora_params {
    float *leaf_w, *leaf_b;
    float *in_w1, *in_b1, *in_w2, *in_b2, *in_mat;
    float *out_w1, *out_b1, *out_w2, *out_b2, *out_mat;
    float *root_h;
    /* DioraTreeLSTM only (composition of cliora/net/vg.py:28-76):
     * lstm_w (3D,D) leaf, lstm_u (5D,2D), lstm_b (5D), root_c (D) = root_vector_out_c;
     * share = 0: lstm_u_out (5D,2D), lstm_b_out (5D) = outside_compose_func.{U,B}, and out_mat = outside_score_func.mat
     * (diora.py:459-464 builds a second compose / score module when the functions are not shared) */
    float *lstm_w, *lstm_u, *lstm_b, *root_c;
    float *lstm_u_out, *lstm_b_out;
    /* compress = True (diora.py:342-343, 466-467): root_mat (D,D) = root_mat_out replaces root_h -- the outside root of a
     * sentence is unit(inside_h[root] @ root_mat_out), so the outside pass starts only after the inside pass has ended */
    float *root_mat;
} cliora_params;

/* A plan fixes (batch B, length L, size D, share, normalize, number of image
 * regions R; R = 0 selects text-only DIORA) and owns the small device index
 * tables for that chart shape: per-level (left,right) / (sibling,parent) cell
 * tables (cliora/net/inside_index.py:182-197, outside_index.py:93-127) and the
 * per-cell use lists the backward gathers over.  Creating a plan builds the
 * tables on the host (no GPU needed); they are uploaded by the FIRST forward
 * call that uses the plan, on the device that is current then (one hipMalloc
 * + copy + stream synchronise; cliora_plan_device_bytes tells how much), and
 * every later call must run on that device.  Create and warm plans outside the
 * step loop, or cache them (the reference caches the same tables in Index,
 * cliora/net/utils.py:67-134; cliora_amd/_lib.py keeps an LRU of plans under
 * a byte budget).
 *
 * Sentence length.  L <= 64 for everything that has a backward, for TreeLSTM plans, compress and the sentence-resident kernels (one
 * split of a cell per lane in their score / softmax kernels).  A DioraMLP or CLIORA plan (arch 0; share 0 / 1, normalize unit / none)
 * may also be created for 64 < L <= 128: a LONG plan, FORWARD ONLY.  It builds no use lists, sizes no backward workspace
 * (cliora_plan_bwd_workspace_bytes = 0), no pair-state tail (cliora_plan_pair_states_bytes = 0) and no ReLU bits: 1 300.8 MiB of
 * forward workspace at B 8 / L 128 / D 400 (text-only, shared weights), 8.1 MiB of device tables.  Its score + softmax and the CKY
 * kernels take two splits per lane; the compose, projection and attention kernels are the ones every plan runs.  On a long plan,
 * refused with CLIORA_EINVAL and a message that says why, before any launch:
 *   cliora_chart_forward without CLIORA_FWD_NO_BACKWARD, with CLIORA_FWD_PAIR_STATES, or with params->root_mat (compress);
 *   cliora_chart_forward while cliora_set_resident(1) / CLIORA_RESIDENT=1 forces the sentence-resident kernels on a plan they would
 *   otherwise take (text-only, D <= 64); cliora_chart_backward; cliora_chart_forward_ragged (its root-level mask holds 64 levels:
 *   cliora_chart_forward_ragged_wide runs a long plan) and the four ragged training entries; cliora_plan_create_ex with arch = 1.  cliora_cky_decode, cliora_cky_spans, cliora_cky_spans_ragged, cliora_ground_eval(_ragged),
 *   cliora_phrase_gather and the cliora_vl_scores_* forward entries take L <= 128.  L > 128 is refused at plan creation. */
int cliora_plan_create(int B, int L, int D, int share, int normalize, int R, cliora_plan** out);
/* arch: 0 = DioraMLP (as above), 1 = DioraTreeLSTM (text-only: R = 0) */
int cliora_plan_create_ex(int B, int L, int D, int share, int normalize, int R, int arch, cliora_plan** out);
void cliora_plan_destroy(cliora_plan* plan);

/* Bytes the caller must provide.  fwd workspace: written by forward, must stay
 * untouched until the matching backward.  bwd workspace: scratch. */
size_t cliora_plan_fwd_workspace_bytes(const cliora_plan* plan);
size_t cliora_plan_bwd_workspace_bytes(const cliora_plan* plan);

/* Host view of a plan table (int32), for tests and tooling.  Names:
 * "level_offset", "pair_a_in", "pair_b_in", "pair_a_out", "pair_b_out",
 * "pair_lvl_base_in", "pair_lvl_base_out", "use_off_<role>", "use_row_<role>",
 * "use_stride_<role>", "use_partner_<role>" with role in {ina, inb, outa, outb};
 * "tile_base_in", "tile_base_out" (L + 1 each): first 16-row tile of a level's pair rows in the
 * tiled split-bf16 operand form of the pair rows' weight gradient (csrc/wgrad_tiles.hpp), per pass.
 * Works without a GPU. */
int cliora_plan_table(const cliora_plan* plan, const char* name, const int32_t** data, size_t* count);

/* Forward: DioraBase.forward -- leaf transform, inside pass, and (run_outside != 0)
 * root init + outside pass (diora.py:283-398).
 *   x_span     (B,L,D)   in
 *   obj_span   (B,R,D)   in, CLIORA only (else NULL)
 *   drop_mask  CLIORA training only: pre-scaled dropout mask (0 or 1/(1-p)) of the
 *              AttentionHead (cliora.py:32,40) for every inside cell, laid out like the chart:
 *              (B,C,R), leaves first; NULL = no dropout (eval)
 *   inside_h/outside_h (B,C,D), inside_s/outside_s (B,C)   out
 *   inside_c   (B,C,D)   out, CLIORA only (else NULL): unit(context) at the leaves, 0 above
 * For DioraMLP the c charts are identically zero (diora.py:70); the caller zero-fills
 * them once, they are not touched here.
 * run_outside is a flag word: bit 0 = run the outside pass; CLIORA_FWD_NO_BACKWARD = no backward call will follow
 * (torch.no_grad / eval): the per-pair state the backward needs is not written (hooks need the default). */
#define CLIORA_FWD_NO_BACKWARD 2
/* CLIORA_FWD_PAIR_STATES: also write the un-aggregated compose outputs of every pair (what inside_hook / outside_hook receive,
 * diora.py:295-334, 364-398) into the TAIL of the workspace: the caller then passes a workspace of
 * cliora_plan_fwd_workspace_bytes() + cliora_plan_pair_states_bytes() bytes.  Without it no per-pair vector is stored. */
#define CLIORA_FWD_PAIR_STATES 4
size_t cliora_plan_pair_states_bytes(const cliora_plan* plan);
int cliora_chart_forward(cliora_plan* plan, const cliora_params* params,
                         const float* x_span, const float* obj_span, const float* drop_mask,
                         float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                         float* inside_c,
                         void* fwd_workspace, size_t fwd_workspace_bytes,
                         int run_outside, void* stream);

/* Backward of the call above (what torch.autograd replays through diora.py:295-398).
 * d_* are the cotangents of the four chart outputs (any may be NULL = zero).
 * Writes d_x_span (B,L,D), d_obj_span (B,R,D, CLIORA) and every field of `grads`
 * that is non-NULL (shared weights: inside+outside contributions summed into in_*). */
int cliora_chart_backward(cliora_plan* plan, const cliora_params* params,
                          const float* x_span, const float* obj_span, const float* drop_mask,
                          const float* inside_h, const float* inside_s,
                          const float* outside_h, const float* outside_s,
                          const float* d_inside_h, const float* d_inside_s,
                          const float* d_outside_h, const float* d_outside_s,
                          void* fwd_workspace, size_t fwd_workspace_bytes,
                          void* bwd_workspace, size_t bwd_workspace_bytes,
                          float* d_x_span, float* d_obj_span, const cliora_params* grads,
                          int ran_outside, void* stream);
/* cliora_chart_backward with one more cotangent: d_split_s, on the per-split INSIDE scores before the softmax -- the rows
 * cliora_bracket_grad writes, cliora_plan_split_score_count floats: row B * lvl_base[level] + (b * (L - level) + pos) * level + k for
 * split k of cell (level, pos) of sentence b.  NULL = zero, and the call is then cliora_chart_backward itself (which is this entry
 * called with NULL): the same launches, the same bits.  Otherwise the row is added to the score gradient where the inside chain's
 * softmax backward forms it, so that everything downstream of a split score sees the sum; a plan the
 * sentence-resident kernels would take runs the launch path for such a call (either path runs on either path's workspace).  Refused
 * as cliora_chart_backward refuses: TreeLSTM plans (cliora_lstm_backward takes no such input), long plans, a missing forward. */
int cliora_chart_backward_split(cliora_plan* plan, const cliora_params* params,
                                const float* x_span, const float* obj_span, const float* drop_mask,
                                const float* inside_h, const float* inside_s,
                                const float* outside_h, const float* outside_s,
                                const float* d_inside_h, const float* d_inside_s,
                                const float* d_outside_h, const float* d_outside_s, const float* d_split_s,
                                void* fwd_workspace, size_t fwd_workspace_bytes,
                                void* bwd_workspace, size_t bwd_workspace_bytes,
                                float* d_x_span, float* d_obj_span, const cliora_params* grads,
                                int ran_outside, void* stream);

/* Hard (single-tree, S-DIORA) chart of a text-only DioraMLP plan: every cell encodes its single best split instead of the softmax
 * mixture.  Per cell of a level the split scores are those of cliora_chart_forward; then, with k the LOWEST split that attains their
 * maximum: the weight row is one-hot at k, h = unit(y_k) (the compose output of pair k alone) and s = s_k.  Only the selected pair of
 * a cell is composed (level_compose_hard: B * Lc rows per level instead of B * Lc * N).
 *   sel_in / sel_out  (B, C) int32 each, caller-owned: k per cell of the inside / outside chart.  The leaves of sel_in and the root of
 *                     sel_out -- and all of sel_out without an outside pass -- are not written.
 *   flags             bit 0 = run the outside pass, CLIORA_FWD_NO_BACKWARD, CLIORA_FWD_HARD_DENSE
 * The workspace is that of cliora_chart_forward (cliora_plan_fwd_workspace_bytes, same layout); the backward is cliora_chart_backward
 * / _split on it, unchanged: with a one-hot weight row its softmax backward gives dS at the selected split and 0 elsewhere, its compose
 * backward the gradient of the selected pair alone -- the gradient of "h = unit(y_k), s = s_k" with k held fixed.  The decodes that
 * read the split scores (cliora_cky_spans, ...) work on such a workspace as on any other.
 * Runs the per-level launch path on the caller's stream whatever cliora_set_wavefront / cliora_set_resident say.
 * Refused before any launch: TreeLSTM plans, plans with regions (R > 0), compress (root_mat), CLIORA_FWD_PAIR_STATES, a long plan
 * (L > 64) without CLIORA_FWD_NO_BACKWARD, NULL selection arrays.
 * CLIORA_FWD_HARD_DENSE: the same one-hot weights through the dense compose kernels of cliora_chart_forward (every split composed and
 * multiplied by 0 or 1) -- the on-device cross-check and the benchmark's baseline; same outputs, bit for bit. */
#define CLIORA_FWD_HARD_DENSE 16
int cliora_chart_forward_hard(cliora_plan* plan, const cliora_params* params, const float* x_span,
                              float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                              int32_t* sel_in, int32_t* sel_out,
                              void* fwd_workspace, size_t fwd_workspace_bytes, int flags, void* stream);
/* The tree of a hard chart from its inside selections, no CKY pass: spans (B, L-1, 2) int32 device in the layout of cliora_cky_spans
 * (children before parents, left subtree first, the root last).  One wave per sentence walks from the root with an explicit stack.
 * Nothing is written for L < 2. */
int cliora_hard_spans(cliora_plan* plan, const int32_t* sel_in, int32_t* spans, void* stream);

/* The hard chart of sentences of DIFFERENT lengths that share one right-padded chart of length L: what
 * cliora_chart_forward_ragged (lengths, status: as there; root_levels: two words in host memory, as cliora_chart_forward_ragged_wide
 * takes them) is to cliora_chart_forward, for cliora_chart_forward_hard.  ONE entry for inference and training:
 *   with CLIORA_FWD_NO_BACKWARD   plans of L <= 128 (a long plan runs the long instances of the hard score / projection kernels)
 *   without it                    plans of L <= 64; the state the backward reads is written, ReLU bits included, and the backward is
 *                                 cliora_chart_backward_ragged on that workspace, unchanged
 *   CLIORA_FWD_HARD_DENSE         as in cliora_chart_forward_hard: same outputs, bit for bit
 * On every cell of sentence b's own triangle (pos + level < lengths[b]) the four charts hold what cliora_chart_forward_hard computes for
 * that sentence alone at its exact length, to rounding, and the selections are that chart's with its numbering: the valid outside
 * pairs of a cell are its first lengths[b] - level - 1, so an index means the same pair at either length and the lowest-maximum tie
 * rule carries over.  Cells beyond a triangle are unspecified in the four charts (inside_s holds -1e30 there).  EVERY entry of the two
 * selection arrays is written: the split on the cells of a triangle above the leaves (sel_in) / other than the sentence's root
 * (lengths[b] - 1, 0) (sel_out), -1 everywhere else -- leaves, outside roots, beyond the triangles, all of sel_out without an outside
 * pass.  Schedule: hard inside levels, mask, root, hard outside levels with the seed fix-up and a re-scoring of the level below after
 * each level that holds some sentence's root, then the -1 fill; all on the caller's stream.  With every length equal to L the charts
 * and the selections are bitwise those of cliora_chart_forward_hard.
 * Refused with CLIORA_EINVAL and a message that starts with the entry's name, each before any HIP call: a NULL plan, params, lengths,
 * root_levels or status; NULL selection arrays; TreeLSTM plans; plans with regions (R > 0); params->root_mat (compress);
 * CLIORA_FWD_PAIR_STATES; unknown flag bits; a long plan without CLIORA_FWD_NO_BACKWARD; a bit of root_levels set at or above L (bit
 * L - 1 is legal and ignored).  There is no drop_mask argument (text-only DIORA has no attention dropout).  status counts the lengths
 * outside [1, L]; the cells and selections of such a sentence are unspecified (nothing is read or written out of bounds). */
int cliora_chart_forward_ragged_hard(cliora_plan* plan, const cliora_params* params, const float* x_span,
                                     float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                                     int32_t* sel_in, int32_t* sel_out,
                                     void* fwd_workspace, size_t fwd_workspace_bytes, int flags,
                                     const int32_t* lengths, const uint64_t* root_levels, int32_t* status, void* stream);
/* cliora_hard_spans with a length per sentence: sentence b is walked from its own root (lengths[b] - 1, 0) with the padded chart's cell
 * ids -- lengths[b] - 1 rows in cliora_cky_spans_ragged's layout (the root last), (-1, -1) beyond.  sel_in: of
 * cliora_chart_forward_ragged_hard, or of cliora_chart_forward_hard on the padded batch (the inside pass is prefix-closed).  status (an
 * int32 on the device, zeroed by the call) counts the lengths outside [1, L]; such a sentence gets -1 in every row.  With every length
 * equal to L the spans are bitwise those of cliora_hard_spans (the same kernel, given lengths). */
int cliora_hard_spans_ragged(cliora_plan* plan, const int32_t* sel_in, const int32_t* lengths, int32_t* spans, int32_t* status,
                             void* stream);

/* DioraTreeLSTM (BASELINE config 5).  PARITY UNPINNED: the reference ships this composition only
 * as commented-out text (cliora/net/vg.py:28-76); what is implemented is that text on the
 * DioraBase skeleton (cliora/net/diora.py:283-398), constant = 1 inside / 0 outside (diora.py:174),
 * root_vector_out_c a parameter (the hint at diora.py:470-471).  Same conventions as
 * cliora_chart_forward / _backward; here the cell-state charts inside_c / outside_c (B,C,D) are
 * real outputs with cotangents.  Uses lstm_w, lstm_u, lstm_b, in_mat, root_h, root_c of `params`. */
int cliora_lstm_forward(cliora_plan* plan, const cliora_params* params, const float* x_span,
                        float* inside_h, float* inside_c, float* inside_s,
                        float* outside_h, float* outside_c, float* outside_s,
                        void* fwd_workspace, size_t fwd_workspace_bytes, int run_outside, void* stream);
int cliora_lstm_backward(cliora_plan* plan, const cliora_params* params, const float* x_span,
                         const float* inside_h, const float* inside_c, const float* inside_s,
                         const float* outside_h, const float* outside_c, const float* outside_s,
                         const float* d_inside_h, const float* d_inside_c, const float* d_inside_s,
                         const float* d_outside_h, const float* d_outside_c, const float* d_outside_s,
                         void* fwd_workspace, size_t fwd_workspace_bytes,
                         void* bwd_workspace, size_t bwd_workspace_bytes,
                         float* d_x_span, const cliora_params* grads, int ran_outside, void* stream);

/* CLIORA span-region / word-region scorers (cliora/net/cliora.py:453-468):
 *   all_atten (B,B,C,R) = einsum('abx,cdx->acbd', inside_h + outside_h, obj_span)
 *   training != 0:  vg_atten (B,B,L,R) = einsum('abx,cdx->acbd', x_word, obj_word)
 *   training == 0:  vg_atten = all_atten[:, :, :L] + einsum(unit(x_word), obj_word)
 * (atten_score is the a == c diagonal of vg_atten: a view, left to the caller.)
 * Backward: d_sum_h (B,C,D) is the gradient w.r.t. (inside_h + outside_h) -- it goes to both
 * charts; d_obj_span, d_obj_word (B,R,D), d_x_word (B,L,D; training mode only).  NULL cotangents
 * are zero; NULL outputs are skipped. */
size_t cliora_plan_vl_workspace_bytes(const cliora_plan* plan);
/* all_atten may be NULL in training mode (only vg_atten is wanted: the contrastive loss takes cliora_vl_scores_max_forward). */
int cliora_vl_scores_forward(cliora_plan* plan, const float* inside_h, const float* outside_h,
                             const float* obj_span, const float* x_word, const float* obj_word,
                             int training, float* all_atten, float* vg_atten,
                             void* vl_workspace, size_t vl_workspace_bytes, void* stream);
int cliora_vl_scores_backward(cliora_plan* plan, const float* inside_h, const float* outside_h,
                              const float* obj_span, const float* x_word, const float* obj_word,
                              int training, const float* d_all_atten, const float* d_vg_atten,
                              float* d_sum_h, float* d_obj_span, float* d_x_word, float* d_obj_word,
                              void* vl_workspace, size_t vl_workspace_bytes, void* stream);

/* The same span-region scores reduced over the R regions of each image, as ContrastiveLoss consumes them
 * (cliora/net/trainer.py:101 `all_atten_score.max(-1).values`): the (B,B,C,R) tensor (124 MB at B 64, L 20, R 36) is never
 * written -- the GEMM's epilogue keeps, per (sentence a, image c, span b), the largest score and the smallest region index
 * that attains it (what torch.max returns):
 *   all_max (B,B,C) float, all_arg (B,B,C) int32
 * Backward: the cotangent of all_max flows to the arg-max region only (torch's max backward); d_sum_h (B,C,D) as above,
 * d_obj_span (B,R,D).  NULL outputs are skipped.  Uses the same workspace as cliora_vl_scores_forward. */
int cliora_vl_scores_max_forward(cliora_plan* plan, const float* inside_h, const float* outside_h, const float* obj_span,
                                 float* all_max, int32_t* all_arg, void* vl_workspace, size_t vl_workspace_bytes, void* stream);
int cliora_vl_scores_max_backward(cliora_plan* plan, const float* inside_h, const float* outside_h, const float* obj_span,
                                  const float* d_all_max, const int32_t* all_arg, float* d_sum_h, float* d_obj_span,
                                  void* vl_workspace, size_t vl_workspace_bytes, void* stream);

/* ContrastiveLoss after the region max (cliora/net/trainer.py:103-128), one launch per direction:
 *   s[b][a][c] = all_max[a][c][b];  txt = clamp(margin + s - s[b][a][a], min=1e-8), img = clamp(margin + s - s[b][c][c], min=1e-8),
 *   both zero on a == c;  vl[a][b] = mean_c txt[b][a][c] + mean_a' img[b][a'][a];  marg[a][b] = exp(in_s + out_s - in_s[a][C-1]);
 *   loss = alpha * mean_a sum_{b < C/2} marg[a][b] * vl[a][b]
 * all_max (B,B,C), inside_s / outside_s (B,C).  The forward also leaves the gradient of the loss w.r.t. its three inputs (for an
 * upstream cotangent of 1) in d_all_max (B,B,C), d_inside_s, d_outside_s (B,C): the caller scales them by the cotangent it
 * receives.  B <= 128.  workspace: cliora_contrastive_workspace_bytes(B, C). */
size_t cliora_contrastive_workspace_bytes(int B, int C);
int cliora_contrastive_loss(int B, int C, const float* all_max, const float* inside_s, const float* outside_s, float margin,
                            float alpha, float* loss, float* d_all_max, float* d_inside_s, float* d_outside_s, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The same loss over B right-padded sentences of lengths[b] words in a chart of length L, C = L (L + 1) / 2.
 * Sentence x owns the cells (level, pos) with pos + level < lengths[x]; such a cell is number level n - level (level - 1) / 2 + pos of
 * its own chart of C_x = n (n + 1) / 2 cells, and half(x) is the cells whose number is below C_x / 2 (none for one word).  For x and a
 * cell of half(x):  txt = (1/B) sum_{y != x} max(margin + s[x][y] - s[x][x], 1e-8) over every image;  img = (1/B) sum over the texts
 * a != x THAT OWN THE CELL of max(margin + s[a][x] - s[x][x], 1e-8) -- the divisor stays B;  marg = exp(in_s + out_s - in_s[x][root(x)])
 * with root(x) the cell (lengths[x] - 1, 0);  loss = alpha / B * sum_x sum_{half(x)} marg (txt + img).  Nothing beyond a triangle is
 * read into a sum (selected, not multiplied by a mask: NaN there does not leak) and every gradient there is exactly 0.  Fixed
 * summation order; with every length = L the results are bitwise cliora_contrastive_loss's.  B <= 128.
 * workspace: 256 + cliora_contrastive_workspace_bytes(B, 2 * C) bytes; its first int32 is the STATUS WORD: the number of lengths outside
 * [1, L].  Such a sentence owns no cell -- nothing is written for it -- and its image still stands as a negative for the others. */
int cliora_contrastive_loss_ragged(int B, int C, const float* all_max, const float* inside_s, const float* outside_s,
                                   const int32_t* lengths, float margin, float alpha, float* loss, float* d_all_max, float* d_inside_s,
                                   float* d_outside_s, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the callers either side of the chart, as kernels of this library ----
 *
 * Projection of (optionally looked-up) rows: y (nrows, D) = gather(x, index) w^T + bias.
 *   Embed.forward (cliora/net/trainer.py:219-224): x = embeddings.weight (V, K), index = the batch's token ids (nrows = B*L,
 *     int64), w = mat or mat1 (D, K), bias = NULL;
 *   ImageEncoder.forward (cliora/net/utils.py:52-55): x = obj_feats (nrows = B*R, K = 2048), index = NULL, w / bias = fc or fc_vis.
 * K must be a multiple of 16.  Backward: d_w (D, K), d_bias (D), d_rows (nrows, K) = gradient of the looked-up rows (the
 * caller scatters it into the table's gradient); any of them may be NULL.  Exact fp32 products (fp32-input MFMA). */
size_t cliora_proj_workspace_bytes(int nrows, int K, int D);
int cliora_proj_forward(const float* x, const int64_t* index, int nrows, int K, const float* w, const float* bias, int D,
                        float* y, void* workspace, size_t workspace_bytes, void* stream);
int cliora_proj_backward(const float* x, const int64_t* index, int nrows, int K, const float* w, const float* d_y, int D,
                         float* d_w, float* d_bias, float* d_rows, void* workspace, size_t workspace_bytes, void* stream);

/* Gradient of an embedding table from the gradients of its looked-up rows -- what autograd does behind F.embedding
 * (cliora/net/trainer.py:219, :54-58; the table trains when emb = none: cliora/data/embeddings.py:164):
 *   table_grad (V, K) = 0;  table_grad[index[i]] += rows[i], i < n      (index int64, K a multiple of 4; ids outside [0, V) are skipped)
 * Repeated ids add up in ascending i, without atomics: bitwise reproducible. */
int cliora_rows_scatter_add(const float* rows, const int64_t* index, int n, int K, float* table_grad, int64_t V, void* stream);
/* The same with the looked-up rows in up to 4 segments (rows[s] (n[s], K), index[s] (n[s])), as ONE zero-fill + ONE launch: a training
 * step reaches the table through several lookups (trainer.py:54-58 positives and negatives of the reconstruction loss, :219 Embed), and
 * autograd would scatter each into its own dense (V, K) tensor and add them.  Row order = segment order, then row order inside a
 * segment; repeated ids add up in that order, bitwise reproducible.  (Host arrays of device pointers.) */
int cliora_rows_scatter_add_segments(const float* const* rows, const int64_t* const* index, const int* n, int nseg, int K, float* table_grad,
                                     int64_t V, void* stream);

/* ReconstructionSoftmaxLoss.forward (cliora/net/trainer.py:46-78): tokens (B*L) and neg (Kn) int64 ids into emb (V, E), mat (D, E),
 * outside_h (B, C, D) of which the leaf cells [:, :L] are read:
 *   proj = emb[ids] mat^T;  logits_r = [proj_pos_r . cell_r | cell_r proj_neg^T];  loss = mean_r CE(logits_r, 0)
 * E must be a multiple of 16.  The backward runs on the SAME workspace (it keeps the projections and the softmax): gscale is the
 * upstream cotangent (a device scalar); d_cell (B*L, D) is the gradient of outside_h[:, :L], d_mat (D, E), d_rows (B*L + Kn, E)
 * the gradient of the looked-up embedding rows (tokens first, then negatives; NULL when the embeddings are frozen). */
size_t cliora_recon_workspace_bytes(int n_tokens, int Kn, int E, int D);
int cliora_recon_forward(const int64_t* tokens, const int64_t* neg, int B, int L, int C, int Kn, const float* emb, int E,
                         const float* mat, int D, const float* outside_h, float* loss, void* workspace, size_t workspace_bytes,
                         void* stream);
int cliora_recon_backward(const int64_t* tokens, const int64_t* neg, int B, int L, int C, int Kn, const float* emb, int E,
                          const float* mat, int D, const float* outside_h, const float* gscale, float* d_cell, float* d_mat,
                          float* d_rows, void* workspace, size_t workspace_bytes, void* stream);

/* VGLoss.forward (cliora/net/trainer.py:139-171, variant V1): vg_atten (B, B, L, R);
 *   logits[a][c] = sum_l max_r vg_atten[a][c][l][r] / L;  loss = alpha * cross_entropy(logits, arange(B))
 * The forward also leaves the gradient of the loss w.r.t. vg_atten (for an upstream cotangent of 1; it flows to the arg-max region
 * of each word, the smallest index on ties) in d_vg_atten (B, B, L, R), or skips it when NULL. */
size_t cliora_vg_workspace_bytes(int B, int L);
int cliora_vg_loss(int B, int L, int R, const float* vg_atten, float alpha, float* loss, float* d_vg_atten, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The same loss over right-padded sentences of lengths[a] words:  logits[a][c] = sum_{l < lengths[a]} max_r vg_atten[a][c][l][r] /
 * lengths[a].  d_vg_atten[a][:][l][:] is exactly 0 for l >= lengths[a], and nothing there is read.  Same summation order: with every
 * length = L the results are bitwise cliora_vg_loss's.  workspace: 256 + cliora_vg_workspace_bytes(B, L) bytes; its first int32 is
 * the STATUS WORD: the number of lengths outside [1, L].  Such a sentence has no row in the cross entropy (the mean's divisor stays
 * B) and a zero gradient; its image still stands as a negative for the others. */
int cliora_vg_loss_ragged(int B, int L, int R, const float* vg_atten, const int32_t* lengths, float alpha, float* loss,
                          float* d_vg_atten, void* workspace, size_t workspace_bytes, void* stream);

/* Trainer.gradient_update (cliora/net/trainer.py:450-455): torch.nn.utils.clip_grad_norm_(params, max_norm) followed by one
 * torch.optim.Adam step (no weight decay, no amsgrad), over ONE flat fp32 buffer holding every parameter (and one holding every
 * gradient, e.g. the buffer the data-parallel all-reduce works on): three launches whatever the number of parameters.  `step`
 * counts from 1.  grads are left clipped, as clip_grad_norm_ leaves them. */
size_t cliora_clip_adam_workspace_bytes(void);
int cliora_clip_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float max_norm, float lr, float beta1,
                     float beta2, float eps, int step, void* workspace, size_t workspace_bytes, void* stream);

/* Un-aggregated per-split tensors the reference hands to inside_hook (diora.py:295-334)
 * for `level`: scores = (B, L-level, level) laid out exactly like the reference's
 * s.view(B, Lc, N, 1); h = the compose outputs, `rows` = B*(L-level)*level rows of D
 * valid floats with row stride `ldh`, same row order as the reference's h (M, D).
 * Both are device pointers into the fwd workspace (h: into its CLIORA_FWD_PAIR_STATES tail; the forward must have run
 * with that flag). */
int cliora_inside_pair_states(const cliora_plan* plan, void* fwd_workspace, int level,
                              const float** scores, const float** h, size_t* rows, size_t* ldh);

/* The same for the outside pass (what the reference hands to outside_hook, diora.py:364-398), for target `level`
 * (0 <= level <= L-2): `rows` = B*(L-level)*(L-level-1) rows in THIS library's split order
 * [sentence][target position j][split n]; the reference's order is [sentence][split i][target position j] with
 *   n = L-2-i-level  if j < (L-level-1) - i,   else n = (L-level-1) - i - 1
 * (cliora/net/outside_index.py:39-62; cliora_amd/index.py::Index.get_outside_index applies it). */
int cliora_outside_pair_states(const cliora_plan* plan, void* fwd_workspace, int level,
                               const float** scores, const float** h, size_t* rows, size_t* ldh);

/* CKY decode (cliora/analysis/cky.py:31-99 + analysis/utils.py:78-95): best binary
 * tree per sentence from the inside per-split scores of the last forward; first
 * maximum wins.  split_out (B, C) int32 device: chosen split n per cell (leaves -1);
 * the tree is rebuilt from it on the host. */
int cliora_cky_decode(cliora_plan* plan, void* fwd_workspace, int32_t* split_out, void* stream);
/* The same decode, with the tree's constituent spans emitted on the device: spans_out (B, L-1, 2) int32 device = (start, end) word
 * positions, children before parents, left subtree first, the root last -- the list the reference builds on the host with
 * get_spans(get_actions(tree)) (cliora/analysis/utils.py:3-49; what scripts/train.py:184-204 scores F1 on): evaluation needs ONE
 * device-to-host copy of B*(L-1)*2 ints and no recursion over a split table.  split_out: as cliora_cky_decode, or NULL. */
int cliora_cky_spans(cliora_plan* plan, void* fwd_workspace, int32_t* split_out, int32_t* spans_out, void* stream);
/* The decode for sentences of DIFFERENT lengths that were run as one batch, each padded on the right to the plan's L.  The inside
 * pass is prefix-closed -- cell (level, pos) with pos + level < n reads only cells of words [0, n) -- so sentence b's own triangle of
 * the padded chart holds what a chart of length n = lengths[b] would ("Mixed-length batches"); nothing here reads the
 * outside pass (cliora_chart_forward_ragged makes that one the sentence's own too).  One workgroup per sentence evaluates levels
 * 1 .. n-1 at positions pos < n - level only (the same candidate in the same order as cliora_cky_spans, first maximum wins) and
 * walks from cell (n-1, 0).
 *   lengths (B) int32 device.  spans_out (B, L-1, 2): the first n-1 rows are the sentence's spans in cliora_cky_spans' order, the
 *   root (0, n-1) last; the remaining rows are (-1, -1).  split_out (B, C) or NULL: -1 at the leaves and outside the triangle.
 *   A length outside [1, L] is not decoded: every row of that sentence is -1 and it is counted in *status (an int32 on the device the
 *   call zeroes first), which the caller must check.  With lengths[b] == L for every b the outputs are those of cliora_cky_spans. */
int cliora_cky_spans_ragged(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, int32_t* split_out, int32_t* spans_out,
                            int32_t* status, void* stream);
/* Span posteriors, log-partition and minimum-Bayes-risk (MBR) tree: the SUM-product pass over the potentials whose MAX-product is
 * cliora_cky_spans.  Per cell, r[cell, k] = score[cell, k] - max_k score[cell, .] (the per-split inside scores of the last forward);
 * a binary tree over the sentence weighs exp(sum of r over its internal cells and their splits).  Per sentence of n words:
 *   inside   a[leaf] = 0,  a[cell] = logsumexp_k(a[left] + a[right] + r[cell, k]);      log_z = a[(n-1, 0)]
 *   outside  b[(n-1, 0)] = 0,  b[cell] = logsumexp over the n-1-level (parent, sibling) uses of b[parent] + a[sibling] + r[parent, k]
 *   mu[cell] = exp(a + b - log_z): the probability that the span is a constituent (1 at the leaves and at the sentence's root)
 *   MBR      v[leaf] = 0,  v[cell] = max_k(v[left] + v[right]) + mu[cell] in fp32, first maximum wins: the tree with the most
 *            expected correct brackets.
 * The reference has no counterpart; the distribution is the one whose mode its parser returns.  One workgroup per sentence, gather
 * form, a and b in fp64, fixed-order reductions, no floating-point atomics: two calls give equal bits.
 *   lengths (B) int32 device, or NULL: every sentence has L words.  Otherwise the sentences share a right-padded chart, with the
 *     rules of cliora_cky_spans_ragged: `status` (an int32 on the device, zeroed by the call) is required and counts the lengths
 *     outside [1, L]; such a sentence gets mu = 0, log_z = 0, every MBR row -1, and none of its scores is read.  With every length
 *     equal to L the outputs are bitwise those of the lengths == NULL call.  status may be NULL when lengths is.
 *   marginals (B, C) fp32: mu in the cell order of inside_s, exactly 0 outside a sentence's triangle.  log_z (B) fp32.
 *   mbr_split (B, C) or NULL: the MBR split per cell, -1 at the leaves and outside the triangle.  mbr_spans (B, L-1, 2) or NULL: the
 *     n - 1 spans of the MBR tree in cliora_cky_spans' order, the root last, (-1, -1) beyond.  Both NULL: the MBR pass is skipped.
 *   scratch: device memory of cliora_span_posteriors_scratch_bytes(plan) bytes; NULL when that is 0 (as it is for every plan today:
 *     the tables fit the LDS up to L = 128, 131 KiB there).
 * Every plan cliora_cky_spans takes is taken: long plans (two splits / uses per lane) and TreeLSTM plans (the same score rows).
 * Refused with CLIORA_EINVAL and a message, before any launch: a NULL plan, workspace, marginals or log_z; lengths without status; a
 * plan that has not run a forward. */
size_t cliora_span_posteriors_scratch_bytes(const cliora_plan* plan);
int cliora_span_posteriors(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, float* marginals, float* log_z,
                           int32_t* mbr_split, int32_t* mbr_spans, void* scratch, int32_t* status, void* stream);
/* The K best binary trees per sentence over the potentials of cliora_cky_spans and cliora_span_posteriors: r[cell, k] = score[cell, k]
 * - max_k score[cell, .], a tree scores the sum of r over its internal cells (so exp(score - log_z) is its posterior mass).  The
 * order is the contract: every cell holds at most K derivations (value, split k, left rank i, right rank j);
 * a leaf holds one, value 1.0f; a candidate is (val_left[i] + val_right[j]) + (s_k - smax) in fp32, in that order; a cell's list is the
 * first K candidates by value descending, then split, left rank, right rank ascending.  Rank 0 is cliora_cky_spans' tree; no tree
 * appears twice.  One workgroup per sentence, fixed-order reductions, no floating-point atomics: two calls give equal bits.
 *   K: 1 .. 16.  lengths (B) int32 device, or NULL: every sentence has L words.  Otherwise the sentences share a right-padded chart,
 *     with the rules of cliora_cky_spans_ragged: `status` (an int32 on the device, zeroed by the call) is required and counts the
 *     lengths outside [1, L]; such a sentence gets count 0, scores -inf, every row -1, and none of its scores is read.  With every
 *     length equal to L the outputs are bitwise those of the lengths == NULL call.  status may be NULL when lengths is.
 *   count_out (B): min(K, Catalan(n - 1)) trees.  scores_out (B, K) fp32: root value - (float)n, -inf beyond count.  spans_out
 *     (B, K, L-1, 2) (may be NULL when L = 1): tree t's n - 1 spans in cliora_cky_spans' order, the root last; (-1, -1) beyond a
 *     tree's n - 1 rows and beyond count.
 *   scratch: device memory of cliora_kbest_scratch_bytes(plan, K) bytes -- 0 when the lists (8 C K bytes per sentence) fit the LDS
 *     beside the walk stacks, else B of them; NULL when that is 0.
 * Every plan cliora_cky_spans takes is taken: long plans, padded charts, TreeLSTM plans.  Refused with CLIORA_EINVAL and a message,
 * before any launch: K outside 1..16; a NULL plan, workspace or output; lengths without status; NULL scratch when the query is not 0;
 * a plan that has not run a forward.  Scores that are NaN or infinite give unspecified trees (inside the sentence). */
size_t cliora_kbest_scratch_bytes(const cliora_plan* plan, int K);
int cliora_kbest_spans(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, int K, int32_t* spans_out, float* scores_out,
                       int32_t* count_out, void* scratch, int32_t* status, void* stream);
/* Binary trees SAMPLED from the distribution whose mode is cliora_cky_spans' tree and whose marginals cliora_span_posteriors returns:
 * r[cell, k] = score[cell, k] - max_k score[cell, .], scaled by an inverse temperature beta >= 0, so a tree weighs exp(beta * sum of
 * r over its internal cells) -- beta = 1 is that posterior, beta = 0 is uniform over the Catalan(n - 1) trees.  Per sentence of n
 * words:
 *   inside   a[leaf] = 0,  a[cell] = logsumexp_k(a[left] + a[right] + beta r[cell, k]) in fp64, beta r formed in fp64;
 *            log_z = a[(n-1, 0)] -- at beta = 1 the log_z of cliora_span_posteriors, bit for bit.
 *   draws    sample s walks from the root; at an internal cell (level, pos) with N = level splits,
 *              w_k = exp(a[left_k] + a[right_k] + beta r_k - a[cell]),  c_k = w_0 + .. + w_k,
 *              split = the number of k with c_k <= u c_{N-1}, clamped to N - 1,
 *              u = (m + 0.5) 2^-53, m = (x0 >> 5) 2^26 + (x1 >> 6), x = Philox4x32-10 of counter (level * 256 + pos, sample_lo,
 *              sample_hi, sentence id) under key (seed_lo, seed_hi): the uniform of cliora_neg_sample.
 *            So a draw depends on (seed, sentence id, sample index, cell) and the sentence's scores alone -- not on B, the padding,
 *            the pack a sentence landed in, or how a caller chunks S.  Sample index = first_sample + s.
 *   lengths (B) int32 device, or NULL: every sentence has L words.  Otherwise the sentences share a right-padded chart, with the
 *     rules of cliora_cky_spans_ragged: `status` (an int32 on the device, zeroed by the call) is required and counts the lengths
 *     outside [1, L]; such a sentence gets every row -1, log_prob 0, log_z 0, and none of its scores is read.  With every length
 *     equal to L the outputs are bitwise those of the lengths == NULL call.  status may be NULL when lengths is.
 *   ids (B) int32 device, or NULL: the caller's sentence numbers (NULL: sentence id = b), so that a sentence keeps its draws
 *     wherever a pack puts it.
 *   spans_out (B, S, L-1, 2) (may be NULL when L = 1): sample s's n - 1 spans in cliora_cky_spans' order, the root last; (-1, -1)
 *     beyond.  log_prob_out (B, S) fp32: beta * (sum of r over the chosen splits) - log_z, summed in fp64.  log_z_out (B) fp32.
 * One workgroup per sentence, a wavefront per sample, fixed-order scans, no floating-point atomics: two calls give equal bits.  The
 * tables fit the LDS up to L = 128 (81 KiB there): no scratch.  Every plan cliora_cky_spans takes is taken: long plans, padded
 * charts, TreeLSTM plans.  Refused with CLIORA_EINVAL and a message, before any launch: S outside 1 .. 2^20; beta negative or not
 * finite; a NULL plan, workspace, log_prob_out or log_z_out; NULL spans_out with L > 1; lengths without status; a plan that has not
 * run a forward. */
int cliora_sample_trees(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const int32_t* ids, int S, uint64_t seed,
                        uint64_t first_sample, float beta, int32_t* spans_out, float* log_prob_out, float* log_z_out, int32_t* status,
                        void* stream);
/* Parsing under REQUIRED and FORBIDDEN brackets: the best tree, the log-partition and the span posteriors over the binary trees that
 * keep every required span as a constituent and no forbidden one -- the distribution of cliora_span_posteriors conditioned on what
 * the caller knows (annotated phrases, a partial bracketing).  The potentials are unchanged: r[cell, k] = score[cell, k] - max_k
 * score[cell, .], the maximum over every split of the cell, so constrained and unconstrained weights share one scale (DESIGN.md
 * section 19).  A cell [i, j] is ALLOWED iff it crosses no required bracket [s, e] (i < s <= j < e or s < i <= e < j) and equals no
 * forbidden one; in a binary tree "nothing crosses [s, e]" is "[s, e] is a constituent", so the qualifying trees are the trees built
 * from allowed cells.  Per sentence of n words:
 *   best tree  cliora_cky_spans' recurrence with a disallowed cell at -inf: val[leaf] = 1.0f, candidate (val_l + val_r) + (s_k - smax)
 *              in fp32 in that order, first maximum wins; score = val[root] - (float)n, as cliora_kbest_spans reports it.
 *   log_zc     cliora_span_posteriors' inside recurrence in fp64 over the allowed cells; log_z: the unconstrained one, bit for bit
 *              the log_z of cliora_span_posteriors; log_prob = log_zc - log_z, formed in fp64: the log of the joint probability that
 *              every bracket holds (<= 0).
 *   marginals  mu_c[cell] = exp(a_c + b_c - log_zc) by the outside recurrence over the allowed cells: the span posteriors given the
 *              brackets, exactly 0 on a disallowed cell and 1 on a required one.
 *   brackets (B, M, 3) int32 device, M in 0 .. 256 (NULL when M = 0): rows (start, end, kind) of inclusive word positions as in
 *     spans_out; kind 1 = required, kind 0 = forbidden; a row with start = -1 is unused.  A required leaf or root changes nothing.
 *   lengths (B) int32 device, or NULL: every sentence has L words.  Otherwise the sentences share a right-padded chart, with the
 *     rules of cliora_cky_spans_ragged.  With every length equal to L the outputs are bitwise those of the lengths == NULL call.
 *   status: an int32 on the device, zeroed by the call, always required: it counts the sentences with a length outside [1, L] or with
 *     a row that is neither unused nor 0 <= start <= end < n with kind 0 or 1, each once.  Such a sentence is not decoded: every row
 *     -1, feasible 0, log_z 0, score / log_zc / log_prob -inf, marginals 0, and none of its scores is read.
 *   spans_out (B, L-1, 2) (may be NULL when L = 1): the n - 1 spans in cliora_cky_spans' order, the root last, (-1, -1) beyond.
 *     score_out, log_z_out, log_zc_out, log_prob_out (B) fp32; feasible_out (B) int32.  marginals (B, C) fp32 in the cell order of
 *     inside_s, exactly 0 outside a sentence's triangle, or NULL: the outside pass is skipped.
 *   No qualifying tree (crossing required brackets, a span both required and forbidden, a forbidden leaf or root) is no error:
 *     feasible 0, every row -1, score / log_zc / log_prob -inf, log_z the real value, marginals 0, nothing counted.
 * Without a disallowed cell the spans are those of cliora_cky_spans, log_z, log_zc and the marginals those of cliora_span_posteriors,
 * bit for bit, and log_prob is 0.  One workgroup per sentence, fixed-order reductions, no floating-point atomics: two calls give
 * equal bits.  The tables fit the LDS up to L = 128 (143 KiB there): no scratch.  Every plan cliora_cky_spans takes is taken: long
 * plans, padded charts, TreeLSTM plans.  Refused with CLIORA_EINVAL and a message, before any launch: M outside 0 .. 256; a NULL
 * plan, workspace, scalar output, feasible_out or status; NULL spans_out with L > 1; NULL brackets with M > 0; a plan that has not
 * run a forward. */
int cliora_constrained_parse(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const int32_t* brackets, int M,
                             int32_t* spans_out, float* score_out, float* log_z_out, float* log_zc_out, float* log_prob_out,
                             int32_t* feasible_out, float* marginals, int32_t* status, void* stream);
/* The K best trees and SAMPLED trees under required and forbidden brackets: cliora_kbest_spans and cliora_sample_trees over the
 * distribution cliora_constrained_parse conditions -- the trees built from allowed cells, under the unchanged potentials r = s_k -
 * max_k s over every split of the cell, allowed or not.  brackets (B, M, 3), M, lengths and status are
 * cliora_constrained_parse's: status is always required and counts, once each, the sentences with a length outside [1, L] or a bad row;
 * such a sentence is not decoded and none of its scores is read.  A sentence with no qualifying tree is no error and is not counted:
 * feasible_out (B) int32 is 0 for it, as for a rejected one.  Every plan cliora_cky_spans takes is taken: long plans, padded charts,
 * TreeLSTM plans.  One workgroup per sentence, fixed-order reductions, no floating-point atomics: two calls give equal bits.
 *
 * cliora_kbest_spans_constrained: the contract of cliora_kbest_spans -- the candidate (val_left[i] + val_right[j]) + (s_k - smax) in
 *   fp32 in that order, a list the first K candidates by value descending, then split, left rank, right rank ascending -- over the
 *   derivations built from allowed cells.  A cell keeps a count: 1 at an allowed leaf, min(K, sum_k count[left_k] * count[right_k]) at
 *   an allowed cell, 0 at a disallowed one; a split with an empty child offers nothing.
 *   count_out (B): min(K, the number of qualifying trees); scores_out (B, K), spans_out (B, K, L-1, 2): as cliora_kbest_spans writes
 *   them.  No qualifying tree, or a rejected sentence: count 0, scores -inf, every row -1.
 *   With no disallowed cell every output is bitwise cliora_kbest_spans'.  Always, rank 0's spans and score are bitwise the spans_out /
 *   score_out of cliora_constrained_parse.
 *   scratch: device memory of cliora_kbest_constrained_scratch_bytes(plan, K, M) bytes -- 0 when the lists fit the LDS beside the walk
 *   stacks, the count bytes and the mask, else B lists of 8 C K bytes; NULL when that is 0.
 *   Refused with CLIORA_EINVAL and a message, before any launch: K outside 1..16; M outside 0..256; a NULL plan, workspace, scores_out,
 *   count_out, feasible_out or status; NULL spans_out with L > 1; NULL brackets with M > 0; NULL scratch when the query is not 0; a plan
 *   that has not run a forward.
 *
 * cliora_sample_trees_constrained: the draws of cliora_sample_trees -- S, seed, first_sample, beta, ids, the Philox counter (level *
 *   256 + pos, sample_lo, sample_hi, sentence id), the fixed-order scan and split = #{k : c_k <= u c_{N-1}} are its -- over the inside
 *   table of the allowed cells at inverse temperature beta, fp64.  A split with a child that no qualifying tree holds weighs exactly 0;
 *   by the scan it could only be chosen through the clamp, so the clamp goes to the largest k whose children both have a finite inside
 *   value, not to N - 1 (without a disallowed cell that is N - 1).
 *   log_prob_out (B, S) fp32: beta * (sum of r over the chosen splits) - log_zc, summed in fp64: the log-probability of the draw given
 *   the brackets.  log_zc_out, log_z_out (B) fp32: the constrained and the unconstrained log-partition at beta, computed in one level
 *   loop; at beta = 1 bitwise the log_zc_out / log_z_out of cliora_constrained_parse.  spans_out (B, S, L-1, 2): as cliora_sample_trees.
 *   No qualifying tree: every row -1, log_prob and log_zc -inf, log_z the real value.  A rejected sentence: every row -1, log_prob and
 *   log_zc -inf, log_z 0.
 *   With no disallowed cell spans, log_prob and log_z are bitwise cliora_sample_trees' for the same (seed, ids, first_sample, beta).
 *   A draw depends on (seed, sentence id, sample index, cell), the sentence's scores and its brackets alone.  The tables fit the LDS up
 *   to L = 128 and M = 256 (161 504 bytes there): no scratch.
 *   Refused with CLIORA_EINVAL and a message, before any launch: S outside 1 .. 2^20; beta negative or not finite; M outside 0..256; a
 *   NULL plan, workspace, log_prob_out, log_zc_out, log_z_out, feasible_out or status; NULL spans_out with L > 1; NULL brackets with
 *   M > 0; a plan that has not run a forward. */
size_t cliora_kbest_constrained_scratch_bytes(const cliora_plan* plan, int K, int M);
int cliora_kbest_spans_constrained(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const int32_t* brackets, int M, int K,
                                   int32_t* spans_out, float* scores_out, int32_t* count_out, int32_t* feasible_out, void* scratch,
                                   int32_t* status, void* stream);
int cliora_sample_trees_constrained(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const int32_t* ids,
                                    const int32_t* brackets, int M, int S, uint64_t seed, uint64_t first_sample, float beta,
                                    int32_t* spans_out, float* log_prob_out, float* log_zc_out, float* log_z_out, int32_t* feasible_out,
                                    int32_t* status, void* stream);
/* The gradient of cliora_constrained_parse's log_prob with respect to the per-split inside scores: what a loss -log_prob (distant
 * supervision from annotated phrases, the log-likelihood of a gold tree as its n - 2 inner brackets, forbidden-bracket penalties)
 * hands to cliora_chart_backward_split.  With a_x / b_x the inside / outside tables of the constrained (x = c,
 * over the allowed cells) and the unconstrained (x = u) distribution, for split k of a cell with children left_k, right_k:
 *   nu_x[cell, k]    = exp(b_x[cell] + a_x[left_k] + a_x[right_k] + r[cell, k] - log_z_x), 0 where the cell or a child is disallowed
 *   d_split[cell, k] = w[b] * ((nu_c - nu_u)[cell, k] - [k == k*] * sum_k (nu_c - nu_u)[cell, .])
 * k* is the first maximum of the cell's scores (the rule of cliora_cky_spans): it carries the derivative of the row maximum in r, so
 * every row sums to zero.  Tables and sums in fp64, fixed order; d_split in fp32.
 *   d_split: cliora_plan_split_score_count floats in the layout of the inside split-score rows: row B * lvl_base[level] + (b * (L -
 *     level) + pos) * level + k.  EVERY element is written (no memset is needed); cells beyond a sentence's triangle get zeros.
 *   weights (B) fp32 device, or NULL = 1: in a backward, the cotangent of log_prob.
 *   brackets, M, lengths, status: as cliora_constrained_parse takes them.  With every length equal to L the outputs are bitwise those
 *     of the lengths == NULL call.
 *   log_prob_out (B) fp32: bitwise the log_prob of cliora_constrained_parse on the same chart; feasible_out (B) int32.
 *   A sentence with no qualifying tree (feasible 0, log_prob -inf), with a bad length or a bad row (feasible 0, log_prob -inf, one
 *     count in *status) gets a zero gradient, and its weight is not read.  Without a disallowed cell the gradient is exactly 0 and
 *     log_prob is 0.
 * One workgroup per sentence, a wavefront per cell, each element written by one lane, no floating-point atomics: two calls give equal
 * bits.  The four tables fit the LDS (71 KiB at L 64 and M 256): no scratch.  Refused with CLIORA_EINVAL and a message, before any
 * launch: a long plan (L > 64: the backward stops at 64 words, so nothing could take the gradient); M outside 0 .. 256; a NULL plan,
 * workspace, d_split, log_prob_out, feasible_out or status; NULL brackets with M > 0; a plan that has not run a forward. */
size_t cliora_plan_split_score_count(const cliora_plan* plan);   /* floats in the inside split-score rows of a batch: B * sum_level level * (L - level) */
int cliora_bracket_grad(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const int32_t* brackets, int M,
                        const float* weights, float* d_split, float* log_prob_out, int32_t* feasible_out, int32_t* status,
                        void* stream);
/* Expectations under the same distribution over binary trees, with their gradient: per sentence
 *   risk    = E_T[sum of cost[cell] over the cells of T, leaves and root included] = sum over the triangle of mu[cell] * cost[cell]
 *   entropy = -sum_T p(T) log p(T) = log_z - E_T[sum of r over T's edges]
 *   d_split = d (w_cost[b] * risk + w_entropy[b] * entropy) / d s over the per-split inside scores.
 * With v[cell, k] = w_cost * cost[cell] - w_entropy * r[cell, k], V(T) its sum over the tree's edges plus w_cost * cost over its leaves:
 *   d_split[cell, k] = G_r[cell, k] - [k == k*] * sum_k G_r[cell, .],   G_r[e] = nu[e] * (E[V | e in T] - E[V])
 * nu the edge marginal and k* the first maximum of the cell's scores, as cliora_bracket_grad has them: every row sums to zero.  The
 * conditional means come from an inside and an outside mean table beside the two log-space tables (an expectation-semiring pass),
 * all in fp64, sums in a fixed order; the outputs are fp32.
 *   cost (B, C) fp32 device in the cell order of inside_s / the marginals of cliora_span_posteriors, or NULL = 0; costs of cells
 *     beyond a sentence's triangle are never read.  w_cost (B) fp32 device or NULL = 1; w_entropy (B) fp32 device or NULL = 0: in a
 *     backward, the cotangents of risk and entropy.
 *   d_split: cliora_plan_split_score_count floats in the layout cliora_bracket_grad writes.  EVERY element is written (no memset is
 *     needed); cells beyond a sentence's triangle get zeros.
 *   risk_out, entropy_out, log_z_out (B) fp32; none depends on the weights.  One word: risk = cost[leaf], entropy = 0.  Two words:
 *     risk is the sum of the three costs, entropy = 0 and the gradient is exactly 0.
 *   lengths (B) int32 device or NULL; status: an int32 on the device, zeroed by the call, always required: it counts the lengths
 *     outside [1, L].  Such a sentence gets a zero gradient and risk = entropy = log_z = 0; its weights, costs and scores are not
 *     read.  With every length equal to L the outputs are bitwise those of the lengths == NULL call.
 * One workgroup per sentence, a wavefront per cell, each element written by one lane, no floating-point atomics: two calls give equal
 * bits, and a sentence of a padded chart gets the bits it gets alone.  The tables fit the LDS (36 C + 4 L + 128 bytes: 73.5 KiB at
 * L 64): no scratch.  Refused with CLIORA_EINVAL and a message, before any launch: a long plan (L > 64: the backward stops at 64
 * words, so nothing could take the gradient); a NULL plan, workspace, d_split, scalar output or status; a plan that has not run a
 * forward. */
int cliora_tree_expectation(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const float* cost, const float* w_cost,
                            const float* w_entropy, float* d_split, float* risk_out, float* entropy_out, float* log_z_out,
                            int32_t* status, void* stream);
/* Max-margin bracket losses over the same potentials: structured hinge, perceptron and ramp.  With dis[cell] = 1
 * on a cell of levels 1 .. n - 2 that the brackets disallow (it crosses a required bracket or equals a forbidden one; leaves and the
 * root are in every tree and carry no cost), F(t) the sum of r over the n - 1 internal cells of a tree t and D(t) the sum of dis:
 *   A    = max_t F(t) + margin * D(t)       its argmax: the cost-augmented tree
 *   Bv   = max_t F(t) - penalty * D(t)      its argmax: the reference tree
 *   loss = A - Bv >= 0
 *   d_split[cell, k] = w[b] * (c[cell, k] - [k == k*] * sum_k c[cell, .]),  c = [(cell, k) in the augmented tree] - [.. in the reference tree]
 * k* is the first maximum of the cell's scores, as cliora_bracket_grad has it: every row sums to zero.  margin >= 0 (finite); penalty in
 * [0, +inf].  penalty = +inf: the second maximum runs over the qualifying trees of cliora_constrained_parse -- a disallowed cell holds
 * -inf, a forbidden leaf or root makes the sentence infeasible -- and the reference tree and feasible are that entry's, bit for bit.
 * margin > 0, penalty = +inf: structured hinge with margin rescaling; margin = 0, penalty = +inf: perceptron; a finite penalty: ramp,
 * defined for a bracket set that no tree satisfies too.
 * Both maxima are cliora_cky_spans' recurrence in fp32 (val[leaf] = 1, candidate (val_l + val_r) + (s_k - smax), first maximum wins)
 * in one level loop, with val[cell] = best + bonus[cell] after the cell's own argmax: + margin * dis in the first pass, - penalty * dis
 * (or -inf on a disallowed cell) in the second.  With margin = 0 the augmented tree is cliora_cky_spans' (cliora_cky_spans_ragged's).
 *   d_split: cliora_plan_split_score_count floats in the layout cliora_bracket_grad writes.  EVERY element is written, once (no memset
 *     is needed); cells beyond a sentence's triangle get zeros.  The integer in the bracket lies in -2 .. 2 and meets w[b] once:
 *     d_split is exact in fp32 given the two trees; a zero is +0 whatever the weight.
 *   weights (B) fp32 device, or NULL = 1: in a backward, the cotangent of the loss.
 *   loss_out, aug_score_out, ref_score_out (B) fp32: A - Bv, A and Bv formed in fp64 from the terms of the two emitted trees (r in fp64
 *     from the fp32 scores, plus the bonuses), rounded once.  A difference below 0 -- the two fp32 maxima within rounding of each
 *     other -- is stored as +0 with a zero gradient.  Equal trees give a loss of exactly +0 under an infinite penalty.
 *   violations_out (B) int32: D of the augmented tree; with margin = 0, the bracket violations of the best tree.  feasible_out (B) int32.
 *   spans_aug, spans_ref (B, L-1, 2) int32, either NULL: the two trees in cliora_cky_spans' layout, (-1, -1) beyond.
 *   brackets, M, lengths, status: as cliora_bracket_grad takes them.  With every length equal to L the outputs are bitwise those of the
 *     lengths == NULL call.
 *   A bad length or a bad row: zero gradient, loss 0, both scores 0, violations 0, feasible 0, rows -1, one count in *status; the weight
 *     is not read.  penalty = +inf and no qualifying tree: zero gradient, loss 0, ref_score -inf, feasible 0, spans_ref rows -1 (the
 *     augmented tree, its score and its violations are still given; nothing is counted); the weight is not read.  No disallowed cell:
 *     both trees are cliora_cky_spans', loss +0, zero gradient, one pass.
 * One workgroup per sentence, a wavefront per cell, each element written by one lane, no floating-point atomics: two calls give equal
 * bits.  The tables fit the LDS (17 C + 52 L + 12 M + 248 bytes: 41 KiB at L 64 and M 256): no scratch.  TreeLSTM plans are taken (the
 * entry only reads the split scores).  Refused with CLIORA_EINVAL and a message that starts with the entry's name, before any launch: a
 * long plan (L > 64: the backward stops at 64 words); M outside 0 .. 256; margin negative, NaN or infinite; penalty negative or NaN; a
 * NULL plan, workspace, d_split, scalar output, feasible_out or status; NULL brackets with M > 0; a plan that has not run a forward. */
int cliora_bracket_margin(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const int32_t* brackets, int M, float margin,
                          float penalty, const float* weights, float* d_split, float* loss_out, float* aug_score_out,
                          float* ref_score_out, int32_t* violations_out, int32_t* feasible_out, int32_t* spans_aug, int32_t* spans_ref,
                          int32_t* status, void* stream);
/* The divergence between TWO charts' distributions over binary trees, with both gradients.  Teacher P =
 * (plan_p, fwd_workspace_p) with split scores s^p, student Q = (plan_q, fwd_workspace_q) with s^q: two plans of the same B and L whose
 * forward has run; D, R, weight sharing, soft or hard, MLP or TreeLSTM may differ -- only the split scores are read.  With
 * r^x[cell, k] = s^x[cell, k] - max_k s^x[cell, .], a tree weighing exp(sum of r^x over its internal cells) under chart x, R^x(T) that sum:
 *   entropy_p     = -sum_T p(T) log p(T) = log_z_p - E_p[R^p]
 *   cross_entropy = -sum_T p(T) log q(T) = log_z_q - E_p[R^q]
 *   kl            = cross_entropy - entropy_p = KL(p || q) >= 0 (to rounding)
 *   J             = w_kl[b] * kl + w_ce[b] * cross_entropy
 *   d_split_q = dJ / d s^q:  G_q[e] = (w_kl + w_ce) * (nu^q[e] - nu^p[e])
 *   d_split_p = dJ / d s^p:  G_p[e] = nu^p[e] * (E_p[V | e in T] - E_p[V]),  v[e] = w_kl * r^p[e] - (w_kl + w_ce) * r^q[e], V(T) its sum
 *   d_split_x[cell, k] = G_x[cell, k] - [k == k*_x] * sum_k G_x[cell, .],  k*_x the first maximum of chart x's OWN row
 * nu^x the edge marginal of chart x, as cliora_bracket_grad has it: every row of both gradients sums to zero.  Log-space inside and
 * outside tables of both charts and, for d_split_p, cliora_tree_expectation's pair of mean tables under p, all in fp64, sums in a fixed
 * order; the outputs are fp32.  nu^p and nu^q are formed by one expression: the same workspace as both charts gives d_split_q == 0
 * exactly, kl == 0 exactly and d_split_p at rounding level.
 *   w_kl (B) fp32 device or NULL = 1; w_ce (B) fp32 device or NULL = 0: in a backward, the cotangents of kl and cross_entropy.
 *   d_split_p, d_split_q: each NULL or cliora_plan_split_score_count floats in the layout cliora_bracket_grad writes, in which EVERY
 *     element is written (no memset is needed); cells beyond a sentence's triangle get zeros.  d_split_p NULL (a detached teacher, the
 *     common case): the two mean tables are neither formed nor carved, and d_split_q has the bits of the call with d_split_p.  Both
 *     NULL: evaluation only.
 *   kl_out, cross_entropy_out, entropy_p_out, log_z_p_out, log_z_q_out (B) fp32, all required; none depends on the weights.  log_z_p and
 *     log_z_q have cliora_span_posteriors' bits, entropy_p has cliora_tree_expectation's.  One word: all zeros.  Two words: kl =
 *     cross_entropy = entropy_p = 0 and both gradients are exactly 0.
 *   lengths (B) int32 device or NULL, one array for both charts; status: an int32 on the device, zeroed by the call, always required: it
 *     counts the lengths outside [1, L].  Such a sentence gets zero gradients and zero scalars; its weights and scores are not read.
 *     With every length equal to L the outputs are bitwise those of the lengths == NULL call.
 * One workgroup per sentence, a wavefront per cell, each element written by one lane, no floating-point atomics: two calls give equal
 * bits, and a sentence of a padded chart gets the bits it gets alone.  The tables fit the LDS (56 C + 4 L + 128 bytes with d_split_p,
 * 40 C + 4 L + 128 without: 114.1 / 81.6 KiB at L 64): no scratch.  TreeLSTM plans are taken.  Refused with CLIORA_EINVAL and a message
 * that starts with the entry's name, before any launch: either plan long (L > 64); plans whose B or L differ; a NULL plan, workspace,
 * scalar output or status; a plan that has not run a forward. */
int cliora_tree_kl(cliora_plan* plan_p, void* fwd_workspace_p, cliora_plan* plan_q, void* fwd_workspace_q, const int32_t* lengths,
                   const float* w_kl, const float* w_ce, float* d_split_p, float* d_split_q, float* kl_out, float* cross_entropy_out,
                   float* entropy_p_out, float* log_z_p_out, float* log_z_q_out, int32_t* status, void* stream);
/* Both passes for sentences of DIFFERENT lengths run as one batch, each padded on the right to the plan's L (inference only).  The
 * arguments of cliora_chart_forward, plus
 *   lengths (B) int32 device; root_levels: bit t set iff some sentence has lengths[b] - 1 == t (the caller holds the lengths on the
 *   host, so the call makes no device-to-host copy; a sentence whose bit is missing gets an unspecified outside chart);
 *   status: an int32 on the device the call zeroes first, then counts the lengths outside [1, L] in -- the caller must check it; the
 *   cells of such a sentence are unspecified (nothing is read or written out of bounds).
 * For every cell of sentence b's own triangle (pos + level < lengths[b]) the four charts hold what cliora_chart_forward computes for
 * that sentence alone at its exact length, to rounding (the level kernels tile a level by its row count).  Cells OUTSIDE a
 * sentence's triangle are unspecified in all four charts -- inside_s holds -1e30 there, written whether or not bit 0 of run_outside
 * asks for the outside pass.  normalize = none: nothing bounds the vectors of the padded cells, so padded input whose unnormalised
 * charts leave fp32's range (as they do at any length beyond a few words with N(0, 1) weights) can bring a non-finite value into a
 * sentence's own cells through a 0-weight pair; the same holds for the padded inside pass.  With normalize = unit every value is
 * finite.  How: the inside pass is prefix-closed; an
 * outside pair (parent, sibling) of a cell of the triangle leaves the triangle iff its sibling does, and its score adds
 * inside_s[sibling], so the -1e30 written after the inside pass gives those pairs a softmax weight of exactly 0 in the unchanged
 * level kernels; the sentence's root cell (lengths[b] - 1, 0) then receives the rows of the padded chart's root cell after its level
 * has run, and the level below is scored again.  Schedule: inside levels, mask, root, outside levels one
 * after the other on the caller's stream -- no wavefront, no side stream, no resident kernels.  The per-split scores in the
 * workspace are untouched by the outside pass: cliora_cky_spans_ragged after this call decodes what it decodes after the
 * inside-only forward.  With every length equal to L the charts are bitwise those of cliora_chart_forward on the sequential
 * schedule (cliora_set_wavefront(0), launch path).
 * Refused with CLIORA_EINVAL and a message: run_outside without CLIORA_FWD_NO_BACKWARD (a padded chart has no backward), with
 * CLIORA_FWD_PAIR_STATES, a drop_mask, params->root_mat (compress), TreeLSTM plans.  Text-only and CLIORA plans, share 0 / 1,
 * normalize unit / none. */
int cliora_chart_forward_ragged(cliora_plan* plan, const cliora_params* params, const float* x_span, const float* obj_span,
                                const float* drop_mask, float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                                float* inside_c, void* fwd_workspace, size_t fwd_workspace_bytes, int run_outside,
                                const int32_t* lengths, uint64_t root_levels, int32_t* status, void* stream);
/* The call above for every DioraMLP / CLIORA plan of L <= 128, LONG plans (64 < L <= 128) included: the same
 * arguments, the same schedule and the same contract, except that root_levels points at TWO words in host memory (read during the
 * call): bit t & 63 of word t >> 6 is set iff some sentence has lengths[b] - 1 == t.  On a long plan the level launches are the long
 * plan's (two splits per lane in the score + softmax kernels); the mask and seed kernels are the same.  On a plan of L <= 64 the
 * launches, and so the bits of every output, are those of cliora_chart_forward_ragged given word 0.  With every length equal to L the
 * charts are bitwise those of cliora_chart_forward on the sequential schedule at any L.
 * Refused with CLIORA_EINVAL and a message that starts with the entry's name, each before any HIP call: a NULL plan, params, lengths,
 * root_levels or status; a TreeLSTM plan; run_outside without CLIORA_FWD_NO_BACKWARD or with CLIORA_FWD_PAIR_STATES; params->root_mat
 * (compress); a drop_mask; a bit of root_levels set at or above L (bit L - 1, the chart's own root, is legal and ignored); on a long
 * plan, cliora_set_resident(1) / CLIORA_RESIDENT=1 forcing the sentence-resident kernels on a plan they would otherwise take. */
int cliora_chart_forward_ragged_wide(cliora_plan* plan, const cliora_params* params, const float* x_span, const float* obj_span,
                                     const float* drop_mask, float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                                     float* inside_c, void* fwd_workspace, size_t fwd_workspace_bytes, int run_outside,
                                     const int32_t* lengths, const uint64_t* root_levels, int32_t* status, void* stream);

/* TRAINING through such a padded chart, text-only DIORA.  cliora_chart_forward_ragged_train: the call above,
 * same schedule, same status word, same charts, with the state the backward needs written -- run_outside WITHOUT
 * CLIORA_FWD_NO_BACKWARD.  cliora_chart_backward_ragged: the arguments of cliora_chart_backward_split (d_split_s may be NULL), plus
 * lengths and root_levels as the forward got them and four caller-allocated buffers m_* of the shapes of the four cotangents
 * ((B,C,D), (B,C), (B,C,D), (B,C); one may be NULL where its cotangent is).  The cotangents of cells beyond a sentence's triangle are
 * ignored, whatever they hold: the call first writes their masked copies into m_* and the chains read those.  Every invalid pair
 * carries a softmax weight of exactly 0 from the forward, and each sentence's root cell (lengths[b] - 1, 0) is cut out of the outside
 * backward of its level -- what accumulates in its vH goes to d root_h through the unit-norm backward -- so the unchanged chains of
 * cliora_chart_backward compute, for every parameter and for d_x_span[b, :lengths[b]], the sum over the sentences of the gradients
 * cliora_chart_backward computes for each alone at its exact length, to rounding; d_x_span[b, lengths[b]:] is exactly 0; d_split_s
 * must be zero beyond each triangle (cliora_bracket_grad and cliora_tree_expectation with `lengths` write it so).  The backward never
 * runs on the sentence-resident kernels; with every length equal to L its results are bitwise those of cliora_chart_backward_split on
 * the launch path.  Both are refused with CLIORA_EINVAL and a message of their own, before any launch, for: TreeLSTM plans, CLIORA
 * plans (R > 0), L > 64, CLIORA_FWD_PAIR_STATES, params->root_mat (compress), a drop_mask; the forward also for
 * CLIORA_FWD_NO_BACKWARD (that is cliora_chart_forward_ragged). */
int cliora_chart_forward_ragged_train(cliora_plan* plan, const cliora_params* params, const float* x_span, const float* obj_span,
                                      const float* drop_mask, float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                                      float* inside_c, void* fwd_workspace, size_t fwd_workspace_bytes, int run_outside,
                                      const int32_t* lengths, uint64_t root_levels, int32_t* status, void* stream);
int cliora_chart_backward_ragged(cliora_plan* plan, const cliora_params* params, const float* x_span, const float* obj_span,
                                 const float* drop_mask, const float* inside_h, const float* inside_s, const float* outside_h,
                                 const float* outside_s, const float* d_inside_h, const float* d_inside_s, const float* d_outside_h,
                                 const float* d_outside_s, const float* d_split_s, void* fwd_workspace, size_t fwd_workspace_bytes,
                                 void* bwd_workspace, size_t bwd_workspace_bytes, float* d_x_span, float* d_obj_span,
                                 const cliora_params* grads, int ran_outside, const int32_t* lengths, uint64_t root_levels,
                                 float* m_inside_h, float* m_inside_s, float* m_outside_h, float* m_outside_s, void* stream);

/* The same pair for CLIORA plans (R > 0): same arguments, with obj_span (B, R, D) REQUIRED, the (B, C, R)
 * drop_mask of cliora_chart_forward taken (NULL: no dropout) and d_obj_span (B, R, D) written (NULL: skipped).  The attention over
 * a sentence's own regions touches the inside cells only and has no term across cells, so nothing is added to the schedule: the
 * attention backward runs over every cell of a level, and a cell beyond a triangle carries vH = 0 and finite attention state (an
 * all-masked cell has uniform weights), so its contribution to d_obj_span and to the chains is an exact zero.  The backward never
 * runs on the sentence-resident kernels; with every length equal to L the results are bitwise those of cliora_chart_backward_split.
 * Refused with CLIORA_EINVAL and a message of their own, before any launch: TreeLSTM plans, text-only plans (R = 0), a NULL obj_span,
 * L > 64, CLIORA_FWD_PAIR_STATES, params->root_mat (compress); the forward also CLIORA_FWD_NO_BACKWARD. */
int cliora_chart_forward_ragged_train_vl(cliora_plan* plan, const cliora_params* params, const float* x_span, const float* obj_span,
                                         const float* drop_mask, float* inside_h, float* inside_s, float* outside_h, float* outside_s,
                                         float* inside_c, void* fwd_workspace, size_t fwd_workspace_bytes, int run_outside,
                                         const int32_t* lengths, uint64_t root_levels, int32_t* status, void* stream);
int cliora_chart_backward_ragged_vl(cliora_plan* plan, const cliora_params* params, const float* x_span, const float* obj_span,
                                    const float* drop_mask, const float* inside_h, const float* inside_s, const float* outside_h,
                                    const float* outside_s, const float* d_inside_h, const float* d_inside_s, const float* d_outside_h,
                                    const float* d_outside_s, const float* d_split_s, void* fwd_workspace, size_t fwd_workspace_bytes,
                                    void* bwd_workspace, size_t bwd_workspace_bytes, float* d_x_span, float* d_obj_span,
                                    const cliora_params* grads, int ran_outside, const int32_t* lengths, uint64_t root_levels,
                                    float* m_inside_h, float* m_inside_s, float* m_outside_h, float* m_outside_s, void* stream);

/* Grounding evaluation (cliora/scripts/parse.py:176-264, the host loop over every phrase and predicted span): ONE launch for a batch,
 * one workgroup per sentence.  All pointers are device memory.
 *   atten (B, L, R) fp32 at element strides (sb, sl, sr) -- DioraMLP.atten_score, a permuted diagonal of vg_atten_score, read in
 *     place; boxes (B, R, 4) fp32 xyxy, contiguous.  atten == NULL (text-only DIORA): counts only, P must be 0.
 *   gold phrases, CSR: phr_off (B+1), phr_span (P, 2) = (start, end) with `end` exclusive as VG_GT stores it, phr_box (P, 4) gold box.
 *   spans (B, L-1, 2): cliora_cky_spans' output, the root last.  gold constituents, CSR: gold_off (B+1), gold_span (G, 2)
 *     (batch_map['GT'][b][:-1]; duplicates allowed).
 * Box of a word range [s, e): the first word whose maximum over the regions is the largest, then the first region of that word's row
 * attaining it (torch's CPU max(dim); a NaN is larger than every number).  IoU: torchvision's box_iou in fp32 and in its operation
 * order; hit = IoU > 0.5 (a 0/0 is NaN: no hit).  CCRA flag = hit and (end - 1 == start, or (start, end - 1) is a predicted span other
 * than the root).
 *   phr_out (P, 4) int32: selected word, selected box, hit, ccr.  A phrase outside 0 <= start < end <= L is not read (the reference
 *     raises on its empty slice): it gets (-1, -1, 0, 0) and is counted in *status, which the caller must check (an int32 the call
 *     zeroes first; predicted spans outside the sentence count there too).
 *   span_box (B, L-1) int32 / span_xyxy (B, L-1, 4) fp32, either NULL: the box id / coordinates chosen for each predicted span
 *     over its words (the root's too; the reference writes boxes for the non-root spans only).
 *   sent_out (B, 3) int32: |pred & gold|, |pred|, |gold| over span SETS, pred without the root -- the integers of the span F1; its
 *     float formulas stay with the caller (SpanF1 semantics, parse.py:215-234). */
int cliora_ground_eval(int B, int L, int R, const float* atten, int64_t atten_sb, int64_t atten_sl, int64_t atten_sr,
                       const float* boxes, int P, const int32_t* phr_off, const int32_t* phr_span, const float* phr_box,
                       const int32_t* spans, int G, const int32_t* gold_off, const int32_t* gold_span, int32_t* phr_out,
                       int32_t* span_box, float* span_xyxy, int32_t* sent_out, int32_t* status, void* stream);
/* The same for a batch of sentences of different lengths padded to L: lengths (B) int32 device.  Sentence b is its first
 * n = lengths[b] words: rows 0 .. n-2 of `spans` are read (cliora_cky_spans_ragged's layout, the root = row n-2), phrases must satisfy
 * 0 <= start < end <= n, rows of atten beyond word n-1 are not read, and rows n-1 .. L-2 of span_box / span_xyxy are written as -1 / 0.
 * A length outside [1, L] is counted in *status and the sentence is not read (its phrases get (-1, -1, 0, 0) and count too).  The same
 * kernel with the same rules; with every length equal to L the outputs are bitwise those of cliora_ground_eval. */
int cliora_ground_eval_ragged(int B, int L, int R, const int32_t* lengths, const float* atten, int64_t atten_sb, int64_t atten_sl,
                              int64_t atten_sr, const float* boxes, int P, const int32_t* phr_off, const int32_t* phr_span,
                              const float* phr_box, const int32_t* spans, int G, const int32_t* gold_off, const int32_t* gold_span,
                              int32_t* phr_out, int32_t* span_box, float* span_xyxy, int32_t* sent_out, int32_t* status, void* stream);

/* Phrase vectors (cliora/scripts/phrase_embed.py:79-92, 223-224; phrase_embed_simple.py:262-287): ONE launch for a batch's
 * phrases, one wavefront per phrase.  All pointers are device memory.
 *   inside_h / outside_h (B, C, D) fp32, C = L(L+1)/2, at element strides (sb, sc) for the sentence and the cell (unit stride along D).
 *   table (N, 3) int32: (sentence, pos, size); the cell is C - (L-size+1)(L-size+2)/2 + pos (offset(L)[size-1] + pos).
 *   out: row row_offset + r (leading dimension ldo >= 2D) = [inside_h[b, cell] | outside_h[b, cell]]; a caller-owned buffer, so a
 *     whole corpus is appended on the device batch by batch.  normalize != 0: the row scaled to unit L2 norm as faiss.normalize_L2
 *     does (a zero row stays zero); the norm is summed in fp64, so a row is within an ulp of an fp64 normalisation.
 *   A row with size < 1, pos < 0, pos + size > L, or a sentence outside [0, B) is not read: it is written as zeros and counted in
 *   *status (an int32 the call zeroes first), which the caller must check. */
int cliora_phrase_gather(int B, int L, int D, const float* inside_h, int64_t in_sb, int64_t in_sc, const float* outside_h,
                         int64_t out_sb, int64_t out_sc, int N, const int32_t* table, int normalize, float* out, int64_t ldo,
                         int64_t row_offset, int32_t* status, void* stream);

/* Exact inner-product top-k, the semantics of faiss.IndexFlatIP(D).add(keys); .search(q, k) (phrase_embed.py:136-146).
 *   q (nq, D) and keys (nk, D) fp32 at leading dimensions ldq, ldk >= D, any D >= 1 (padded to 32 internally); 1 <= k <= 128
 *   (anything else: CLIORA_EINVAL with a message).  D_out (nq, k) fp32 at ldd, I_out (nq, k) int64 at ldi: the k best keys per
 *   query by descending score; slots past nk hold I = -1 and D = -inf.
 *   Scores on the MFMA of cliora_set_mfma_mode: split-bf16 (three v_mfma_f32_16x16x32_bf16 per product) or fp32-input
 *   (v_mfma_f32_16x16x4f32); fp32 accumulation.  The N x N score matrix is never written: each workgroup scores a 64-query tile
 *   against a range of keys 256 at a time, the scores pass through LDS into a running top-k per query, the per-range lists go to the
 *   workspace and a merge kernel reduces them.  The number of ranges grows as nq shrinks, so a few queries still fill the device.
 *   Determinism: a score is a fixed-order sum over the columns that does not depend on where its rows sit in a tile; equal scores
 *   are ordered by ascending key index; a NaN score ranks below every number.  So a query's result is bitwise the same whatever
 *   other queries share the launch and however the keys were split, and two runs are bitwise equal.
 *   ws: device workspace of cliora_knn_ip_workspace_bytes(nq, nk, D, k) bytes (0 for invalid arguments). */
size_t cliora_knn_ip_workspace_bytes(int nq, int nk, int D, int k);
int cliora_knn_ip(int nq, int nk, int D, int k, const float* q, int64_t ldq, const float* keys, int64_t ldk, float* D_out, int64_t ldd,
                  int64_t* I_out, int64_t ldi, void* ws, size_t ws_bytes, void* stream);

/* The post-search filter of phrase_embed.py:250-263 for a self-search (query i is phrase i): per query walk its k_candidates
 * (I, D at leading dimensions ldi, ldd), skip I == -1 (past the keys: the reference would index example_ids[-1] there, the last
 * phrase), skip a candidate with the query's example id, skip one with the query's phrase id (an integer per distinct token tuple),
 * keep the first k_top.  I_out (nq, k_top) int64 / D_out (nq, k_top) fp32, -1 / -inf past what was found; count (nq) int32 the
 * number found, which the caller compares with k_top.  example_ids / phrase_ids: n_ids >= nq int32 each. */
int cliora_knn_filter(int nq, int k_candidates, const int64_t* I, int64_t ldi, const float* D, int64_t ldd, const int32_t* example_ids,
                      const int32_t* phrase_ids, int n_ids, int k_top, int64_t* I_out, float* D_out, int32_t* count, void* stream);

/* Caption-image retrieval scores: the weighted late-interaction ("MaxSim") product of grouped rows,
 *   S[n][m] = sum over the tokens t of caption n of  w[t] * max over the regions r of image m of <Q[t], O[r]>,
 * the logit of the reference's VGLoss (cliora.py:460, 463-464; trainer.py:145-152) for any set of captions against any set of images.
 *   Q (NT, D) / O (MR, D) fp32 on the device at leading dimensions ldq, ldo >= D, any D >= 1 (padded to 32 internally); caption n
 *   owns rows q_off[n] .. q_off[n+1] of Q (q_off: N + 1 int32 on the device), image m rows o_off[m] .. o_off[m+1] of O; w (NT) fp32.
 *   S (N, M) fp32 at leading dimension lds >= M.  No host synchronisation; everything is enqueued on `stream`.
 *   Arithmetic: the mode of cliora_set_mfma_mode, as cliora_knn_ip; fp32 accumulation.  No buffer of NT x MR or NT x M elements is
 *   written: a scan kernel lays the groups out in 16-row MFMA tiles (a caption tile belongs to one caption, an image's tiles never
 *   straddle a 256-row key step), the operands are packed into fragment blocks, each workgroup scores 64 packed query rows against
 *   a range of key steps, reduces every accumulator tile to its per-row maximum over the VALID key rows (padding is masked, never
 *   scored), combines an image's tiles, multiplies by w and sums the 16 rows of a query tile in a fixed butterfly order; one fp32
 *   partial per (query tile, image) goes to the workspace and a second kernel adds a caption's tiles in ascending order.
 *   Determinism: S[n][m] is a function of caption n's rows and weights and image m's rows alone -- bitwise the same whatever else
 *   is in the call, in whatever order, however the key steps were split over workgroups; two runs are bitwise equal.
 *   An empty caption gives a row of 0.0; an empty image a column of -inf (0.0 against an empty caption).  A NaN in a token makes
 *   that caption's row NaN, a NaN in a region that image's column; nothing else.
 *   status (2 int32 on the device, zeroed by the call): [0] the number of images with more than 256 regions (their columns are
 *   NaN); [1] the number of groups with a decreasing offset or an offset outside [0, NT] / [0, MR], or that no longer fit the
 *   layout bound because earlier groups overlap (such a group reads nothing; its row / column is NaN).  The caller must check it.
 *   Refused before any launch with CLIORA_EINVAL: D < 1, negative counts, ldq / ldo < D, lds < M, a NULL argument; CLIORA_ENOMEM:
 *   ws_bytes below cliora_maxsim_workspace_bytes(N, NT, M, MR, D) (0 for invalid arguments). */
size_t cliora_maxsim_workspace_bytes(int N, int NT, int M, int MR, int D);
int cliora_maxsim_scores(int N, int NT, int M, int MR, int D, const float* Q, int64_t ldq, const int32_t* q_off, const float* w,
                         const float* O, int64_t ldo, const int32_t* o_off, float* S, int64_t lds, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream);

/* Ranks of the paired items in a score matrix S (N captions x M images, leading dimension lds >= M), ordered as cliora_knn_ip
 * orders candidates: descending score, ascending index on ties, NaN below every number.  image_of (N) int32: the image of caption n.
 *   rank_t2i[n]: the number of images m != image_of[n] that order before it in row n (0 = retrieved first).
 *   rank_i2t[m]: over the captions n of image m, the smallest number of captions of OTHER images that order before n in column m;
 *   -1 for an image without captions.
 *   image_of[n] outside [0, M): rank_t2i[n] = -1, the caption belongs to no image, and *status (one int32, zeroed by the call) counts it. */
int cliora_retrieval_ranks(int N, int M, const float* S, int64_t lds, const int32_t* image_of, int32_t* rank_t2i, int32_t* rank_i2t,
                           int32_t* status, void* stream);

/* The k best entries (1 <= k <= 128) of every row of a strided matrix, S[r * row_stride + c * col_stride], under the same order:
 * D_out (rows, k) fp32 and I_out (rows, k) int64, contiguous; slots past `cols` hold -inf / -1.  One wavefront per row.  Swapping
 * the strides (and rows / cols) ranks the columns: the captions per image. */
int cliora_score_topk(int rows, int cols, int k, const float* S, int64_t row_stride, int64_t col_stride, float* D_out, int64_t* I_out,
                      void* stream);

/* The exact word-prediction loss over the whole vocabulary: for token t with projected outside row Q[t] = o_t . mat and word tok[t],
 *   s[t][v] = <Q[t], K[v]>   (the reference's score, trainer.py:58-66, for every word v of the table K),
 *   nll[t] = logsumexp_v s[t][v] - s[t][tok[t]],   loss = sum_t w[t] nll[t].
 *   Q (T, E) / K (V, E) fp32 on the device at leading dimensions ldq, ldk >= E, any E >= 1 (padded to 32 internally); tok (T) int64;
 *   w (T) fp32: 1 / T for the mean, 1 / n_valid on the real words of a padded chart and 0 on its padding.
 *   Outputs (T each, on the device): lse, tgt (the target's logit), nll fp32; lse_lo fp32 or NULL: what fp32 drops of lse (lse is
 *   combined in fp64; lse + lse_lo carries it to 2^-48, and the backward's p = exp((s - lse) - lse_lo) then does not inherit the half
 *   ulp of an lse of magnitude 100, 4e-6 relative on every p of the token); rank int32 or NULL: the number of words that order
 *   before tok[t] as cliora_knn_ip orders candidates (descending score, ascending index on ties, NaN below every number);
 *   loss: one fp32.  No host synchronisation; everything is enqueued on `stream`.
 *   Arithmetic: the mode of cliora_set_mfma_mode, as cliora_knn_ip, and its score chain instruction for instruction; fp32
 *   accumulation.  No buffer of T x V elements is written: each workgroup scores 64 tokens against a range of 8 x 256 words, keeps a
 *   running (max, sum exp(. - max)) per token over the VALID words of a step (words at or past V are masked, never scored; the
 *   maximum is subtracted before every exp), one (max, sum) pair and one count per (token, range) go to the workspace by plain
 *   stores, and a second kernel combines a token's ranges in ascending order.  The ranges are a function of V alone.  tgt comes
 *   from the same chain on the rows K[tok[t]] packed in token order, so it is bit for bit the main pass's score of (t, tok[t]):
 *   rank[t] == 0 exactly when cliora_knn_ip(k = 1) returns tok[t].  loss is one fp64 chain in ascending token order, rounded once.
 *   Determinism: no float atomics; a token's lse / tgt / nll / rank are a function of its row, its word and K alone -- bitwise the
 *   same whatever else is in the call and in whatever order; two runs are bitwise equal.
 *   Edge cases: a tok[t] outside [0, V) is counted in *status (one int32, zeroed by the call; the caller must check it), gets
 *   nll = tgt = NaN and rank = -1, and adds nothing to loss or to the gradients.  A token with w[t] == 0 adds nothing BY SELECTION
 *   (a NaN in a padded row does not leak).  A NaN in Q[t] makes token t's outputs, and loss if w[t] != 0, NaN; no other token's.
 *   V = 1: nll = 0, rank = 0.  T = 0: loss = 0.
 *   ws: cliora_vocab_workspace_bytes(T, V, E, want_backward) bytes; every byte read is written first.  With al(x) = x rounded up to
 *   256, c = ceil(E / 32), F = 2048 c (one packed 16-row tile), qt = ceil(T / 64), kt = ceil(V / 256), q4 = ceil(T / 256):
 *     forward  = 2 al(4 qt F) + al(16 kt F) + al(8 T ceil(kt / 8)) + al(4 T ceil(kt / 8))
 *     backward = al(16 q4 F) + al(16 kt F) + al(4 T) + al(16384 ceil(E / 16) kt) + al(16384 ceil(E / 16) q4)
 *                + al(64 ceil(E / 16) max(ceil(kt / r) 64 qt, ceil(q4 / 16) 64 ceil(V / 64))),  r = 2 for kt <= 64, 16 for kt >= 512,
 *                  ceil(kt / 32) between
 *   and the size is `forward`, or max(forward, backward) with want_backward (0 for T < 0, V < 1, E < 1).
 *   Refused before any launch with CLIORA_EINVAL: T < 0, V < 1, E < 1, a leading dimension below E, a NULL argument (rank may be
 *   and lse_lo may be NULL; with T = 0 only K, loss, status and ws are needed); CLIORA_ENOMEM: ws_bytes below the size above. */
size_t cliora_vocab_workspace_bytes(int T, int V, int E, int want_backward);
int cliora_vocab_nll_forward(int T, int V, int E, const float* Q, int64_t ldq, const float* K, int64_t ldk, const int64_t* tok,
                             const float* w, float* loss, float* nll, float* lse, float* lse_lo, float* tgt, int32_t* rank, int32_t* status,
                             void* ws, size_t ws_bytes, void* stream);

/* Its gradients for the upstream cotangent g (one fp32 on the device), from lse and lse_lo (or NULL: zeros) of the forward (nothing
 * else is kept): with p[t][v] = exp((s[t][v] - lse[t]) - lse_lo[t]) recomputed tile by tile -- each score the forward's chain, the
 * word's block its A operand on either side, so the same bits -- and wsel[t] = w[t] on the tokens that count (w[t] != 0, tok[t] inside
 * [0, V)), 0 elsewhere,
 *   dQ[t] = g wsel[t] sum_v (p[t][v] - [v == tok[t]]) K[v],     dK[v] = g sum_t wsel[t] (p[t][v] - [v == tok[t]]) Q[t].
 *   dQ (T, E) at lddq, dK (V, E) at lddk: written, not accumulated; either may be NULL and is then skipped (the other half is
 *   bitwise what it is with both).  One kernel, the stationary side a template parameter (tokens: dQ, words: dK): 64 stationary rows
 *   per workgroup, the other side streamed 256 rows at a time, the coefficients through the LDS score tile into a second MFMA product
 *   against the streamed operand packed along its rows; ranges of r x 256 words for dQ (about 32 ranges, so that a batch's few token tiles fill the device) and of
 *   16 x 256 tokens for dK (a function of the streamed side's size
 *   alone) give partials that a second kernel adds in ascending order.  Widths above 448 take ceil(E / 448) passes over the output
 *   columns, each computing the scores again.  No float atomics; a token's dQ row is bitwise the same whatever else is in the call.
 *   ws: cliora_vocab_workspace_bytes(T, V, E, 1) bytes (it may be the forward's; its contents are not needed).  Refusals as above. */
int cliora_vocab_nll_backward(int T, int V, int E, const float* Q, int64_t ldq, const float* K, int64_t ldk, const int64_t* tok,
                              const float* w, const float* lse, const float* lse_lo, const float* g, float* dQ, int64_t lddq, float* dK,
                              int64_t lddk, void* ws, size_t ws_bytes, void* stream);

/* Corpus token counts, the frequency vector of the reference's negative sampler (cliora/blocks/negative_sampler.py:15-24): ids (n)
 * int64 on the device -> counts (V) fp32, counts[v] = the number of ids equal to v, converted from an exact integer count (so the
 * reference's np.asarray(counts, float32) bit for bit).  Counted with integer atomics in LDS for V <= 16384, in HBM above.  Ids
 * outside [0, V) are not counted there: their number goes to *n_out_of_range (one int64 on the device, zeroed by the call), which
 * the caller must check.  n < 2^32.  Asynchronous on `stream`. */
int cliora_token_counts(int64_t n, const int64_t* ids, int V, float* counts, int64_t* n_out_of_range, void* stream);

/* S independent draws of k distinct ids from [0, V) without replacement, each new id drawn in proportion to its weight among those
 * not yet drawn -- numpy's legacy RandomState.choice(V, k, replace=False, p=w / sum(w)) (negative_sampler.py:36-37), in law.
 *   w (V) fp32 on the device, >= 0 and finite, any scale (the reference's freq**power + eps / V unnormalised); n_positive: the number
 *   of w > 0, which the caller knows; 1 <= k <= min(1024, n_positive), else CLIORA_EINVAL ("Fewer non-zero entries in p than size"
 *   as numpy words it), checked before any device call.  Zero weights are never drawn.
 *   Draw s is the exponential race E_i = -log(u_i) / w_i (double), its ids the k smallest (E, id) in ascending order (the draw order
 *   of the successive sampling).  u_i = (m + 0.5) 2^-53, m = (x0 >> 5) 2^26 + (x1 >> 6), x = Philox4x32-10 of counter
 *   (i, d_lo, d_hi, stream_id), key (seed_lo, seed_hi), d = offset + s.  So a draw depends on (seed, stream_id, d) alone: not on S,
 *   on the launch geometry or on the other draws of the call.
 *   ids_out (S, k) int64; keys_out (S, k) fp64 or NULL: the selected E.  No V-long key vector is written: blocks of 1024 ids
 *   (up to 4096 for k > 256) keep their k smallest (bitonic sort in LDS), and merge launches reduce the per-block lists (4 launches
 *   at V = 400k, k = 100).
 *   ws: cliora_neg_sample_workspace_bytes(V, S, k) bytes of device workspace (0 when V <= 4096, and for invalid arguments). */
size_t cliora_neg_sample_workspace_bytes(int V, int S, int k);
int cliora_neg_sample(int V, const float* w, int n_positive, int S, int k, uint64_t seed, uint64_t offset, uint32_t stream_id,
                      int64_t* ids_out, double* keys_out, void* ws, size_t ws_bytes, void* stream);

/* Optional HIP-event timing of one kernel class (used by bench.py for the roofline
 * line): enable, run steps, then read the accumulated device time and launch count. */
int cliora_prof_enable(int kernel_class, int on);
int cliora_prof_read(int kernel_class, double* total_ms, long long* launches, void* stream);
#define CLIORA_KCLASS_COMPOSE_FWD 0
#define CLIORA_KCLASS_COMPOSE_BWD 1
#define CLIORA_KCLASS_WGRAD 2
#define CLIORA_KCLASS_COUNT 3

const char* cliora_last_error(void);
/* Arithmetic of the compose-layer GEMMs (y = W2 x, dx = W2^T dz) and of the pair weight gradient dW2 = dz^T x:
 *   CLIORA_MFMA_SPLIT_BF16 (default): every fp32 operand is carried as two bf16 (hi + lo) and a product is three
 *     v_mfma_f32_16x16x32_bf16 with fp32 accumulation (operand rounding 2^-18; outputs stay within 1e-4 of the reference --
 *     2e-5 measured; gradient elements ~1e-5 of their tensor's scale in the median, single elements up to a few 1e-2 where
 *     a ReLU pre-activation within ~1e-5 of zero changes sign: DESIGN.md section 5);
 *   CLIORA_MFMA_F32: the fp32-input MFMA (products exact in fp32) -- the reference's arithmetic (cliora/net/diora.py:65-68
 *     nn.Linear in fp32), ~1.25x slower per step.
 * Everything else on the path (cell projections, scores, softmax, norms) is fp32 in both modes.
 * Process-wide; the environment variable CLIORA_MFMA=f32|bf16x3 sets the initial value.  Returns the previous mode. */
#define CLIORA_MFMA_F32 0
#define CLIORA_MFMA_SPLIT_BF16 1
int cliora_set_mfma_mode(int mode);

/* Scheduling of the two passes.  Outside level t only reads inside levels <= L-2-t (cliora/net/outside_index.py:39-127), so the
 * outside pass (and, in the backward, the inside pass's backward) can run one step behind the other pass instead of after it:
 * two dependent chains on two HIP streams (the caller's and one owned by the library, forked and joined by events inside every
 * call, so the caller's stream semantics are unchanged).  CLIORA_WAVEFRONT_AUTO (default; the environment variable
 * CLIORA_WAVEFRONT=0|1 sets the initial value) uses two streams when a level carries enough work to pay for the events;
 * OFF runs the reference's order on the caller's stream alone.  Results are bitwise identical either way.  Process-wide;
 * returns the previous mode. */
#define CLIORA_WAVEFRONT_AUTO (-1)
#define CLIORA_WAVEFRONT_OFF 0
#define CLIORA_WAVEFRONT_ON 1
/* MERGED (DioraMLP and CLIORA plans, R >= 0): the same wavefront on ONE queue -- step k of the FORWARD runs ONE compose grid over
 * inside level k and outside level L-k and ONE projection / score grid for both, on the caller's stream (CLIORA plans: the region
 * attention of the new inside cells, cliora.py:140-157, between the two grids): no side stream and no cross-stream event per step.
 * AUTO takes it wherever the two-stream form would pay; ON keeps the two streams.  TreeLSTM plans and compress = True treat MERGED
 * as ON (two streams); the backward always runs its two chains on two streams.  Bitwise the same results again
 * (CLIORA_WAVEFRONT=2). */
#define CLIORA_WAVEFRONT_MERGED 2
int cliora_set_wavefront(int mode);

/* One workgroup per sentence.  For a text-only DioraMLP plan whose rows fit a wavefront (D <= 64; BASELINE configs[0]) the level
 * loops of the forward (cliora/net/diora.py:312-331, 378-398) and of the backward run inside ONE launch each, a workgroup walking
 * every level of one sentence's chart with workgroup barriers between them (csrc/resident_kernels.hpp): sentences exchange nothing
 * inside the recursion.  AUTO (the default; CLIORA_RESIDENT=0|1 sets the initial value) takes it for short sentences
 * (CLIORA_RESIDENT_MAX_PAIRS span pairs per sentence, both passes) or batches of at least half as many sentences as the device has
 * compute units, OFF never, ON for every shape the kernels cover.  Same buffers
 * and formats as the launch-per-level path, exact fp32 FMA arithmetic, results equal to fp32 rounding.  Process-wide; returns the
 * previous mode. */
#define CLIORA_RESIDENT_AUTO (-1)
#define CLIORA_RESIDENT_OFF 0
#define CLIORA_RESIDENT_ON 1
int cliora_set_resident(int mode);

/* Float offset of a named region of the forward workspace ("pi", "po", "hp", "hp_o", "sp", "pp", "ymask", "nrmi", "nrmo", "t",
 * "qrleaf", "total"), for tests and tooling that compare two runs region by region; (size_t)-1 for an unknown name. */
size_t cliora_plan_fwd_offset(const cliora_plan* plan, const char* name);

/* Bytes of device index tables the plan uploads at its first use. */
size_t cliora_plan_device_bytes(const cliora_plan* plan);

/* A stream of the library's, on the current device, for work of the CALLER that is independent of the chart call it surrounds (the
 * word branch of cliora/net/cliora.py:459-461 and trainer.py:139-171: word projections, word-region scorer, VG loss gradient; the
 * region-matrix half of the span-region scorer's backward): chosen once per device so that it runs concurrently with `caller_stream`
 * and with the two streams the chart calls fork onto.  The caller orders it against its own streams with events (torch:
 * torch.cuda.ExternalStream(handle), wait_stream); the library never waits on it.  The handle stays valid for the life of the process. */
int cliora_device_side_stream(void* caller_stream, void** out);

/* Diagnostics: the wall-clock stamps (100 MHz) the sentence-resident kernels leave when CLIORA_RES_TRACE=1 (tools/resident_trace.py):
 * copies `count` 64-bit words of the device's stamp buffer to `out` (host) after synchronising `stream`. */
int cliora_resident_trace(cliora_plan* plan, unsigned long long* out, size_t count, void* stream);

/* The launch record: which kernel instances the run-time dispatchers chose.  Each rule of csrc/gemm_launch.hpp and
 * csrc/api_mlp_launch.hpp turns a width or a row count into a template instance; while the record is on, every launch of theirs notes
 * the kernel's name with its template arguments as chosen -- "level_compose_bwd<5,0,f32>", "rows_gemm_ksplit<2,4,frag>",
 * "tn_gemm_dma3x<7,9,5>(two ranges)", "tn_gemm<2,2,colsum>", "level_project<5,2,short>" -- so that a test can hold its shape to the
 * instance it was written for (tests/dispatch_cases.py).  The vision-language entries note theirs as well (tests/vl_cases.py): the
 * attention launches "cell_attend_fwd<9>", "cell_attend_bwd<16>", "obj_grad_reduce<9>" (regions per wave), cliora_vl_scores_backward
 * "region_segments(one)" or "region_segments(several x2)" (the LDS segments of the region axis), cliora_vl_scores_max_backward
 * "region_max_bwd_obj(nchunk 7)", the scorer GEMMs "rows_gemm_ws<4,5,8>", "rows_gemm_ws3<5,4,25>", "tn_gemm(ij)<4,5,nocolsum>".
 * Host code only, process-wide, safe with several host threads; off (the default) it costs one flag test per launch.
 * cliora_launch_record(on): turns it on (and clears what was recorded) or off; returns the previous state.
 * cliora_launch_record_read: the distinct entries, sorted, one per line, NUL-terminated, into buf[cap]; *needed (optional) gets the bytes
 * that takes.  buf == NULL with needed: the size alone.  CLIORA_EINVAL if buf is too small. */
int cliora_launch_record(int on);
int cliora_launch_record_read(char* buf, size_t cap, size_t* needed);

const char* cliora_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CLIORA_CHART_H */
