// Evaluation kernel of the vision-language parse script (cliora/scripts/parse.py:176-264): per gold phrase the region box its words
// attend to most, the IoU of that box with the phrase's gold box, the phrase's CCRA flag; per predicted constituent the box chosen by
// the same rule; per sentence the integer counts of the span F1.  One workgroup per sentence; everything it reads is at most L rows of
// R scores, R boxes and the sentence's phrase / span lists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cliora {

constexpr int GROUND_THREADS = 256;

// torch's CPU max(dim): the first maximal element wins, a NaN counts as larger than every number (the first NaN wins).
// (v, i) beats the running (w, j)?
__device__ __forceinline__ bool ground_beats(float v, int i, float w, int j) {
    const bool vn = v != v, wn = w != w;
    if (vn || wn) return vn && (!wn || i < j);
    return v > w || (v == w && i < j);
}

// torchvision.ops.box_iou of one pair in its operation order (areas, clamp(rb - lt, min=0), w * h, a1 + a2 - inter, inter / union),
// fp32 (the unit is compiled with -ffp-contract=off: no fused multiply-adds).  a = the selected box, g = the gold box.
__device__ __forceinline__ float ground_iou(const float* a, const float* g) {
    const float a1 = (a[2] - a[0]) * (a[3] - a[1]);
    const float a2 = (g[2] - g[0]) * (g[3] - g[1]);
    float w = fminf(a[2], g[2]) - fmaxf(a[0], g[0]);
    float h = fminf(a[3], g[3]) - fmaxf(a[1], g[1]);
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float inter = w * h;
    const float uni = a1 + a2 - inter;
    return inter / uni;
}

// First word of [s, e) whose row maximum is the largest (parse.py:180-182, 241-243); the rows' maxima are in LDS.
__device__ __forceinline__ int ground_pick_word(const float* rowmax, int s, int e) {
    int w = s;
    for (int l = s + 1; l < e; ++l)
        if (ground_beats(rowmax[l], l, rowmax[w], w)) w = l;
    return w;
}

// atten (B, L, R) at element strides (sb, sl, sr): DioraMLP.atten_score is a permuted diagonal of vg_atten_score, read in place.
// phr_out (P, 4): selected word, selected box, hit, ccr; a phrase outside 0 <= start < end <= L gets (-1, -1, 0, 0) and is counted
// in *status.  span_box (B, L-1) / span_xyxy (B, L-1, 4): the box of every predicted span (the root's too).  sent_out (B, 3):
// |pred & gold|, |pred|, |gold| over the span SETS, pred without its root (the last span).  atten == nullptr: counts only.
// lengths == nullptr: every sentence has L words (cliora_ground_eval).  Else (cliora_ground_eval_ragged) sentence b has n = lengths[b]
// words of a batch padded to L: its spans are rows 0 .. n-2 (the root row n-2), its words the first n rows of atten, a phrase must end
// at or before n, and the rows n-1 .. L-2 of span_box / span_xyxy are written as -1 / 0.  n outside [1, L]: one count in *status, no
// word, span or phrase of the sentence is read.
__global__ __launch_bounds__(GROUND_THREADS) void ground_eval_kernel(
        int L, int R, const float* __restrict__ atten, int64_t sb, int64_t sl, int64_t sr, const float* __restrict__ boxes,
        int P, const int32_t* __restrict__ phr_off, const int32_t* __restrict__ phr_span, const float* __restrict__ phr_box,
        const int32_t* __restrict__ spans, int G, const int32_t* __restrict__ gold_off, const int32_t* __restrict__ gold_span,
        int32_t* __restrict__ phr_out, int32_t* __restrict__ span_box, float* __restrict__ span_xyxy, int32_t* __restrict__ sent_out,
        int32_t* __restrict__ status, const int32_t* __restrict__ lengths) {
    extern __shared__ float rowmax[];             // L row maxima, then L first-argmax region ids
    int32_t* rowarg = reinterpret_cast<int32_t*>(rowmax + L);
    __shared__ int32_t cnt[3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NSL = L - 1;                        // span rows per sentence in the tables
    int nw = L;                                   // the sentence's words
    if (lengths) {
        nw = lengths[b];
        if (nw < 1 || nw > L) { nw = 0; if (tid == 0) atomicAdd(status, 1); }
    }
    const int NS = nw > 0 ? nw - 1 : 0;           // predicted spans of the sentence, the root last
    const int32_t* sp = spans + (size_t)b * NSL * 2;
    if (tid < 3) cnt[tid] = 0;
    // 1. per word: max over the regions and the first region attaining it (one wavefront per row)
    if (atten) {
        for (int l = wave; l < nw; l += GROUND_THREADS / 64) {
            const float* row = atten + (int64_t)b * sb + (int64_t)l * sl;
            float best = -INFINITY; int bi = 0x7fffffff;
            for (int r = lane; r < R; r += 64) {          // increasing r: a later equal value never replaces the lane's first
                const float v = row[(int64_t)r * sr];
                if (ground_beats(v, r, best, bi)) { best = v; bi = r; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
                if (ground_beats(ov, oi, best, bi)) { best = ov; bi = oi; }
            }
            if (lane == 0) { rowmax[l] = best; rowarg[l] = bi; }
        }
    }
    __syncthreads();
    // 2. gold phrases: box, IoU > 0.5 (NaN is no hit), CCRA = hit and (one word, or a predicted non-root span)
    int p0 = phr_off[b], p1 = phr_off[b + 1];
    p0 = min(max(p0, 0), P); p1 = min(max(p1, p0), P);
    for (int p = p0 + tid; p < p1; p += GROUND_THREADS) {
        const int s = phr_span[2 * p], e = phr_span[2 * p + 1];
        int32_t* o = phr_out + (size_t)4 * p;
        if (!atten || s < 0 || s >= e || e > nw) {
            o[0] = -1; o[1] = -1; o[2] = 0; o[3] = 0;
            atomicAdd(status, 1);
            continue;
        }
        const int w = ground_pick_word(rowmax, s, e);
        const int box = rowarg[w];
        const float iou = ground_iou(boxes + ((size_t)b * R + box) * 4, phr_box + (size_t)4 * p);
        const int hit = iou > 0.5f;
        int ccr = 0;
        if (hit) {
            ccr = e - 1 == s;
            for (int k = 0; k < NS - 1 && !ccr; ++k) ccr = sp[2 * k] == s && sp[2 * k + 1] == e - 1;
        }
        o[0] = w; o[1] = box; o[2] = hit; o[3] = ccr;
    }
    // 3. predicted spans: box of each; distinct non-root spans
    for (int k = tid; k < NS; k += GROUND_THREADS) {
        const int s = sp[2 * k], e = sp[2 * k + 1];
        const bool ok = s >= 0 && s <= e && e < nw;
        if (!ok) atomicAdd(status, 1);
        if (atten) {
            const int box = ok ? rowarg[ground_pick_word(rowmax, s, e + 1)] : -1;
            if (span_box) span_box[(size_t)b * NSL + k] = box;
            if (span_xyxy)
                for (int c = 0; c < 4; ++c) span_xyxy[((size_t)b * NSL + k) * 4 + c] = ok ? boxes[((size_t)b * R + box) * 4 + c] : 0.f;
        }
        if (ok && k < NS - 1) {
            bool first = true;
            for (int j = 0; j < k && first; ++j) first = !(sp[2 * j] == s && sp[2 * j + 1] == e);
            if (first) atomicAdd(&cnt[1], 1);
        }
    }
    if (atten)                                    // rows beyond the sentence's own spans (ragged batches only: NS == NSL otherwise)
        for (int k = NS + tid; k < NSL; k += GROUND_THREADS) {
            if (span_box) span_box[(size_t)b * NSL + k] = -1;
            if (span_xyxy)
                for (int c = 0; c < 4; ++c) span_xyxy[((size_t)b * NSL + k) * 4 + c] = 0.f;
        }
    // 4. distinct gold spans, and those among the predicted non-root spans
    int g0 = gold_off[b], g1 = gold_off[b + 1];
    g0 = min(max(g0, 0), G); g1 = min(max(g1, g0), G);
    for (int g = g0 + tid; g < g1; g += GROUND_THREADS) {
        const int s = gold_span[2 * g], e = gold_span[2 * g + 1];
        bool first = true;
        for (int j = g0; j < g && first; ++j) first = !(gold_span[2 * j] == s && gold_span[2 * j + 1] == e);
        if (!first) continue;
        atomicAdd(&cnt[2], 1);
        bool in = false;
        for (int k = 0; k < NS - 1 && !in; ++k) in = sp[2 * k] == s && sp[2 * k + 1] == e;
        if (in) atomicAdd(&cnt[0], 1);
    }
    __syncthreads();
    if (tid < 3) sent_out[(size_t)b * 3 + tid] = cnt[tid];
}

}  // namespace cliora
