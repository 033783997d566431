// criterion_eval.hip -- SetCriterion for evaluation: the losses every image of a batch would get ALONE, forward only, one launch.
//
// cdetr_criterion_eval: grid = B, workgroup b computes what A2/models/anchor_detr.py:143-367 returns for image b evaluated as a batch of
// one (the reference's inference driver runs one image per call, A2/infer.py:27-122): the normaliser is max(T_b, 1) from tgt_off, the
// means of the variance loss run over image b's own min(Q, T_b) pairs, cardinality_error is |#object queries of b - T_b|.  No gradients are
// formed or written (criterion.hip's cdetr_criterion_fwd zero-fills and writes five gradient tensors, walks the whole batch with one
// workgroup and is limited to B <= 64).  The expressions and the summation order are criterion_fwd_kernel's at B == 1, term by term: 256
// threads stride over the image's Q rows / its pairs, per-wave shuffle tree, then a serial sum over the waves -- bit-reproducible, and row b
// does not depend on the other images of the batch.  The counts are read from device memory (tgt_off): a capacity plan (ops.MatchPlan.capacity)
// and a captured graph serve any target counts.
#include "../../include/cdetr_hip.h"
#include "common.h"

namespace {

constexpr int NT = 256;                          // threads of a workgroup: the stride of every loop and the four waves of block_sums
constexpr int NRED = 10;
enum { R_CE = 0, R_CARD, R_L1, R_GIOU, R_CORRECT, R_DW, R_DH, R_IW, R_IH, R_LOGS };

__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// block-wide ordered sums of v[0..N) into red[slot0..slot0+N) (called by all threads; one barrier pair for the N values)
template <int N>
__device__ __forceinline__ void block_sums(const float (&v)[N], float* wred, float* red, int slot0, int tid) {
    constexpr int nw = NT >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float s = wave_sum(v[k]);
        if ((tid & 63) == 0) wred[(tid >> 6) * NRED + slot0 + k] = s;
    }
    __syncthreads();
    if (tid < N) {
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += wred[w * NRED + slot0 + tid];
        red[slot0 + tid] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void criterion_eval_kernel(const cdetr_criterion_eval_desc d) {
    extern __shared__ int tcls[];                    // [Q] target class of every query of THIS image (num_classes = no object)
    __shared__ float wred[(NT >> 6) * NRED], red[NRED];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Q = d.Q, C = d.C;
    const int t0 = d.tgt_off[b];
    const int T = max(d.tgt_off[b + 1] - t0, 0);
    const int K = min(min(Q, T), d.Mmax);            // pairs of this image (uniform)
    const float inv_nb = 1.f / fmaxf((float)T, 1.f); // the reference's num_boxes of a batch of one (:321-325)
    const float* logits = d.logits + (long)b * Q * C;
    const float* boxes = d.boxes + (long)b * Q * 4;
    const float* vars = d.vars + (long)b * Q * 2;
    const int64_t* idx_i = d.idx_i + (long)b * d.Mmax;
    const int64_t* idx_j = d.idx_j + (long)b * d.Mmax;

    for (int i = tid; i < Q; i += NT) tcls[i] = d.num_classes;
    __syncthreads();
    // ---- matched pairs -> target classes (a pair outside [0, Q) x [0, T) -- an unsolved assignment -- is skipped everywhere)
    for (int m = tid; m < K; m += NT) {
        const long q = idx_i[m], j = idx_j[m];
        if (q >= 0 && q < Q && j >= 0 && j < T) tcls[q] = (int)d.tgt_labels[t0 + j];
    }
    __syncthreads();
    // ---- focal loss over every (q, c) + the number of "object" queries
    float ce_card[2] = {0.f, 0.f};
    for (int r = tid; r < Q; r += NT) {
        const int tc = tcls[r];
        float best = -INFINITY;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            const float x = logits[(long)r * C + c];
            if (x > best) { best = x; arg = c; }
            const float t = (c == tc) ? 1.f : 0.f;
            const float p = 1.f / (1.f + expf(-x));
            const float ce = softplusf(x) - x * t;                     // BCE with logits
            const float pt = p * t + (1.f - p) * (1.f - t);
            const float m = 1.f - pt;
            const float at = d.alpha * t + (1.f - d.alpha) * (1.f - t);
            ce_card[0] += at * ce * m * m;
        }
        ce_card[1] += (arg != C - 1) ? 1.f : 0.f;                     // whole numbers <= Q: exact in fp32
    }
    block_sums(ce_card, wred, red, R_CE, tid);
    // ---- matched pairs: L1, GIoU, accuracy, statistics of the variance loss
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};             // l1, giou, correct, dw, dh, 1/|v0|, 1/|v1|, |log|
    for (int m = tid; m < K; m += NT) {
        const long q = idx_i[m], j = idx_j[m];
        if (!(q >= 0 && q < Q && j >= 0 && j < T)) continue;
        const long t = t0 + j;
        const float4 sb = *reinterpret_cast<const float4*>(boxes + q * 4);
        const float4 tb = *reinterpret_cast<const float4*>(d.tgt_boxes + t * 4);
        const float e0 = sb.x - tb.x, e1 = sb.y - tb.y, e2 = sb.z - tb.z, e3 = sb.w - tb.w;
        s[0] += fabsf(e0) + fabsf(e1) + fabsf(e2) + fabsf(e3);
        // GIoU on xyxy
        const float x1 = sb.x - 0.5f * sb.z, y1 = sb.y - 0.5f * sb.w, x2 = sb.x + 0.5f * sb.z, y2 = sb.y + 0.5f * sb.w;
        const float u1 = tb.x - 0.5f * tb.z, v1 = tb.y - 0.5f * tb.w, u2 = tb.x + 0.5f * tb.z, v2 = tb.y + 0.5f * tb.w;
        const float a1 = (x2 - x1) * (y2 - y1), a2 = (u2 - u1) * (v2 - v1);
        const float iw = fmaxf(fminf(x2, u2) - fmaxf(x1, u1), 0.f), ih = fmaxf(fminf(y2, v2) - fmaxf(y1, v1), 0.f);
        const float inter = iw * ih;
        const float uni = a1 + a2 - inter;
        const float iou = inter / uni;
        const float cw = fmaxf(fmaxf(x2, u2) - fminf(x1, u1), 0.f), ch = fmaxf(fmaxf(y2, v2) - fminf(y1, v1), 0.f);
        const float area = cw * ch;
        s[1] += 1.f - (iou - (area - uni) / area);
        // accuracy of the matched query (first-maximum argmax)
        {
            float best = -INFINITY;
            int arg = 0;
            for (int c = 0; c < C; ++c) {
                const float x = logits[q * C + c];
                if (x > best) { best = x; arg = c; }
            }
            s[2] += (arg == (int)d.tgt_labels[t]) ? 1.f : 0.f;
        }
        const float v0 = vars[q * 2], v1v = vars[q * 2 + 1];
        s[3] += fabsf(e2);
        s[4] += fabsf(e3);
        s[5] += 1.f / fabsf(v0);
        s[6] += 1.f / fabsf(v1v);
        s[7] += fabsf(logf(v0)) + fabsf(logf(v1v));                    // log of a negative variance: NaN, as in the reference
    }
    block_sums(s, wred, red, R_L1, tid);
    if (tid == 0) {
        float* out = d.losses + (long)b * 7;
        const float Kf = (float)K;
        const float mw = red[R_DW] / Kf, mh = red[R_DH] / Kf;          // NaN when K == 0 (never used then)
        out[0] = red[R_CE] / (float)Q * inv_nb * (float)Q;             // .mean(1).sum() / nb * Q
        out[1] = K > 0 ? 100.f - red[R_CORRECT] * (100.f / Kf) : 100.f;
        out[2] = fabsf(red[R_CARD] - (float)T);
        out[3] = red[R_L1] * inv_nb;
        out[4] = red[R_GIOU] * inv_nb;
        out[5] = K > 0 ? (mw * red[R_IW] + mh * red[R_IH] + red[R_LOGS]) * inv_nb : 0.f;
        float tot = 0.f;
        if (d.loss_weights)                           // the weighted total (A2/engine.py:37), as cdetr_criterion_fwd forms it
            for (int k = 0; k < 6; ++k) tot += d.loss_weights[k] != 0.f ? d.loss_weights[k] * out[k] : 0.f;
        out[6] = tot;
    }
}

}  // namespace

extern "C" int cdetr_criterion_eval(const cdetr_criterion_eval_desc* dp, void* stream) {
    CDETR_CHECK_ARG(dp != nullptr, "cdetr_criterion_eval: null descriptor");
    const cdetr_criterion_eval_desc d = *dp;
    CDETR_CHECK_ARG(d.B > 0 && d.Q > 0 && d.C > 0 && d.Mmax > 0, "cdetr_criterion_eval: bad sizes");
    CDETR_CHECK_ARG((long)d.Q * 4 <= 160 * 1024 - 4096, "cdetr_criterion_eval: Q too large for one workgroup's LDS");
    CDETR_CHECK_ARG(d.logits && d.boxes && d.vars && d.tgt_boxes && d.tgt_labels && d.tgt_off && d.idx_i && d.idx_j && d.losses,
                    "cdetr_criterion_eval: null pointer");
    const int bytes = d.Q * 4;
    if (bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(criterion_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) {
            cdetr_set_error("cdetr_criterion_eval: hipFuncSetAttribute(%d): %s", bytes, hipGetErrorString(e));
            return CDETR_ERR_LAUNCH;
        }
    }
    hipLaunchKernelGGL(criterion_eval_kernel, dim3(d.B), dim3(NT), bytes, reinterpret_cast<hipStream_t>(stream), d);
    return cdetr_launch_status("cdetr_criterion_eval");
}
