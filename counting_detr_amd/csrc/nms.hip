// Greedy non-maximum suppression ahead of the emit (infer.py --nms_iou): a filter on prob [B, Q] that runs before anything else reads it.
//
// cdetr_nms_suppress : per image of the batch, the queries with prob >= threshold are walked in the evaluation order (descending prob, equal
//   probabilities in ascending query order); one is suppressed when its float64 IoU with an earlier SURVIVING one is > iou.  prob_out is prob
//   with the suppressed entries replaced by NaN -- which cdetr_emit_detections, cdetr_count_sweep and the host loop never count --, removed
//   their number per image.
//
// Everything must EQUAL the host rule (counting_detr_amd/nms.py): the boxes are the evaluation boxes of detections.hip (single fp32
// multiplies, truncation, coco_ap.reference_box in integers), the IoU is records.h's, operation by operation, so contraction is switched off
// for this translation unit.  No atomics: every output has one writer, and nothing is read from prob_out.
//
// One workgroup = one image.  The candidates are compacted and sorted in LDS as in the emit kernel (records.h).  Rank r then belongs to thread
// r % 1024, which keeps its box in registers (Q <= 4096: at most 4 ranks a thread), so the 64 ranks of chunk c are slot c / 16 of wave c % 16.
// Per chunk that wave puts its 64 boxes into LDS and resolves them among themselves, one wave-uniform step per surviving rank; then every
// thread tests its own later candidates against the chunk's survivors and marks the ones they suppress, which are never suppressors
// themselves.  Two barriers a chunk (the chunk buffer is double-buffered).  LDS: 32 KiB keys + 4 KiB boxes + 4 KiB flags.
#pragma clang fp contract(off)

#include <cmath>

#include "records.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int NMS_MAX_Q = 4096;           // keys of one image in LDS: 4096 x 8 B = 32 KiB (the emit kernel's limit)
constexpr int NMS_THREADS = 1024;
constexpr int NMS_WAVES = NMS_THREADS / 64;
constexpr int NMS_SLOTS = NMS_MAX_Q / NMS_THREADS;

struct dbox {
    double x, y, w, h;
};

// box_iou_xywh(a, s) > iou.  Where the intersection is empty the IoU is 0 whatever the union, and 0 > iou is false for every iou >= 0: the
// division is only performed for boxes that meet, and then it is the checker's.
__device__ __forceinline__ bool suppresses(const dbox& a, const dbox& s, double iou) {
    const double w = fmin(a.x + a.w, s.x + s.w) - fmax(a.x, s.x);
    const double h = fmin(a.y + a.h, s.y + s.h) - fmax(a.y, s.y);
    if (!(w > 0.0 && h > 0.0)) return false;
    return iou_xywh(a.x, a.y, a.w, a.h, s.x, s.y, s.w, s.h) > iou;
}

__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(cdetr_nms_suppress_desc p) {
    __shared__ unsigned long long key[NMS_MAX_Q];
    __shared__ dbox sbox[2][64];
    __shared__ unsigned long long surv_s[2];
    __shared__ unsigned char gone[NMS_MAX_Q];
    __shared__ int red[NMS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ pr = p.prob + (size_t)b * p.Q;
    const float* __restrict__ bx = p.boxes + (size_t)b * p.Q * 4;
    const float H = (float)p.orig_hw[2 * b], W = (float)p.orig_hw[2 * b + 1];
    const double iou = p.iou;

    // the candidates' keys in query order: ballot + prefix inside a wave, the waves' counts through LDS, 1024 queries per round
    int cnt = 0;
    for (int q0 = 0; q0 < p.Q; q0 += NMS_THREADS) {
        const int q = q0 + tid;
        const float pq = q < p.Q ? pr[q] : 0.0f;
        const bool k = q < p.Q && pq >= p.threshold;    // false for a NaN
        const unsigned long long m = __ballot(k);
        __syncthreads();                                // `red` of the previous round has been read
        if (lane == 0) red[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < NMS_WAVES; ++w) {
            before += w < wave ? red[w] : 0;
            total += red[w];
        }
        if (k) key[cnt + before + __popcll(m & ((1ull << lane) - 1ull))] = sort_key(pq, q);
        cnt += total;
    }
    sort_keys<NMS_THREADS>(key, cnt);                   // the walk's order; cnt <= Q <= 4096

    // rank r = tid + 1024 k is slot k of this thread: its query and its evaluation box, the integers widened to float64
    dbox own[NMS_SLOTS];
    int oq[NMS_SLOTS];
    unsigned dead = 0;                                  // bit k: slot k is a candidate that has been suppressed
#pragma unroll
    for (int k = 0; k < NMS_SLOTS; ++k) {
        const int r = tid + k * NMS_THREADS;
        oq[k] = 0;
        own[k] = dbox{0.0, 0.0, 0.0, 0.0};
        if (r < cnt) {
            const int q = (int)(unsigned)(key[r] & 0xffffffffull);
            const float* __restrict__ bq = bx + 4 * (size_t)q;
            const int cx = (int)(bq[0] * W), cy = (int)(bq[1] * H), w = (int)(bq[2] * W), h = (int)(bq[3] * H);
            const long long x2 = 2ll * cx - w, y2 = 2ll * cy - h;
            oq[k] = q;
            own[k] = dbox{(double)(x2 / 2), (double)(y2 / 2), (double)w, (double)h};
        }
    }

    const int chunks = (cnt + 63) >> 6;
    for (int c = 0; c < chunks; ++c) {
        const int ow = c % NMS_WAVES, ok = c / NMS_WAVES, buf = c & 1;       // the chunk's ranks: slot ok of wave ow, lane by lane
        dbox me = own[0];
#pragma unroll
        for (int k = 1; k < NMS_SLOTS; ++k)
            if (k == ok) me = own[k];
        if (wave == ow) sbox[buf][lane] = me;
        __syncthreads();
        if (wave == ow) {
            // inside the chunk: rank j, if it still stands when its turn comes, takes out the later lanes it overlaps
            bool alive = c * 64 + lane < cnt && !((dead >> ok) & 1u);
            for (int j = 0; j < 63; ++j) {
                const unsigned long long a = __ballot(alive);
                if ((a >> j) <= 1ull) {                 // nobody stands behind j
                    break;
                }
                if (!((a >> j) & 1ull)) continue;       // wave-uniform
                if (alive && lane > j && suppresses(me, sbox[buf][j], iou)) alive = false;
            }
            if (c * 64 + lane < cnt && !alive) dead |= 1u << ok;
            const unsigned long long s = __ballot(alive);
            if (lane == 0) surv_s[buf] = s;
        }
        __syncthreads();
        // the chunk's survivors against everything ranked behind the chunk
        const unsigned long long s = surv_s[buf];
        const int end = (c + 1) * 64;
        unsigned live = 0;
#pragma unroll
        for (int k = 0; k < NMS_SLOTS; ++k) {
            const int r = tid + k * NMS_THREADS;
            if (r >= end && r < cnt && !((dead >> k) & 1u)) live |= 1u << k;
        }
        for (unsigned long long m = s; m != 0 && __any(live != 0); m &= m - 1) {
            const int j = __ffsll((long long)m) - 1;   // wave-uniform: one LDS broadcast per survivor
            const dbox sv = sbox[buf][j];
#pragma unroll
            for (int k = 0; k < NMS_SLOTS; ++k)
                if (((live >> k) & 1u) && suppresses(own[k], sv, iou)) {
                    live &= ~(1u << k);
                    dead |= 1u << k;
                }
        }
    }

    // write back: one flag byte per query, then prob_out in query order with the bits of everything that was not suppressed
    for (int q = tid; q < p.Q; q += NMS_THREADS) gone[q] = 0;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int k = 0; k < NMS_SLOTS; ++k)
        if ((dead >> k) & 1u) {
            gone[oq[k]] = 1;
            ++n;
        }
    n = block_sum<NMS_WAVES>(n, red);                   // its barriers also publish `gone`
    const unsigned* __restrict__ bits = reinterpret_cast<const unsigned*>(pr);
    unsigned* __restrict__ out = reinterpret_cast<unsigned*>(p.prob_out + (size_t)b * p.Q);
    for (int q = tid; q < p.Q; q += NMS_THREADS) out[q] = gone[q] ? 0x7fc00000u : bits[q];
    if (tid == 0) p.removed[b] = n;
}

}  // namespace

extern "C" int cdetr_nms_suppress(const cdetr_nms_suppress_desc* d, void* stream) {
    CDETR_CHECK_ARG(d != nullptr, "cdetr_nms_suppress: null descriptor");
    CDETR_CHECK_ARG(d->B > 0 && d->Q > 0, "cdetr_nms_suppress: bad sizes B = %d, Q = %d", d->B, d->Q);
    if (d->Q > NMS_MAX_Q || d->B > STORE_MAX_B) {
        cdetr_set_error("cdetr_nms_suppress: Q = %d queries (limit %d) or B = %d images per call (limit %d) not supported", d->Q, NMS_MAX_Q, d->B,
                        STORE_MAX_B);
        return CDETR_ERR_UNSUPPORTED;
    }
    CDETR_CHECK_ARG(std::isfinite(d->iou) && d->iou >= 0.0 && d->iou <= 1.0, "cdetr_nms_suppress: iou = %g is not a number in [0, 1]", d->iou);
    CDETR_CHECK_ARG(d->threshold == d->threshold, "cdetr_nms_suppress: the threshold is NaN");
    CDETR_CHECK_ARG(d->prob && d->boxes && d->orig_hw && d->prob_out && d->removed, "cdetr_nms_suppress: null pointer");
    CDETR_CHECK_ARG(d->prob_out != d->prob, "cdetr_nms_suppress: prob_out must not alias prob");
    hipLaunchKernelGGL(nms_kernel, dim3(d->B), dim3(NMS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *d);
    return cdetr_launch_status("cdetr_nms_suppress");
}
