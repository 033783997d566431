// Detections emitted on the device (infer.py --device_detections): what infer.py's per-image host loop, coco_ap.reference_box and the
// ordering of coco_ap.pack_images compute between the forward and the box-AP matcher, for a whole forwarded batch in one call.
//
// cdetr_emit_detections : per image of the batch, the queries with prob >= threshold become
//   wire records (query order; the fields of predictions_<split>.json) and evaluation records (descending score, equal scores in
//   ascending query order, cut at max_det; the float64 arrays cdetr_coco_match reads), appended to a device-resident store for the split.
//
// Everything must EQUAL the host path: the scalings are single fp32 multiplies followed by a truncation, the area is the fp32 product of
// the unrounded width and height.  A product contracted into an FMA with a later operation would differ, so contraction is switched
// off for this translation unit (as in coco_eval.hip).  No fast-math anywhere in the build.
//
// Placement is deterministic: a count kernel writes every image's number of kept queries, the emit kernel's workgroup b adds up the counts
// of the images before it -- no atomic decides where a record lands (the only atomic is the OR into the status word).
#pragma clang fp contract(off)

#include "common.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int EMIT_MAX_Q = 4096;          // keys of one image in LDS: 4096 x 8 B = 32 KiB
constexpr int EMIT_MAX_B = 65535;
constexpr int EMIT_MAX_CAP = 1 << 30;     // records: running sums stay inside int32 (2^30 + 65535 x 4096 < 2^31)
constexpr int EMIT_THREADS = 1024;
constexpr int EMIT_WAVES = EMIT_THREADS / 64;

// prob >= threshold, false for a NaN on either side (numpy's and torch's >=)
__device__ __forceinline__ bool kept(float p, float thr) { return p >= thr; }

// sum of `v` over the workgroup, the same value in every thread; `red` holds one int per wave.  Ends with a barrier-protected read: the
// caller may reuse `red` after its next __syncthreads().
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < nw; ++w) s += red[w];
    return s;
}

// counts[first + b] = number of kept queries of image b
__global__ __launch_bounds__(256) void emit_count_kernel(cdetr_emit_detections_desc p) {
    __shared__ int red[4];
    const int b = blockIdx.x;
    const float* __restrict__ pr = p.prob + (size_t)b * p.Q;
    int n = 0;
    for (int q = threadIdx.x; q < p.Q; q += 256) n += kept(pr[q], p.threshold) ? 1 : 0;
    n = block_sum(n, red);
    if (threadIdx.x == 0) p.counts[p.first + b] = n;
}

struct wire_fields {
    int cx, cy, w, h, area, px, py;
};

// infer.py's arithmetic: boxes[..., 0] *= ori_w ... in fp32 (one multiply each), int() of each; area = int(w * h) with the fp32 product
// of the UNtruncated w and h
__device__ __forceinline__ wire_fields wire_of(const float* __restrict__ box, const float* __restrict__ pt, float W, float H) {
    const float fx = box[0] * W, fy = box[1] * H, fw = box[2] * W, fh = box[3] * H;
    wire_fields r;
    r.cx = (int)fx; r.cy = (int)fy; r.w = (int)fw; r.h = (int)fh;
    r.area = (int)(fw * fh);
    r.px = (int)(pt[0] * W); r.py = (int)(pt[1] * H);
    return r;
}

// ascending key = descending score, equal scores by ascending query: high half = the inverted image of the score under the
// order-preserving map float -> uint32 (sign bit flipped for positives, all bits for negatives; -0 is made +0 first, the two compare equal)
__device__ __forceinline__ unsigned long long sort_key(float p, int q) {
    if (p == 0.0f) p = 0.0f;
    unsigned u = __float_as_uint(p);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)(~u) << 32) | (unsigned)q;
}

// One workgroup = one image of the batch.
__global__ __launch_bounds__(EMIT_THREADS) void emit_kernel(cdetr_emit_detections_desc p) {
    __shared__ unsigned long long key[EMIT_MAX_Q];
    __shared__ int red[EMIT_WAVES];
    const int b = blockIdx.x, n = p.first + b;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // where this image starts: the store's offsets at `first` (written by the previous call, in stream order) + the counts of the
    // batch's images before this one
    int sw = 0, se = 0;
    for (int j = threadIdx.x; j < b; j += EMIT_THREADS) {
        const int c = p.counts[p.first + j];
        sw += c;
        se += min(c, p.max_det);
    }
    sw = block_sum(sw, red);
    se = block_sum(se, red);
    const int start_w = p.wire_off[p.first], start_e = p.eval_off[p.first];
    const int cnt = p.counts[n];
    const int ecnt = min(cnt, p.max_det);
    const bool start_ok = start_w >= 0 && start_w <= p.wire_cap && start_e >= 0 && start_e <= p.eval_cap;
    const int w0 = start_w + sw, e0 = start_e + se;     // (start_ok: < 2^30 + B * Q, inside int32)
    if (threadIdx.x == 0) {
        p.wire_off[n + 1] = start_ok ? w0 + cnt : start_w;
        p.eval_off[n + 1] = start_ok ? e0 + ecnt : start_e;
    }
    const bool fits_w = start_ok && cnt >= 0 && cnt <= p.Q && w0 + cnt <= p.wire_cap;
    const bool fits_e = start_ok && e0 + ecnt <= p.eval_cap;
    if (!fits_w || !fits_e) {                           // uniform over the workgroup: nothing of this image is written
        if (threadIdx.x == 0) atomicOr(p.status, !start_ok ? 4 : ((fits_w ? 0 : 1) | (fits_e ? 0 : 2)));
        return;
    }

    const float* __restrict__ pr = p.prob + (size_t)b * p.Q;
    const float* __restrict__ bx = p.boxes + (size_t)b * p.Q * 4;
    const float* __restrict__ pt = p.points + (size_t)b * p.Q * 2;
    const float H = (float)p.orig_hw[2 * b], W = (float)p.orig_hw[2 * b + 1];

    // wire records in query order: ballot + prefix inside a wave, the waves' counts through LDS, 1024 queries per round
    int done = 0;
    for (int q0 = 0; q0 < p.Q; q0 += EMIT_THREADS) {
        const int q = q0 + threadIdx.x;
        const float pq = q < p.Q ? pr[q] : 0.0f;
        const bool k = q < p.Q && kept(pq, p.threshold);
        const unsigned long long m = __ballot(k);
        __syncthreads();                                // `red` of the previous round / of block_sum has been read
        if (lane == 0) red[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < EMIT_WAVES; ++w) {
            before += w < wave ? red[w] : 0;
            total += red[w];
        }
        const int pos = done + before + __popcll(m & ((1ull << lane) - 1ull));
        if (k && pos < cnt) {
            const wire_fields f = wire_of(bx + 4 * (size_t)q, pt + 2 * (size_t)q, W, H);
            int4* dst = reinterpret_cast<int4*>(p.wire + 8 * (size_t)(w0 + pos));
            dst[0] = make_int4(f.cx, f.cy, f.w, f.h);
            dst[1] = make_int4(f.area, f.px, f.py, __float_as_int(pq));
            key[pos] = sort_key(pq, q);
        }
        done += total;
    }
    if (ecnt == 0) return;

    // stable order by (score descending, query ascending): bitonic sort of the padded keys in LDS
    int npad = 1;
    while (npad < cnt) npad <<= 1;
    for (int i = cnt + threadIdx.x; i < npad; i += EMIT_THREADS) key[i] = ~0ull;
    __syncthreads();
    for (int k2 = 2; k2 <= npad; k2 <<= 1) {
        for (int j = k2 >> 1; j >= 1; j >>= 1) {
            for (int i = threadIdx.x; i < npad; i += EMIT_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = key[i], c = key[l];
                    if ((a > c) == ((i & k2) == 0)) { key[i] = c; key[l] = a; }
                }
            }
            __syncthreads();
        }
    }

    // evaluation records: coco_ap.reference_box on the wire integers ([int(cx - w/2), int(cy - h/2), w, h] = tdiv2(2 cx - w), ...: C++'s
    // integer division truncates toward zero like int()), area = w * h, score, as float64
    for (int r = threadIdx.x; r < ecnt; r += EMIT_THREADS) {
        const int q = (int)(unsigned)(key[r] & 0xffffffffull);
        const wire_fields f = wire_of(bx + 4 * (size_t)q, pt + 2 * (size_t)q, W, H);
        const long long x2 = 2ll * f.cx - f.w, y2 = 2ll * f.cy - f.h;
        double* bo = p.eval_boxes + 4 * (size_t)(e0 + r);
        bo[0] = (double)(x2 / 2);
        bo[1] = (double)(y2 / 2);
        bo[2] = (double)f.w;
        bo[3] = (double)f.h;
        p.eval_area[e0 + r] = (double)((long long)f.w * (long long)f.h);
        p.eval_score[e0 + r] = (double)pr[q];
    }
}

}  // namespace

extern "C" int cdetr_emit_detections(const cdetr_emit_detections_desc* d, void* stream) {
    CDETR_CHECK_ARG(d != nullptr, "cdetr_emit_detections: null descriptor");
    CDETR_CHECK_ARG(d->B > 0 && d->Q > 0 && d->N > 0 && d->first >= 0 && d->max_det >= 0 && d->wire_cap >= 0 && d->eval_cap >= 0,
                    "cdetr_emit_detections: bad sizes B = %d, Q = %d, N = %d, first = %d, max_det = %d, wire_cap = %d, eval_cap = %d", d->B, d->Q,
                    d->N, d->first, d->max_det, d->wire_cap, d->eval_cap);
    if (d->Q > EMIT_MAX_Q || d->B > EMIT_MAX_B) {
        cdetr_set_error("cdetr_emit_detections: Q = %d queries (limit %d) or B = %d images per call (limit %d) not supported", d->Q, EMIT_MAX_Q, d->B,
                        EMIT_MAX_B);
        return CDETR_ERR_UNSUPPORTED;
    }
    CDETR_CHECK_ARG((int64_t)d->first + d->B <= d->N, "cdetr_emit_detections: images %d .. %d do not fit a store of N = %d", d->first,
                    d->first + d->B - 1, d->N);
    CDETR_CHECK_ARG(d->wire_cap <= EMIT_MAX_CAP && d->eval_cap <= EMIT_MAX_CAP, "cdetr_emit_detections: capacities %d / %d exceed %d records",
                    d->wire_cap, d->eval_cap, EMIT_MAX_CAP);
    CDETR_CHECK_ARG(d->prob && d->boxes && d->points && d->orig_hw, "cdetr_emit_detections: null input pointer");
    CDETR_CHECK_ARG(d->counts && d->wire_off && d->eval_off && d->status, "cdetr_emit_detections: null counts / offset table / status pointer");
    CDETR_CHECK_ARG(d->wire_cap == 0 || d->wire, "cdetr_emit_detections: null wire-record pointer");
    CDETR_CHECK_ARG(d->eval_cap == 0 || (d->eval_boxes && d->eval_area && d->eval_score), "cdetr_emit_detections: null evaluation-record pointer");
    CDETR_CHECK_ARG((reinterpret_cast<uintptr_t>(d->wire) & 15) == 0, "cdetr_emit_detections: wire records must be 16-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(emit_count_kernel, dim3(d->B), dim3(256), 0, s, *d);
    hipLaunchKernelGGL(emit_kernel, dim3(d->B), dim3(EMIT_THREADS), 0, s, *d);
    return cdetr_launch_status("cdetr_emit_detections");
}
