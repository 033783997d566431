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
// of the images before it (records.h) -- no atomic decides where a record lands (the only atomic is the OR into the status word).
#pragma clang fp contract(off)

#include "records.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int EMIT_MAX_Q = 4096;          // keys of one image in LDS: 4096 x 8 B = 32 KiB
constexpr int EMIT_THREADS = 1024;
constexpr int EMIT_WAVES = EMIT_THREADS / 64;

// prob >= threshold, false for a NaN on either side (numpy's and torch's >=)
__device__ __forceinline__ bool kept(float p, float thr) { return p >= thr; }

// counts[first + b] = number of kept queries of image b
__global__ __launch_bounds__(256) void emit_count_kernel(cdetr_emit_detections_desc p) {
    __shared__ int red[4];
    const int b = blockIdx.x;
    const float* __restrict__ pr = p.prob + (size_t)b * p.Q;
    int n = 0;
    for (int q = threadIdx.x; q < p.Q; q += 256) n += kept(pr[q], p.threshold) ? 1 : 0;
    n = block_sum<4>(n, red);
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

// One workgroup = one image of the batch.
__global__ __launch_bounds__(EMIT_THREADS) void emit_kernel(cdetr_emit_detections_desc p) {
    __shared__ unsigned long long key[EMIT_MAX_Q];
    __shared__ int red[EMIT_WAVES];
    const int b = blockIdx.x, n = p.first + b;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    const auto at = place_records<EMIT_WAVES>([&](int j) { return p.counts[p.first + j]; }, b, p.Q, p.max_det, p.wire_off, p.eval_off, p.first,
                                              p.wire_cap, p.eval_cap, red);
    const int cnt = at.cnt, ecnt = at.ecnt;
    if (threadIdx.x == 0) {
        // the next offsets keep running past the capacities, UNclamped (cdetr_emit_pseudo_labels stops them at the capacity instead);
        // with the start inside the store they are < 2^30 + B * Q, inside int32
        p.wire_off[n + 1] = at.start_ok ? at.w0 + cnt : at.start_w;
        p.eval_off[n + 1] = at.start_ok ? at.e0 + ecnt : at.start_e;
    }
    if (!at.fits()) {                                   // uniform over the workgroup: nothing of this image is written
        if (threadIdx.x == 0) atomicOr(p.status, at.status_bits());
        return;
    }
    const size_t w0 = (size_t)at.w0, e0 = (size_t)at.e0;

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
            int4* dst = reinterpret_cast<int4*>(p.wire + 8 * (w0 + pos));
            dst[0] = make_int4(f.cx, f.cy, f.w, f.h);
            dst[1] = make_int4(f.area, f.px, f.py, __float_as_int(pq));
            key[pos] = sort_key(pq, q);
        }
        done += total;
    }
    if (ecnt == 0) return;

    // stable order by (score descending, query ascending): bitonic sort of the padded keys in LDS (records.h)
    sort_keys<EMIT_THREADS>(key, cnt);

    // evaluation records: coco_ap.reference_box on the wire integers ([int(cx - w/2), int(cy - h/2), w, h] = tdiv2(2 cx - w), ...: C++'s
    // integer division truncates toward zero like int()), area = w * h, score, as float64
    for (int r = threadIdx.x; r < ecnt; r += EMIT_THREADS) {
        const int q = (int)(unsigned)(key[r] & 0xffffffffull);
        const wire_fields f = wire_of(bx + 4 * (size_t)q, pt + 2 * (size_t)q, W, H);
        const long long x2 = 2ll * f.cx - f.w, y2 = 2ll * f.cy - f.h;
        write_eval_record(p.eval_boxes, p.eval_area, p.eval_score, e0 + r, (double)(x2 / 2), (double)(y2 / 2), f.w, f.h, (double)pr[q]);
    }
}

}  // namespace

extern "C" int cdetr_emit_detections(const cdetr_emit_detections_desc* d, void* stream) {
    CDETR_CHECK_ARG(d != nullptr, "cdetr_emit_detections: null descriptor");
    if (const int rc = check_record_store("cdetr_emit_detections", "Q", "queries", "wire_cap", "wire-record", d->B, d->Q, EMIT_MAX_Q, d->N, d->first,
                                          d->max_det, d->wire_cap, d->eval_cap, d->prob && d->boxes && d->points && d->orig_hw, d->counts, d->wire_off,
                                          d->eval_off, d->status, d->wire, d->wire != nullptr, d->eval_boxes, d->eval_area, d->eval_score))
        return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(emit_count_kernel, dim3(d->B), dim3(256), 0, s, *d);
    hipLaunchKernelGGL(emit_kernel, dim3(d->B), dim3(EMIT_THREADS), 0, s, *d);
    return cdetr_launch_status("cdetr_emit_detections");
}
