// Stage-1 pseudo labels emitted on the device (main_stage1.py --device_labels): what stage1.write_pseudo_labels' host loop computes per
// annotated dot between the forward and pseudo_bbox_<split>.json, plus the evaluator's view of those boxes (A1/offline_coco_evaluator.py:
// the pseudo json's [cx, cy, w, h] as detections of score 1.0) and, when the batch carries its ground-truth boxes, the IoU of every
// pseudo box with the box its dot came from -- for a whole forwarded batch in one launch.
//
// cdetr_emit_pseudo_labels : per image b of the batch, its first counts[b] rows become wire records (row order; the fields of a
//   pseudo_bbox annotation), paired IoUs, and evaluation records (row order -- every score is 1.0 and COCOeval's sort is stable -- cut at
//   max_det; the float64 arrays cdetr_coco_match reads), appended to a device-resident store for the split.
//
// Everything must EQUAL the host path: the scalings are single fp32 multiplies followed by a truncation, the area is the fp32 product of
// the unrounded width and height, the IoU is coco_ap.box_iou_xywh's float64 expression.  A product contracted into an FMA with a later
// operation would differ, so contraction is switched off for this translation unit (as in coco_eval.hip and detections.hip).
//
// Placement is deterministic: every workgroup of image b adds up the counts of the batch's images before it and the store's running offset
// at `first` -- no atomic decides where a record lands (the only atomic is the OR into the status word).
#pragma clang fp contract(off)

#include "common.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int PL_ROWS = 256;              // rows of one image per workgroup = threads
constexpr int PL_WAVES = PL_ROWS / 64;
constexpr int PL_MAX_B = 65535;
constexpr int PL_MAX_ROWS = 1 << 20;      // padded rows per image
constexpr int PL_MAX_CAP = 1 << 30;       // records

// sum of `v` over the workgroup, the same value in every thread; `red` holds one value per wave and may be reused after the call
__device__ __forceinline__ long long block_sum(long long v, long long* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int w = 0; w < PL_WAVES; ++w) s += red[w];
    return s;
}

// coco_ap.box_iou_xywh, one pair: da, ga = w * h; union = (da + ga) - inter; 0 where the union is not positive
__device__ __forceinline__ double iou_xywh(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh) {
    const double da = dw * dh, ga = gw * gh;
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    const double inter = fmax(w, 0.0) * fmax(h, 0.0);
    const double uni = (da + ga) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

// grid (ceil(R / PL_ROWS), B): workgroup (x, b) owns rows x * PL_ROWS .. of image b
__global__ __launch_bounds__(PL_ROWS) void emit_pseudo_labels_kernel(cdetr_emit_pseudo_labels_desc p) {
    __shared__ long long red[PL_WAVES];
    const int b = blockIdx.y, n = p.first + b;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;        // one thread per image writes its offsets and status bits

    // a count outside 0 .. R describes no rows: it counts as 0 everywhere (and its own image reports it)
    auto rows_of = [&](int j) -> int {
        if (p.counts == nullptr) return p.R;
        const int c = p.counts[j];
        return (c < 0 || c > p.R) ? 0 : c;
    };
    long long sw = 0, se = 0;
    for (int j = threadIdx.x; j < b; j += PL_ROWS) {
        const int c = rows_of(j);
        sw += c;
        se += min(c, p.max_det);
    }
    sw = block_sum(sw, red);
    se = block_sum(se, red);
    const int start_w = p.row_off[p.first], start_e = p.eval_off[p.first];
    const int cnt = rows_of(b);
    const int ecnt = min(cnt, p.max_det);
    const bool count_ok = p.counts == nullptr || (p.counts[b] >= 0 && p.counts[b] <= p.R);
    const bool start_ok = start_w >= 0 && start_w <= p.row_cap && start_e >= 0 && start_e <= p.eval_cap;
    const long long w0 = start_w + sw, e0 = start_e + se;
    const bool fits_w = start_ok && w0 + cnt <= p.row_cap;
    const bool fits_e = start_ok && e0 + ecnt <= p.eval_cap;
    const bool fits = fits_w && fits_e;
    if (lead) {
        // offsets keep running while they stay inside the capacities (so that a later image that fits lands where it should); beyond
        // them they stop at the capacity, which every later image then fails against as well
        p.img_counts[n] = cnt;
        p.row_off[n + 1] = !start_ok ? start_w : (int)min(w0 + cnt, (long long)p.row_cap);
        p.eval_off[n + 1] = !start_ok ? start_e : (int)min(e0 + ecnt, (long long)p.eval_cap);
        const int bits = (!start_ok ? 4 : ((fits_w ? 0 : 1) | (fits_e ? 0 : 2))) | (count_ok ? 0 : 8);
        if (bits) atomicOr(p.status, bits);
    }
    if (!fits) return;                                  // uniform over the image's workgroups: nothing of it is written

    const int r = blockIdx.x * PL_ROWS + threadIdx.x;
    if (r >= cnt) return;
    const size_t src = (size_t)b * p.R + r;
    const float W = (float)p.orig_wh[2 * b], H = (float)p.orig_wh[2 * b + 1];
    // stage1.write_pseudo_labels' arithmetic: pts[:, 0] *= width ... in fp32 (one multiply each), int() of each; area = int(w * h) with the
    // fp32 product of the UNtruncated w and h
    const float2 pt = reinterpret_cast<const float2*>(p.points)[src];
    const float2 wh = reinterpret_cast<const float2*>(p.pred_wh)[src];
    const float xf = pt.x * W, yf = pt.y * H, wf = wh.x * W, hf = wh.y * H;
    const int cx = (int)xf, cy = (int)yf, w = (int)wf, h = (int)hf;
    const int area = (int)(wf * hf);
    const size_t dst = (size_t)(w0 + r);                // < row_cap: checked above
    int4* rec = reinterpret_cast<int4*>(p.wire + 8 * dst);
    rec[0] = make_int4(n, cx, cy, w);
    rec[1] = make_int4(h, area, 0, 0);

    // the evaluator's detection (A1/offline_coco_evaluator.py:134-143, COCO loadRes): [cx - w / 2, cy - h / 2, w, h] from the json's ints,
    // not truncated again; area = w * h
    const double bx = (double)cx - (double)w / 2.0, by = (double)cy - (double)h / 2.0, bw = (double)w, bh = (double)h;
    double iou = 0.0;
    if (p.gt_xywh != nullptr) {
        const double* g = p.gt_xywh + 4 * src;
        iou = iou_xywh(bx, by, bw, bh, g[0], g[1], g[2], g[3]);
    }
    p.pair_iou[dst] = iou;
    if (r < ecnt) {
        const size_t e = (size_t)(e0 + r);              // < eval_cap: checked above
        double* bo = p.eval_boxes + 4 * e;
        bo[0] = bx; bo[1] = by; bo[2] = bw; bo[3] = bh;
        p.eval_area[e] = (double)((long long)w * (long long)h);
        p.eval_score[e] = 1.0;
    }
}

}  // namespace

extern "C" int cdetr_emit_pseudo_labels(const cdetr_emit_pseudo_labels_desc* d, void* stream) {
    CDETR_CHECK_ARG(d != nullptr, "cdetr_emit_pseudo_labels: null descriptor");
    CDETR_CHECK_ARG(d->B > 0 && d->R > 0 && d->N > 0 && d->first >= 0 && d->max_det >= 0 && d->row_cap >= 0 && d->eval_cap >= 0,
                    "cdetr_emit_pseudo_labels: bad sizes B = %d, R = %d, N = %d, first = %d, max_det = %d, row_cap = %d, eval_cap = %d", d->B, d->R,
                    d->N, d->first, d->max_det, d->row_cap, d->eval_cap);
    if (d->R > PL_MAX_ROWS || d->B > PL_MAX_B) {
        cdetr_set_error("cdetr_emit_pseudo_labels: R = %d rows per image (limit %d) or B = %d images per call (limit %d) not supported", d->R,
                        PL_MAX_ROWS, d->B, PL_MAX_B);
        return CDETR_ERR_UNSUPPORTED;
    }
    CDETR_CHECK_ARG((int64_t)d->first + d->B <= d->N, "cdetr_emit_pseudo_labels: images %d .. %d do not fit a store of N = %d", d->first,
                    d->first + d->B - 1, d->N);
    CDETR_CHECK_ARG(d->row_cap <= PL_MAX_CAP && d->eval_cap <= PL_MAX_CAP, "cdetr_emit_pseudo_labels: capacities %d / %d exceed %d records",
                    d->row_cap, d->eval_cap, PL_MAX_CAP);
    CDETR_CHECK_ARG(d->points && d->pred_wh && d->orig_wh, "cdetr_emit_pseudo_labels: null input pointer");
    CDETR_CHECK_ARG(d->img_counts && d->row_off && d->eval_off && d->status, "cdetr_emit_pseudo_labels: null counts / offset table / status pointer");
    CDETR_CHECK_ARG(d->row_cap == 0 || (d->wire && d->pair_iou), "cdetr_emit_pseudo_labels: null wire-record / pair_iou pointer");
    CDETR_CHECK_ARG(d->eval_cap == 0 || (d->eval_boxes && d->eval_area && d->eval_score), "cdetr_emit_pseudo_labels: null evaluation-record pointer");
    CDETR_CHECK_ARG((reinterpret_cast<uintptr_t>(d->wire) & 15) == 0, "cdetr_emit_pseudo_labels: wire records must be 16-byte aligned");
    CDETR_CHECK_ARG(((reinterpret_cast<uintptr_t>(d->points) | reinterpret_cast<uintptr_t>(d->pred_wh)) & 7) == 0,
                    "cdetr_emit_pseudo_labels: points and pred_wh must be 8-byte aligned");
    hipLaunchKernelGGL(emit_pseudo_labels_kernel, dim3((d->R + PL_ROWS - 1) / PL_ROWS, d->B), dim3(PL_ROWS), 0,
                       reinterpret_cast<hipStream_t>(stream), *d);
    return cdetr_launch_status("cdetr_emit_pseudo_labels");
}
