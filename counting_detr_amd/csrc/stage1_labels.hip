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
// at `first` (records.h) -- no atomic decides where a record lands (the only atomic is the OR into the status word).
#pragma clang fp contract(off)

#include "records.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int PL_ROWS = 256;              // rows of one image per workgroup = threads
constexpr int PL_WAVES = PL_ROWS / 64;
constexpr int PL_MAX_ROWS = 1 << 20;      // padded rows per image

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
    const auto at = place_records<PL_WAVES>(rows_of, b, p.R, p.max_det, p.row_off, p.eval_off, p.first, p.row_cap, p.eval_cap, red);
    const int cnt = at.cnt, ecnt = at.ecnt;
    const long long w0 = at.w0, e0 = at.e0;
    const bool count_ok = p.counts == nullptr || (p.counts[b] >= 0 && p.counts[b] <= p.R);
    if (lead) {
        // offsets keep running while they stay inside the capacities (so that a later image that fits lands where it should); beyond
        // them they stop AT the capacity, which every later image then fails against as well (cdetr_emit_detections lets them run on, unclamped)
        p.img_counts[n] = cnt;
        p.row_off[n + 1] = !at.start_ok ? at.start_w : (int)min(w0 + cnt, (long long)p.row_cap);
        p.eval_off[n + 1] = !at.start_ok ? at.start_e : (int)min(e0 + ecnt, (long long)p.eval_cap);
        const int bits = at.status_bits() | (count_ok ? 0 : 8);
        if (bits) atomicOr(p.status, bits);
    }
    if (!at.fits()) return;                             // uniform over the image's workgroups: nothing of it is written

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
    if (r < ecnt) write_eval_record(p.eval_boxes, p.eval_area, p.eval_score, (size_t)(e0 + r), bx, by, w, h, 1.0);      // < eval_cap: checked above
}

}  // namespace

extern "C" int cdetr_emit_pseudo_labels(const cdetr_emit_pseudo_labels_desc* d, void* stream) {
    CDETR_CHECK_ARG(d != nullptr, "cdetr_emit_pseudo_labels: null descriptor");
    if (const int rc = check_record_store("cdetr_emit_pseudo_labels", "R", "rows per image", "row_cap", "wire-record / pair_iou", d->B, d->R, PL_MAX_ROWS,
                                          d->N, d->first, d->max_det, d->row_cap, d->eval_cap, d->points && d->pred_wh && d->orig_wh, d->img_counts,
                                          d->row_off, d->eval_off, d->status, d->wire, d->wire && d->pair_iou, d->eval_boxes, d->eval_area,
                                          d->eval_score))
        return rc;
    CDETR_CHECK_ARG(((reinterpret_cast<uintptr_t>(d->points) | reinterpret_cast<uintptr_t>(d->pred_wh)) & 7) == 0,
                    "cdetr_emit_pseudo_labels: points and pred_wh must be 8-byte aligned");
    hipLaunchKernelGGL(emit_pseudo_labels_kernel, dim3((d->R + PL_ROWS - 1) / PL_ROWS, d->B), dim3(PL_ROWS), 0,
                       reinterpret_cast<hipStream_t>(stream), *d);
    return cdetr_launch_status("cdetr_emit_pseudo_labels");
}
