"""cdetr_render_boxes (csrc/render.hip) behind ops.render_boxes, render.render_images(device=) and infer.py --render_worst / --render_ids, against
the painter of tests/render_ref.py (pinned to hand-written pixels by tests/test_render_cpu.py).  Every comparison is == on uint8 arrays or on
file bytes."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import coco_ap_cases as cc
import eval_split as es
import render_ref as rr
from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops, render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW, CH = render.TILE_H, render.TILE_W, render.CHUNK


def same_images(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape, (k, g.dtype, g.shape, w.shape)
        bad = int((g != w).any(axis=2).sum())
        print(f"canvas {k} {w.shape}: {bad} pixels differ")
        assert bad == 0, k


def check(canvases, pack, matched, ignored, sel, dt_cnt=None, exs=None, style=rr.STYLE, dot=1):
    """One launch against the painter -> the painter's images."""
    want = rr.paint_pack(canvases, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=exs, style=style, dot=dot)
    same_images(render.render_images(canvases, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=exs, style=style, dot=dot, device=DEV), want)
    return want


def has(img, k):
    return bool((img == np.array(rr.STYLE[k][:3], dtype=np.uint8)).all(axis=2).any())


# ------------------------------------------------------------------------------------------------------------ 1. canvases around the tile
def test_canvases_around_the_tile_in_one_launch():
    rng = np.random.default_rng(11)
    sizes = [(1, 1), (TH + 1, TW + 1), (2 * TH - 1, 3 * TW + 1)]
    canvases, pack, matched, ignored, exs = rr.random_set(rng, sizes, 0, counts=[(3, 2, 1), (0, 0, 2), (40, 30, 3)])
    assert pack["dt_off"].tolist() == [0, 3, 3, 43] and pack["gt_off"].tolist() == [0, 2, 2, 32]       # the middle canvas: neither detection nor ground truth
    want = check(canvases, pack, matched, ignored, [0, 1, 2], exs=exs)
    assert has(want[2], rr.TP) and has(want[2], rr.FP) and has(want[2], rr.GT)


# ------------------------------------------------------------------------------------------------------------ 2. counts around the chunk
COUNTS = [(0, 0, 0), (0, 1, 0), (0, 0, 1),                                     # 0 and 1 primitives
          (CH // 2 - 28, 55, 0),                                               # CHUNK - 1 = 2 * 100 + 55 at CHUNK = 256
          (CH // 2, 0, 0), (CH // 2 - 28, 56, 0),                              # CHUNK: the list ends on the boundary
          (CH // 2, 1, 0), (CH // 2 - 28, 56, 1), (CH // 2, 0, 1),             # CHUNK + 1: the boundary between outlines | ground truths | exemplars
          (CH + 1, 1, 0),                                                      # 2 CHUNK + 3: the first boundary inside the dots, the second inside the outlines
          (CH - 56, CH // 2 - 28, 15),                                         # 2 CHUNK + 3: the first inside the outlines, the second inside the exemplars
          (CH // 2, CH, 3)]                                                    # 2 CHUNK + 3: both boundaries between layers


def test_primitive_counts_around_the_chunk():
    lens = sorted({2 * d + g + e for d, g, e in COUNTS})
    assert lens == [0, 1, CH - 1, CH, CH + 1, 2 * CH + 3]
    rng = np.random.default_rng(12)
    canvases, pack, matched, ignored, exs = rr.random_set(rng, [(3 * TH, 4 * TW)] * len(COUNTS), 0, counts=COUNTS, small=7.0, margin=4.0)
    want = check(canvases, pack, matched, ignored, list(range(len(COUNTS))), exs=exs)
    assert has(want[-2], rr.EXEMPLAR) and has(want[-1], rr.EXEMPLAR)            # the last chunk's primitives show
    # without dots the same sets are CHUNK / 2 ... long: other boundaries
    check(canvases, pack, matched, ignored, list(range(len(COUNTS))), exs=exs, dot=-1)
    # the one-detection list: its dot and its outline are two primitives
    one = rr.random_set(rng, [(TH, TW)], 0, counts=[(1, 0, 0)], small=7.0, margin=0.0)
    check(one[0], one[1], one[2], one[3], [0], exs=one[4], dot=-1)
    check(one[0], one[1], one[2], one[3], [0], exs=one[4], dot=0)


# ------------------------------------------------------------------------------------------------------------ 3. the pathological boxes
@pytest.mark.parametrize("case", rr.HAND_CASES, ids=[c[0] for c in rr.HAND_CASES])
def test_hand_written_pixels_on_the_device(case):
    canvases, pack, matched, ignored, sel, dt_cnt, exs, style, dot = rr.hand_inputs(case)
    got = render.render_images(canvases, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=exs, style=style, dot=dot, device=DEV)
    same_images(got, [rr.hand_expected(case[-1])])


# ------------------------------------------------------------------------------------------------------------ 4. sel, and what is written
def test_sel_names_an_image_twice_and_nothing_is_written_behind_out():
    rng = np.random.default_rng(14)
    sizes = [(TH + 3, 2 * TW + 5), (2 * TH + 1, TW - 3), (7, 9)]
    canvases, pack, matched, ignored, exs = rr.random_set(rng, sizes, 0, counts=[(30, 20, 2), (25, 10, 0), (5, 5, 1)])
    sel = [2, 0, 2, 1]                                                          # not the identity; pack image 2 on two canvases of different sizes
    shown = [canvases[2], canvases[0], rng.integers(0, 256, (TH + 9, TW + 2, 3), dtype=np.uint8), canvases[1]]
    ex = [exs[2], exs[0], exs[1], np.zeros((0, 4))]
    dt_cnt = [20, 100, 3]
    want = rr.paint_pack(shown, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=ex)
    with torch.cuda.device(DEV):
        kwargs, pix_off = render.device_inputs(shown, pack, matched, ignored, sel, dt_cnt, ex, render.DEFAULT_STYLE, 1, DEV)
        n = int(pix_off[-1])
        out = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        back = ops.render_boxes(**kwargs, out=out)
        assert back is out
        host = out.cpu().numpy()
    same_images([host[pix_off[k]:pix_off[k + 1]].reshape(shown[k].shape) for k in range(4)], want)
    assert (host[n:] == 0xAB).all() and len(host[n:]) == 64
    with pytest.raises(RuntimeError, match="cdetr_render_boxes.*rc=-3"):
        ops.render_boxes(**{**kwargs, "sel_host": [2, 0, 3, 1]})
    with pytest.raises(ValueError, match="sel"):
        render.render_images(shown, pack, matched, ignored, [2, 0, 3, 1], device=DEV)


# ------------------------------------------------------------------------------------------------------------ 5. the crowded image
def test_one_crowded_image():
    rng = np.random.default_rng(15)
    H, W, G, D = 384, 576, 3731, 1100
    xy = rng.uniform(0.0, [W - 8.0, H - 8.0], (G, 2))
    gts = np.concatenate([xy, rng.uniform(4.0, 14.0, (G, 2))], axis=1)
    pick = rng.integers(0, G, D)
    dts = gts[pick] + np.concatenate([rng.normal(0.0, 1.5, (D, 2)), rng.normal(0.0, 1.0, (D, 2))], axis=1)
    pack = rr.make_pack([(dts, gts)])
    canvas = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ex = [gts[:3].copy()]
    want = check([canvas], pack, rng.random(D) < 0.6, rng.random(D) < 0.05, [0], exs=ex)
    assert all(has(want[0], k) for k in (rr.TP, rr.FP, rr.IGNORED, rr.GT))
    check([canvas], pack, rng.random(D) < 0.6, rng.random(D) < 0.05, [0], dt_cnt=[900], exs=ex)


# ------------------------------------------------------------------------------------------------------------ 6. flags where they lie
def test_flags_where_the_matching_left_them():
    gts, dts = cc.float_family()
    pack = ca.pack_images(gts, dts)
    matching = ca.Matching.launch(pack, DEV)
    keep = [matching.matched, matching.det_ignored, matching.npig]
    assert all(k.is_cuda for k in keep) and keep[0].shape == keep[1].shape == (4, 10, len(pack["dt_score"])) and matching.device == keep[0].device
    rng = np.random.default_rng(16)
    B = len(pack["image_ids"])
    canvases = [rng.integers(0, 256, (300 + 17 * k, 420 - 31 * k, 3), dtype=np.uint8) for k in range(B)]
    _, matched, ignored, _ = cc.host_flags(gts, dts, "all")
    want = rr.paint_pack(canvases, pack, matched[0], ignored[0], list(range(B)))
    assert sum(has(w, rr.TP) for w in want) >= 2 and sum(has(w, rr.FP) for w in want) >= 2
    ex = [np.zeros((0, 4))] * B
    with torch.cuda.device(DEV):
        kwargs, pix_off = render.device_inputs(canvases, pack, *matching.row50(), list(range(B)), None, ex, render.DEFAULT_STYLE, 1, DEV)
        assert kwargs["matched50"].data_ptr() == keep[0].data_ptr() and kwargs["ignored50"].data_ptr() == keep[1].data_ptr()      # no copy of the flags
        assert keep[0].data_ptr() == keep[0]._base.data_ptr() and keep[1]._base.data_ptr() == keep[0].data_ptr()                  # the launch's one buffer
        host = ops.render_boxes(**kwargs).cpu().numpy()
    same_images([host[pix_off[k]:pix_off[k + 1]].reshape(canvases[k].shape) for k in range(B)], want)


# ------------------------------------------------------------------------------------------------------------ 7. the routes of infer.py
CANDIDATE_THRESHOLDS = (0.5, 0.45, 0.4, 0.35, 0.3, 0.25, 0.2, 0.15, 0.1, 0.05, 0.02)


def _pick_threshold(prob, boxes, sizes, gt_by):
    """The first candidate threshold at which some image has a true and a false positive at IoU 0.5 among the detections infer.py would write
    (its arithmetic: fp32 scaling, int(), reference_box), matched by coco_ap's host matcher."""
    T = len(ca.IOU_THRS)
    for thr in CANDIDATE_THRESHOLDS:
        found = []
        for k, (p, bx, (h, w)) in enumerate(zip(prob, boxes, sizes)):
            keep = p >= np.float32(thr)
            b = bx[keep].astype(np.float32).copy()
            b[:, 0] *= w; b[:, 1] *= h; b[:, 2] *= w; b[:, 3] *= h
            dts = []
            for s, (cx, cy, bw, bh) in zip(p[keep].tolist(), b):
                box = ca.reference_box([int(cx), int(cy), int(bw), int(bh)])
                dts.append({"bbox": box, "score": float(s), "area": float(box[2] * box[3])})
            _, m, ig, _ = ca._evaluate_image(dts, gt_by.get(k + 1, []), ca.AREA_RNG["all"], ca.MAX_DETS)
            m, ig = m.reshape(T, -1)[0], ig.reshape(T, -1)[0]
            found.append((int((m & ~ig).sum()), int((~m & ~ig).sum())))
        print("threshold", thr, "tp / fp per image", found)
        if any(tp and fp for tp, fp in found):
            return thr
    raise AssertionError("no candidate threshold gives an image with a true and a false positive")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """infer.py on the five-image split of tests/eval_split.py with the seeded model of tests/test_image_report_gpu.py (class bias shifted into
    the gap under the three highest images): every run the comparisons below read, each once.

    The three routes are compared at ONE --eval_batch_size each time, 1 and 2.  A forward of two images does not give the bits of two forwards
    of one (tests/test_image_report_gpu.py compares its batches of two among themselves for the same reason): measured on this split, the
    host route at batch 1 and the store route at batch 2 wrote the same five PNGs byte for byte, while image 1's own AP in index.json's `row`
    was 0.028241079141471184 against 0.028336166950028326 (scores that differ in the last bits change places in the evaluation order)."""
    import infer as infer_mod
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import default_args, get_args_parser
    from counting_detr_amd.misc import NestedTensor
    from oracle.weights import seeded_state_dict
    root = tmp_path_factory.mktemp("render")
    args = default_args()
    args.data_path, args.scale_factor, args.split, args.num_workers, args.device = es.write_split(root / "ds"), 32, "val", 0, DEV
    model, _, _ = build_model(args)
    model.load_state_dict(seeded_state_dict(), strict=True)
    model.to(DEV)
    model.eval()
    ds = data.build_test_dataset(args, "val")
    with torch.no_grad():
        outs = [model(NestedTensor(b["image"].to(DEV), b["mask"].to(DEV)), rects=b["ex_rects"].to(DEV))[0] for b in (data.collate([ds[i]]) for i in range(len(ds)))]
        logit = torch.stack([o["pred_logits"][0, :, 0] for o in outs]).double().cpu()
        lo, hi = logit.min(1).values, logit.max(1).values
        order = torch.argsort(lo)
        shift = 0.5 * (float(hi[order[1]]) + float(lo[order[2]]))
        for ce in {id(m): m for m in model.transformer.cls_embed}.values():
            ce.bias[0] -= shift
        outs = [model(NestedTensor(b["image"].to(DEV), b["mask"].to(DEV)), rects=b["ex_rects"].to(DEV))[0] for b in (data.collate([ds[i]]) for i in range(len(ds)))]
    prob = [o["pred_logits"][0, :, 0].sigmoid().float().cpu().numpy() for o in outs]
    boxes = [o["pred_boxes"][0].float().cpu().numpy() for o in outs]
    gt_by = ca.gt_from_json(os.path.join(args.data_path, "instances_val.json"), [1, 2, 3, 4, 5])
    threshold = _pick_threshold(prob, boxes, [(im[2], im[1]) for im in es.IMAGES], gt_by)
    ckpt = root / "shifted.pth"
    torch.save({"model": model.state_dict()}, ckpt)
    common = ["-dp", args.data_path, "--split", "val", "--resume", str(ckpt), "--no_aux_loss", "--num_query_pattern", "1", "--num_workers", "0",
              "--device", DEV, "--threshold", str(threshold), "--image_report"]
    rend = ["--render_worst", "2", "--render_ids", "3,5"]
    two = ["--eval_batch_size", "2"]
    store = ["--device_detections"]
    out = {"root": root, "threshold": threshold}
    real = ops.render_boxes
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    for name, extra in (("host", ["--ap_on_host", *rend]), ("match", rend), ("store", [*store, *rend]),
                        ("host2", ["--ap_on_host", *two, *rend]), ("match2", [*two, *rend]), ("store2", [*store, *two, *rend]),
                        ("store2_sweep", [*store, *two, *rend, "--sweep_thresholds", f"{threshold / 2},{threshold},0.9"]),
                        ("host_plain", ["--ap_on_host"]), ("match_plain", []), ("store2_plain", [*store, *two])):
        buf = io.StringIO()
        del calls[:]
        try:
            ops.render_boxes = counted
            with contextlib.redirect_stdout(buf):
                infer_mod.main(get_args_parser().parse_args(common + ["-o", str(root / name)] + extra))
        finally:
            ops.render_boxes = real
        out[name] = json.loads(buf.getvalue().strip().splitlines()[-1])
        out[name + "_launches"] = len(calls)
    return out


def _files(runs, name):
    d = runs["root"] / name / "render_val"
    return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_the_overlays_show_true_and_false_positives(runs):
    from PIL import Image
    files = _files(runs, "host")
    index = json.loads(files["index.json"])
    print("threshold", runs["threshold"], [(e["image_id"], e["reasons"], e["row"]["tp50"], e["row"]["fp50"]) for e in index["images"]])
    assert list(index) == ["split", "threshold", "style", "dot", "images"] and index["threshold"] == runs["threshold"] and index["style"] == rr.STYLE
    ids = [e["image_id"] for e in index["images"]]
    assert 3 in ids and 5 in ids and 2 <= len(ids) <= 5 and sorted(files) == sorted(["index.json"] + [f"{i}.png" for i in ids])
    both = marks = 0
    for e in index["images"]:
        img = np.asarray(Image.open(runs["root"] / "host" / "render_val" / e["png"]))
        w, h = [(im[1], im[2]) for im in es.IMAGES if im[0] == e["file_name"]][0]
        assert img.shape == (h, w, 3)
        both += has(img, rr.TP) and has(img, rr.FP)
        marks += has(img, rr.GT) or has(img, rr.EXEMPLAR)
    assert both >= 1 and marks >= 1                                                            # not a comparison of empty overlays


@pytest.mark.parametrize("tag", ["", "2"], ids=["eval_batch_size_1", "eval_batch_size_2"])
def test_three_routes_write_the_same_bytes(runs, tag):
    host, match, store = _files(runs, "host" + tag), _files(runs, "match" + tag), _files(runs, "store" + tag)
    assert list(host) == list(match) == list(store) and len(host) >= 3
    for f in host:
        assert host[f] == match[f], f
        assert host[f] == store[f], f
    assert (runs[f"host{tag}_launches"], runs[f"match{tag}_launches"], runs[f"store{tag}_launches"]) == (0, 1, 1)


def test_batches_of_two_draw_the_same_images(runs):
    one, two = json.loads(_files(runs, "store")["index.json"]), json.loads(_files(runs, "store2")["index.json"])
    assert [(e["image_id"], e["reasons"], e["file_name"]) for e in one["images"]] == [(e["image_id"], e["reasons"], e["file_name"]) for e in two["images"]]
    assert {k: v for k, v in one.items() if k != "images"} == {k: v for k, v in two.items() if k != "images"}


def test_with_a_sweep_the_pngs_are_unchanged(runs):
    store, sweep = _files(runs, "store2"), _files(runs, "store2_sweep")
    assert list(store) == list(sweep) and all(store[f] == sweep[f] for f in store) and runs["store2_sweep_launches"] == 1
    sw = json.loads(open(runs["root"] / "store2_sweep" / "threshold_sweep_val.json").read())
    kept = [sum(r["count_pred"] for r in json.loads(open(runs["root"] / n / "image_report_val.json").read())["rows"]) for n in ("store2", "store2_sweep")]
    print("sweep thresholds", sw["thresholds"], "kept at the run's threshold", kept)
    assert len(sw["rows"]) == 3 and kept[0] == kept[1]                          # the store of the sweep was emitted at half the run's threshold


def test_the_runs_other_outputs_do_not_change(runs):
    eq = lambda a, b: a == b or (a != a and b != b)                             # noqa: E731
    for name in ("host", "match", "store2"):
        a, b = runs["root"] / name, runs["root"] / (name + "_plain")
        assert not os.path.exists(b / "render_val") and runs[name + "_plain_launches"] == 0
        for f in ("predictions_val.json", "image_report_val.json", "results_val.txt"):
            assert open(a / f, "rb").read() == open(b / f, "rb").read(), (name, f)
        assert list(runs[name]) == list(runs[name + "_plain"]) and all(eq(runs[name][k], runs[name + "_plain"][k]) for k in runs[name]), name
        assert sorted(os.listdir(a)) == sorted(os.listdir(b) + ["render_val"])
