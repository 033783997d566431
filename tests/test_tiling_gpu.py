"""cdetr_tile_images, cdetr_exemplar_group_fwd and cdetr_tile_stitch (csrc/tiling.hip) behind ops against the host rule
(counting_detr_amd/tiling.py), the capability count_pred > Q through ops.DetectionStore, then --tiles end to end: infer.py's host and device
passes on a four-image tree with the seeded model of tests/test_threshold_sweep_gpu.py.  Every comparison is exact: equal NaN masks, the other
entries bit for bit, equal bytes, == metrics."""
import json
import os

import numpy as np
import pytest
import torch

from counting_detr_amd import ops, tiling

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
COUNT_KEYS = ("MAE", "RMSE", "NAE", "SRE")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(a, b):
    """fp32 arrays: equal NaN masks, every other entry bit for bit."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ------------------------------------------------------------------------------------------------------------------ cdetr_tile_images
def _cut(image, plan, records=None):
    """One launch into sentinel-filled outputs -> (tiles, mask) on the host."""
    tiles = torch.full((plan.T, 3, plan.Hm, plan.Wm), -7.0, dtype=torch.float32, device=DEV)
    mask = torch.zeros((plan.T, plan.Hm, plan.Wm), dtype=torch.uint8, device=DEV).fill_(3).view(torch.bool)
    got = ops.tile_images(T(image), T(plan.records if records is None else records), plan.Hm, plan.Wm, tiles=tiles, mask=mask)
    assert got[0] is tiles and got[1] is mask
    return tiles.cpu().numpy(), mask.view(torch.uint8).cpu().numpy()


@pytest.mark.parametrize("H,W,R,C,M,S", [(96, 160, 2, 2, 32, 1), (96, 160, 2, 2, 32, 2), (64, 64, 2, 2, 0, 1), (70, 100, 1, 2, 32, 2), (70, 100, 1, 2, 7, 2),
                                         (70, 100, 1, 2, 7, 1), (96, 1100, 1, 2, 32, 1)])
def test_tile_images_equals_the_rule(H, W, R, C, M, S):
    image = np.random.default_rng(H + W + M + S).standard_normal((3, H, W)).astype(np.float32)
    plan = tiling.Plan(H, W, R, C, M, S)
    want_t, want_m = tiling.tile_images(image, plan)
    got_t, got_m = _cut(image, plan)
    print("tiles", plan.boxes, "padded", plan.Hm, plan.Wm)
    assert plan.T == R * C and np.array_equal(got_m, want_m.astype(np.uint8))                  # bytes 0 / 1, the sentinel 3 gone
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
    if (H, W) == (70, 100):
        assert want_m.any() and not want_m.all() and len({b[2] - b[0] for b in plan.boxes}) == 2      # ragged tiles: padding on the narrow one


def test_a_record_out_of_range_gives_an_all_padding_tile():
    H, W = 64, 128
    image = np.random.default_rng(1).standard_normal((3, H, W)).astype(np.float32)
    plan = tiling.Plan(H, W, 2, 2, 0, 1)
    good = plan.records.copy()
    assert good.tolist() == [[0, 0, 64, 32, 1], [64, 0, 64, 32, 1], [0, 32, 64, 32, 1], [64, 32, 64, 32, 1]] and (plan.Hm, plan.Wm) == (32, 64)
    # right of the image, reaching over its right / lower edge, negative, a scale that does not exist, empty, wider than Wm, too large once scaled
    bad = np.array([[128, 0, 64, 32, 1], [100, 0, 64, 32, 1], [0, 40, 64, 32, 1], [-1, 0, 64, 32, 1], [0, 0, 64, 32, 3], [0, 0, 0, 32, 1], [0, 0, 65, 32, 1],
                    [0, 0, 64, 32, 2], [0, 2 ** 31 - 1, 64, 32, 1], [2 ** 31 - 1, 0, 2 ** 31 - 1, 32, 1]], dtype=np.int32)
    for rec in bad:
        records = good.copy()
        records[1] = rec
        got_t, got_m = _cut(image, plan, records)
        want_t, want_m = tiling.tile_images(image, plan)
        want_t[1], want_m[1] = 0.0, True
        assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)) and np.array_equal(got_m, want_m.astype(np.uint8)), rec


# ------------------------------------------------------------------------------------------------------------------ cdetr_exemplar_group_fwd
def _group_case(B, seed):
    """Map 3 x 5, C = 2048, K = 3: tile 0 with two exemplars sharing a cell and one absent row, tile 1 with every row absent, tiles 2 and 3 with one
    exemplar each and smaller extents; tiles 4 .. 7 (B = 8) with no exemplar at all."""
    rng = np.random.default_rng(seed)
    h, w, C, K = 3, 5, 2048, 3
    x = rng.standard_normal((B, h * w, C)).astype(np.float32)
    rects = np.full((B, K, 4), -1.0, dtype=np.float32)
    rects[0, 0], rects[0, 2] = (0.11, 0.13, 0.31, 0.29), (0.13, 0.12, 0.29, 0.32)
    rects[2, 1], rects[3, 0] = (0.70, 0.52, 0.93, 0.91), (0.41, 0.05, 0.58, 0.27)
    extent = np.tile(np.array([[3, 5]], dtype=np.float32), (B, 1))
    extent[2], extent[3] = (2, 4), (3, 4)
    return x, rects, extent, h, w


@pytest.mark.parametrize("B,G", [(4, 4), (8, 4), (4, 2), (4, 1)])
def test_exemplar_group_fwd_equals_the_rule(B, G):
    x, rects, extent, h, w = _group_case(B, 10 * B + G)
    pf, idx = ops.exemplar_group_fwd(T(x).view(B, h, w, -1), T(rects), T(extent), G)
    want_pf, want_idx = tiling.group_feature(x, rects, extent, h, w, G)
    print("idx", idx.cpu().tolist())
    assert np.array_equal(idx.cpu().numpy(), want_idx) and same(pf.cpu().numpy(), want_pf)
    assert want_idx[0, 0] == want_idx[0, 2] >= 0 and (want_idx[1] == -1).all()                 # a shared cell, a tile without exemplars
    pf = pf.cpu().numpy()
    for g in range(B // G):
        assert all(np.array_equal(pf[g * G].view(np.uint32), pf[b].view(np.uint32)) for b in range(g * G, (g + 1) * G))
    if (B, G) == (8, 4):
        assert (pf[4:] == 0).all() and np.abs(pf[:4]).max() > 0                                 # a group with nothing present
    if G == 4:
        assert not np.array_equal(pf[0], tiling.group_feature(x, rects, extent, h, w, 1)[0][0])  # pooled over the group, not the tile's own


def test_group_of_one_equals_cdetr_exemplar_fwd():
    rng = np.random.default_rng(3)
    B, h, w, C, K = 6, 3, 5, 2048, 3
    x = rng.standard_normal((B, h * w, C)).astype(np.float32)
    c, s = rng.uniform(0.0, 1.0, (B, K, 2)), rng.uniform(0.01, 0.3, (B, K, 2))
    rects = np.concatenate([c - s / 2, c + s / 2], 2).astype(np.float32)
    rects[1, 1], rects[4] = -1.0, -1.0
    extent = np.stack([rng.integers(1, h + 1, B), rng.integers(1, w + 1, B)], 1).astype(np.float32)
    xd, rd, ed = T(x).view(B, h, w, C), T(rects), T(extent)
    pf1, idx1, _ = ops.exemplar_fwd_raw(xd, rd, ed, True)
    pf, idx = ops.exemplar_group_fwd(xd, rd, ed, 1)
    assert torch.equal(idx, idx1) and np.array_equal(pf.cpu().numpy().view(np.uint32), pf1.cpu().numpy().view(np.uint32))
    want_pf, want_idx = tiling.group_feature(x, rects, extent, h, w, 1)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and same(pf.cpu().numpy(), want_pf)
    pf_raw, idx_raw, inv = ops.exemplar_fwd_raw(xd, rd, ed, True, group=3)                      # the argument the model's two paths go through
    assert inv is None and same(pf_raw.cpu().numpy(), tiling.group_feature(x, rects, extent, h, w, 3)[0])
    with pytest.raises(RuntimeError, match="forward only"):                                     # the model asks once for both of its paths
        ops.forward_only_group(3)
    with torch.no_grad():
        assert ops.forward_only_group(3) == 3
    assert ops.forward_only_group(1) == 1
    torch.cuda.synchronize()


def test_a_grouped_forward_with_gradients_enabled_is_an_error():
    from counting_detr_amd import build_model
    from counting_detr_amd.args import default_args
    model, _, _ = build_model(default_args())
    model.to(DEV).eval()
    images, rects = torch.zeros((2, 3, 64, 64), device=DEV), torch.full((2, 3, 4), -1.0, device=DEV)
    with pytest.raises(RuntimeError, match="forward only"):
        model(images, rects=rects, group=2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ cdetr_tile_stitch
PLANS = {1: (32, 32), 2: (32, 256), 4: (128, 256)}            # image sizes at which a 2x2 request has 1, 2 and 4 tiles (R * C = 4 slots)


def _stitch_inputs(plan, Q, seed):
    """Tile outputs with centres spread over each tile, some placed exactly on a core bound of the tile (in tile coordinates that map onto it
    exactly where the coefficients are exact), NaN and +-inf entries."""
    rng = np.random.default_rng(seed)
    Tn = plan.T
    prob = rng.uniform(0, 1, (Tn, Q)).astype(np.float32)
    boxes, points = rng.uniform(-0.1, 1.1, (Tn, Q, 4)).astype(np.float32), rng.uniform(0, 1, (Tn, Q, 2)).astype(np.float32)
    for t in range(Tn):
        (x0, y0, x1, y1), (kx0, ky0, kx1, ky1) = plan.boxes[t], plan.cores[t]
        for q, (bx, by) in enumerate(((kx0, ky0), (kx1, ky1), (kx0, ky1), (kx1, ky0))):
            if q < Q:
                boxes[t, q, 0], boxes[t, q, 1] = np.float32((bx - x0) / (x1 - x0)), np.float32((by - y0) / (y1 - y0))
    special = [np.nan, np.inf, -np.inf, -0.0]
    for k, v in enumerate(special):
        if Q > 8 + 3 * k + 2:
            prob[k % Tn, 8 + 3 * k], boxes[(k + 1) % Tn, 9 + 3 * k, k % 4], points[k % Tn, 10 + 3 * k, k % 2] = v, v, v
    return prob, boxes, points


def _stitch(prob, boxes, points, plan):
    Q = prob.shape[1]
    Qv = plan.slots * Q
    out = (torch.full((1, Qv), -3.0, device=DEV), torch.full((1, Qv, 4), -3.0, device=DEV), torch.full((1, Qv, 2), -3.0, device=DEV))
    got = ops.tile_stitch(T(prob), T(boxes), T(points), T(plan.coef), plan.slots, plan.H, plan.W, out=out)
    assert all(g is o for g, o in zip(got, out))
    return tuple(o[0].cpu().numpy() for o in out)


@pytest.mark.parametrize("M", [32, 0])
@pytest.mark.parametrize("Tn", [1, 2, 4])
@pytest.mark.parametrize("Q", [1, 64, 65, 900])
def test_tile_stitch_equals_the_rule(Q, Tn, M):
    plan = tiling.Plan(*PLANS[Tn], 2, 2, M, 1)
    assert plan.T == Tn and plan.slots == 4
    prob, boxes, points = _stitch_inputs(plan, Q, 1000 * Q + 10 * Tn + M)
    got, want = _stitch(prob, boxes, points, plan), tiling.stitch(prob, boxes, points, plan)
    kept = int((~np.isnan(want[0])).sum())
    print("Q", Q, "tiles", Tn, "kept", kept, "of", Tn * Q)
    assert all(same(g, w) for g, w in zip(got, want))
    assert np.isnan(got[0][Tn * Q:]).all() and (got[1][Tn * Q:] == 0).all() and (got[2][Tn * Q:] == 0).all()      # slots without a tile
    if Tn == 1:                                                                                 # one whole-image tile: the identity on every bit
        assert all(np.array_equal(g[:Q].view(np.uint32), a[0].view(np.uint32)) for g, a in zip(got, (prob, boxes, points)))
    elif Q >= 64:
        assert 0 < kept < Tn * Q
    if M == 0 and Tn == 4:                 # tiles = cores, a = 1 / 2 exactly: a centre on the low bound is the tile's own, one on the high bound is not
        p = got[0].reshape(4, Q)
        for t in range(4):
            low_x, low_y = plan.cores[t][0] == 0, plan.cores[t][1] == 0
            high_x, high_y = plan.cores[t][2] == plan.W, plan.cores[t][3] == plan.H
            assert not np.isnan(p[t, 0])                                                        # query 0: (lo, lo)
            if Q > 1:
                assert np.isnan(p[t, 1]) == (not (high_x and high_y))                          # query 1: (hi, hi), kept only where hi is the image's end


def test_tile_stitch_arguments_are_checked_before_any_launch():
    plan = tiling.Plan(128, 256, 2, 2, 32, 1)
    prob, boxes, points = (T(a) for a in _stitch_inputs(plan, 1025, 0))
    with pytest.raises(RuntimeError, match="cdetr_tile_stitch.*4100"):
        ops.tile_stitch(prob, boxes, points, T(plan.coef), 4, 128, 256)
    with pytest.raises(RuntimeError, match="tile_stitch"):
        ops.tile_stitch(prob, boxes, points, T(plan.coef[:3]), 4, 128, 256)
    with pytest.raises(RuntimeError, match="tile_stitch"):
        ops.tile_stitch(prob.double(), boxes, points, T(plan.coef), 4, 128, 256)
    with pytest.raises(RuntimeError, match="cdetr_tile_stitch"):
        ops.tile_stitch(prob[:, :8].contiguous(), boxes[:, :8].contiguous(), points[:, :8].contiguous(), T(plan.coef), 3, 128, 256)      # slots < T
    torch.cuda.synchronize()


def test_four_tiles_count_past_the_query_cap():
    """Stub outputs: every query of four tiles above the threshold and centred in its own tile's core -> 4 Q detections of ONE image."""
    Q = 900
    plan = tiling.Plan(128, 192, 2, 2, 32, 1)
    rng = np.random.default_rng(8)
    prob = rng.uniform(0.6, 0.99, (4, Q)).astype(np.float32)
    boxes, points = np.zeros((4, Q, 4), dtype=np.float32), rng.uniform(0, 1, (4, Q, 2)).astype(np.float32)
    for t in range(4):
        (x0, y0, x1, y1), (kx0, ky0, kx1, ky1) = plan.boxes[t], plan.cores[t]
        boxes[t, :, 0] = (rng.uniform(kx0 + 1, kx1 - 1, Q) - x0) / (x1 - x0)
        boxes[t, :, 1] = (rng.uniform(ky0 + 1, ky1 - 1, Q) - y0) / (y1 - y0)
        boxes[t, :, 2:] = rng.uniform(0.02, 0.1, (Q, 2))
    p, b, r = ops.tile_stitch(T(prob), T(boxes), T(points), T(plan.coef), plan.slots, plan.H, plan.W)
    assert tuple(p.shape) == (1, 4 * Q) and same(p[0].cpu().numpy(), prob.reshape(-1))
    store = ops.DetectionStore(1, 4 * Q, DEV, threshold=0.5)
    store.emit(p, b, r, T(np.array([[140, 200]], dtype=np.int32)))
    host = store.finish()
    assert host["counts"].tolist() == [4 * Q] and 4 * Q > Q and host["wire"].shape[0] == 4 * Q
    want = tiling.stitch(prob, boxes, points, plan)
    assert same(b[0].cpu().numpy(), want[1]) and same(r[0].cpu().numpy(), want[2])
    assert np.array_equal(host["wire"][:, 0], (want[1][:, 0] * np.float32(200)).astype(np.int32))       # whole-image pixels


# ------------------------------------------------------------------------------------------------------------------ end to end
# (file, width, height, objects, exemplar side): resized to 192 x 128 and 128 x 192, so a 2x2 grid has four real tiles of 96 x 128 / 128 x 96; the
# first and the last image have small exemplars (mean sqrt(w h) about 9 resized pixels), the two in the middle large ones (about 30)
IMAGES = [("s0.png", 200, 140, 12, 9.0), ("l0.png", 141, 203, 7, 31.0), ("l1.png", 199, 139, 9, 30.0), ("s1.png", 140, 200, 11, 10.0)]
BELOW = 18.0


def write_tree(root, seed=4):
    """A four-image FSC-147 validation split of seeded-noise PNGs under `root`, in the manner of tests/eval_split.py -> its data_path."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "images_384_VarV2"))
    anno, images, annotations = {}, [], []
    for k, (name, w, h, n, side) in enumerate(IMAGES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "images_384_VarV2", name))
        wh = rng.uniform(side * 0.9, side * 1.1, (n, 2))
        xy = rng.uniform(1.0, [w - 1.2 * side - 1, h - 1.2 * side - 1], (n, 2))
        images.append({"id": k + 1, "file_name": name, "width": w, "height": h})
        for (x, y), (bw, bh) in zip(xy.tolist(), wh.tolist()):
            annotations.append({"id": len(annotations) + 1, "image_id": k + 1, "bbox": [x, y, bw, bh], "category_id": 1, "area": bw * bh, "iscrowd": 0})
        ex = [[[x, y], [x, y + bh], [x + bw, y + bh], [x + bw, y]] for (x, y), (bw, bh) in zip(xy[:3].tolist(), wh[:3].tolist())]
        anno[name] = {"box_examples_coordinates": ex, "points": (xy + wh / 2).tolist(), "H": h, "W": w}
    names = [im[0] for im in IMAGES]
    for fn, obj in (("annotation_FSC147_384.json", anno), ("Train_Test_Val_FSC_147.json", {"train": [], "val": names, "test": []}),
                    ("instances_val.json", {"images": images, "annotations": annotations, "categories": [{"id": 1, "name": "fg"}]})):
        with open(os.path.join(root, fn), "w") as f:
            json.dump(obj, f)
    return str(root)


def _same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


RUNS = {"plain": [], "t1x1": ["--tiles", "1x1"], "t2x2": ["--tiles", "2x2"], "below": ["--tiles", "2x2", "--tile_below", str(BELOW)],
        "full": ["--tiles", "2x2", "--tile_scale", "2", "--nms_iou", "0.5", "--sweep_thresholds", "0.3:0.7:3", "--image_report"]}


@pytest.fixture(scope="module")
def passes(tmp_path_factory):
    """Every pass the end-to-end tests read, run once through infer.evaluate_split from a parsed command line, each on the host loop and with
    --device_detections, all on ONE engine of the seeded model (class bias shifted to the first image's median logit)."""
    import infer as infer_mod
    from counting_detr_amd import build_model
    from counting_detr_amd.args import default_args, get_args_parser
    from counting_detr_amd.engine import InferenceEngine
    from counting_detr_amd.misc import NestedTensor
    from oracle.weights import seeded_state_dict
    root = tmp_path_factory.mktemp("tiling_tree")
    data_path = write_tree(root / "data")
    model, criterion, _ = build_model(default_args())
    model.load_state_dict(seeded_state_dict(), strict=True)
    model.to(DEV); criterion.to(DEV)
    model.eval()
    out = {"root": root, "stats": {}}

    def parse(name, loop):
        return get_args_parser().parse_args(["-dp", data_path, "--split", "val", "-o", str(root / f"{name}_{loop}"), "--device", DEV, "--scale_factor", "32",
                                             "--num_workers", "0"] + (["--device_detections"] if loop == "device" else []) + RUNS[name])
    dl, _ = infer_mod.eval_loader(parse("plain", "host"), torch.device(DEV))
    first = next(iter(dl))
    with torch.no_grad():
        logit = model(NestedTensor(first["image"].to(DEV), first["mask"].to(DEV)), rects=first["ex_rects"].to(DEV))[0]["pred_logits"][0, :, 0]
        for ce in {id(m): m for m in model.transformer.cls_embed}.values():
            ce.bias[0] -= logit.median()
    engine = InferenceEngine(model, 0.5, device=DEV)
    for name in RUNS:
        for loop in ("host", "device"):
            args = parse(name, loop)
            os.makedirs(args.output_dir)
            dl, per_image = infer_mod.eval_loader(args, torch.device(DEV))
            before = dict(engine.stats)
            out[name, loop] = infer_mod.evaluate_split(model, criterion, dl, per_image, torch.device(DEV), args, engine=engine)
            out["stats"][name, loop] = {k: engine.stats.get(k, 0) - before.get(k, 0) for k in ("calls", "grouped_calls")}
            print(name, loop, out[name, loop], out["stats"][name, loop])
    return out


def _bytes(passes, name, loop, fn="predictions_val.json"):
    return open(passes["root"] / f"{name}_{loop}" / fn, "rb").read()


def test_one_tile_is_the_run_without_the_flag(passes):
    plain = _bytes(passes, "plain", "device")
    assert plain == _bytes(passes, "plain", "host") and len(json.loads(plain)["annotations"]) > 0
    for loop in ("host", "device"):
        assert _bytes(passes, "t1x1", loop) == plain
        a, b = passes["t1x1", loop], passes["plain", loop]
        keys = COUNT_KEYS + AP_KEYS + ("images",)
        assert all(k in a for k in keys) and _same({k: a[k] for k in keys}, {k: b[k] for k in keys})     # (APl is NaN on both sides: no large object)
        assert "loss_ce" in b and not any(k.startswith("loss_") or k in ("class_error", "cardinality_error") for k in a)
        assert passes["stats"]["t1x1", loop] == {"calls": len(IMAGES), "grouped_calls": 0}


def test_host_and_device_loops_agree_at_2x2(passes):
    host, dev = _bytes(passes, "t2x2", "host"), _bytes(passes, "t2x2", "device")
    assert host == dev != _bytes(passes, "plain", "device") and len(json.loads(dev)["annotations"]) > 0
    assert _same(passes["t2x2", "host"], passes["t2x2", "device"])
    m = passes["t2x2", "device"]
    assert all(k in m for k in COUNT_KEYS + AP_KEYS) and not any(k.startswith("loss_") or k in ("class_error", "cardinality_error") for k in m)
    assert passes["stats"]["t2x2", "device"] == passes["stats"]["t2x2", "host"] == {"calls": len(IMAGES), "grouped_calls": len(IMAGES)}


def test_host_and_device_loops_agree_with_scale_nms_sweep_and_report(passes):
    for fn in ("predictions_val.json", "threshold_sweep_val.json", "image_report_val.json"):
        assert _bytes(passes, "full", "host", fn) == _bytes(passes, "full", "device", fn), fn
    assert _same(passes["full", "host"], passes["full", "device"])
    m = passes["full", "device"]
    assert "nms_removed" in m and "AR1100" in m and not any(k.startswith("loss_") for k in m)
    assert _bytes(passes, "full", "device") != _bytes(passes, "t2x2", "device")
    rows = json.loads(_bytes(passes, "full", "device", "image_report_val.json"))["rows"]
    assert len(rows) == len(IMAGES)


def test_tile_below_tiles_exactly_the_images_with_small_exemplars(passes):
    small = sum(1 for im in IMAGES if im[4] < BELOW)
    assert 0 < small < len(IMAGES)
    for loop in ("host", "device"):
        assert passes["stats"]["below", loop] == {"calls": len(IMAGES), "grouped_calls": small}
    assert _bytes(passes, "below", "host") == _bytes(passes, "below", "device") and _same(passes["below", "host"], passes["below", "device"])
    ann = {name: json.loads(_bytes(passes, name, "device"))["annotations"] for name in ("plain", "t2x2", "below")}
    for k, im in enumerate(IMAGES):                 # per image the detections are the tiled pass's or the plain pass's
        pick = "t2x2" if im[4] < BELOW else "plain"
        got, want = ([{x: a[x] for x in ("bbox", "score", "point")} for a in ann[n] if a["image_id"] == k + 1] for n in ("below", pick))
        assert got == want, im[0]
