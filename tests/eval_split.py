"""Shared by tests/test_eval_batches_cpu.py and tests/test_eval_batches_gpu.py (not a test module): a five-image FSC-147 validation split of
seeded-noise PNGs written into a directory -- three images of one resized size and two of another, interleaved, so that
data.SizeBucketBatchSampler at batch size 2 gives [0, 2], [4], [1, 3] -- and the stacks of reference goldens (batch 1, equal Q) that the
per-image criterion is pinned to."""
import json
import os

import numpy as np

# (file, width, height, targets): 101x70 / 100x66 / 97x69 resize to 96x64 at scale_factor 32, 70x100 / 67x99 to 64x96
IMAGES = [("a0.png", 101, 70, 6), ("b0.png", 70, 100, 9), ("a1.png", 100, 66, 4), ("b1.png", 67, 99, 7), ("a2.png", 97, 69, 5)]
RESIZED = [(96, 64), (64, 96), (96, 64), (64, 96), (96, 64)]
BATCHES_AT_2 = [[0, 2], [4], [1, 3]]

# reference goldens stacked into one batch: (file, [case, ...]); every case is a batch of one with the same Q
STACKS = {"q300": [("g45_matcher_criterion.npz", "q300_t37"), ("g45_matcher_criterion.npz", "q300_t450"), ("g45_large_t.npz", "q300_t1100"),
                   ("g45_large_t.npz", "q300_t3000")],
          "q900": [("g45_matcher_criterion.npz", "q900_t56"), ("g45_matcher_criterion.npz", "q900_t900"), ("g45_large_t.npz", "q900_t3000")],
          "negvar": [("g45_matcher_criterion.npz", "negvar"), ("g45_matcher_criterion.npz", "negvar")]}
LOSS_KEYS = ("loss_ce", "class_error", "cardinality_error", "loss_bbox", "loss_giou", "loss_variance")


def write_split(root, seed=3):
    """-> data_path of the split written under `root` (val = the five images of IMAGES, image ids 1 .. 5)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "images_384_VarV2"))
    anno, images, annotations = {}, [], []
    for k, (name, w, h, n) in enumerate(IMAGES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "images_384_VarV2", name))
        wh = rng.uniform(4.0, 12.0, (n, 2))
        xy = rng.uniform(1.0, [w - 14.0, h - 14.0], (n, 2))
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


def load_stack(golden, key):
    """-> (outputs dict of [B, Q, .] numpy arrays, [target boxes [T_b, 4]], [(idx_i, idx_j)], {loss key: [B] recorded L_*}) of one stack."""
    cases = [(golden(f), n) for f, n in STACKS[key]]
    for z, n in cases:
        assert int(z[f"{n}/B"]) == 1
    outs = {k: np.concatenate([z[f"{n}/{k}"] for z, n in cases]) for k in ("pred_logits", "pred_boxes", "pred_vars")}
    tgts = [z[f"{n}/tgt0"].reshape(-1, 4) for z, n in cases]
    idx = [(z[f"{n}/idx_i0"], z[f"{n}/idx_j0"]) for z, n in cases]
    want = {k: np.array([float(z[f"{n}/L_{k}"]) for z, n in cases], dtype=np.float32) for k in LOSS_KEYS}
    return outs, tgts, idx, want
