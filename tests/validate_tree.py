"""Shared by tests/test_validate_cpu.py and tests/test_validate_gpu.py (not a test module): an FSC-147 tree with a train split AND a val
split, for validation inside a training run (main.py / main_stage1.py --eval_every).

  val    the five images of eval_split.IMAGES with instances_val.json (eval_split.write_split, unchanged);
  train  four seeded-noise images, two resizing to 96x64 and two to 64x96 (the training reader's floor(w / 32) * 32), 4-9 pseudo-label
         boxes each in annotations/pseudo_bbox_train.json ([cx, cy, w, h] pixels, what the stage-2 reader wants), three exemplar boxes each in
         annotation_FSC147_384.json (stage 2's rectangles, stage 1's points + sizes) and their names under "train" in the split file.
The smallest shapes at which stale weight images, dropped graphs or a wrong epoch in the best-keeper still show."""
import json
import os

import numpy as np

from eval_split import IMAGES, write_split

# (file, width, height, boxes)
TRAIN_IMAGES = [("t0.png", 100, 70, 4), ("t1.png", 70, 100, 9), ("t2.png", 99, 67, 6), ("t3.png", 66, 98, 7)]
TRAIN_RESIZED = [(96, 64), (64, 96), (96, 64), (64, 96)]
VAL_IMAGES = IMAGES
# the model of the existing end-to-end tests
MODEL_FLAGS = ["--no_aux_loss", "--num_query_pattern", "1", "--num_query_position", "100", "--num_workers", "0"]


def write_tree(root, seed=5):
    """-> data_path of the tree written under `root` (which must not exist yet, or be empty)."""
    from PIL import Image
    root = write_split(root)
    rng = np.random.default_rng(seed)
    with open(os.path.join(root, "annotation_FSC147_384.json")) as f:
        anno = json.load(f)
    with open(os.path.join(root, "Train_Test_Val_FSC_147.json")) as f:
        split = json.load(f)
    os.makedirs(os.path.join(root, "annotations"))
    images, annotations = [], []
    for k, (name, w, h, n) in enumerate(TRAIN_IMAGES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "images_384_VarV2", name))
        wh = rng.uniform(4.0, 12.0, (n, 2))
        xy = rng.uniform(1.0, [w - 14.0, h - 14.0], (n, 2))                # top-left corners: every box lies inside the image
        images.append({"id": 101 + k, "file_name": name, "width": w, "height": h})
        for (cx, cy), (bw, bh) in zip((xy + wh / 2).tolist(), wh.tolist()):
            annotations.append({"id": len(annotations) + 1, "image_id": 101 + k, "bbox": [cx, cy, bw, bh], "category_id": 1, "area": bw * bh,
                                "iscrowd": 0})
        ex = [[[x, y], [x, y + bh], [x + bw, y + bh], [x + bw, y]] for (x, y), (bw, bh) in zip(xy[:3].tolist(), wh[:3].tolist())]
        anno[name] = {"box_examples_coordinates": ex, "points": (xy + wh / 2).tolist(), "H": h, "W": w}
    split["train"] = [im[0] for im in TRAIN_IMAGES]
    for fn, obj in (("annotation_FSC147_384.json", anno), ("Train_Test_Val_FSC_147.json", split),
                    (os.path.join("annotations", "pseudo_bbox_train.json"),
                     {"images": images, "annotations": annotations, "categories": [{"id": 1, "name": "fg"}]})):
        with open(os.path.join(root, fn), "w") as f:
            json.dump(obj, f)
    return root
