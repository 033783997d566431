"""A serial restatement of the bootstrap for the tests: the lists are expanded LITERALLY by multiplicity and handed to the code the project
already had (coco_ap.accumulate / _six, engine.counting_metrics); the draws are restated with Python ints.  Shared by test_bootstrap_cpu.py
and test_bootstrap_gpu.py; the random cases are made here once and are not modified by the tests."""
import numpy as np

from counting_detr_amd import coco_ap

M64 = (1 << 64) - 1


def draws_int(seed, r, N):
    """counting_detr_amd.bootstrap.draws, one Python int at a time."""
    out = []
    for j in range(N):
        x = ((seed * 0x9E3779B97F4A7C15) & M64) ^ ((r << 32) | j)
        x = (x + 0x9E3779B97F4A7C15) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        x ^= x >> 31
        out.append(((x >> 32) * N) >> 32)
    return out


def expanded_precision(matching, m, counts=None):
    """precision [A, T, 101] of ONE replicate the literal way: every detection of image k of `matching.image_ids` repeated m[k] times in the
    merged order (numpy.repeat: the copies stay together, so the order is still by descending score), npig summed with the same weights,
    coco_ap.accumulate on the expansion."""
    pack = matching.pack
    matched, ignored, npig = matching.host()
    slot = {int(i): k for k, i in enumerate(matching.image_ids)}
    w_img = np.array([m[slot[i]] for i in pack["image_ids"]], dtype=np.int64).reshape(-1)
    dt_off = np.asarray(pack["dt_off"], dtype=np.int64)
    image = np.repeat(np.arange(len(dt_off) - 1), np.diff(dt_off))
    keep = np.ones(len(image), dtype=bool)
    pc = matching.pack_counts(counts)
    if pc is not None:
        keep = (np.arange(len(image)) - dt_off[image]) < np.asarray(pc, dtype=np.int64)[image]
    order = np.argsort(-pack["dt_score"], kind="mergesort")
    order = order[keep[order]]
    rep = np.repeat(order, w_img[image[order]])
    out = []
    for a in range(len(matching.areas)):
        out.append(coco_ap.accumulate(pack["dt_score"][rep], matched[a][:, rep], ignored[a][:, rep], int((w_img * npig[a]).sum())))
    return np.stack(out)


def expanded_six(matching, m, counts=None):
    six = coco_ap._six(dict(zip(matching.areas, expanded_precision(matching, m, counts))))
    return [six[k] for k in ("AP", "AP50", "AP75", "APs", "APm", "APl")]


def expanded_counting(gt, pred, m):
    """engine.counting_metrics on the image list with image i repeated m[i] times, divided by the ORIGINAL number of images as the rule does
    (sum m = N for drawn multiplicities, where the two agree)."""
    from counting_detr_amd.engine import counting_metrics
    rep = np.repeat(np.arange(len(gt)), np.asarray(m, dtype=np.int64))
    return counting_metrics([int(pred[i]) for i in rep], [int(gt[i]) for i in rep])


def random_case(seed, n_img=7, max_gt=6, max_dt=9, ties=True, big=False):
    """A small evaluation with heavy score ties -> (gt_by_img, dt_by_img, image ids).  Some images have no detection, some no ground truth;
    `big`: boxes large enough for the area range `large` on a FEW images only (so that a replicate may draw none of them)."""
    rng = np.random.default_rng(seed)
    gt_by, dt_by, ids = {}, {}, list(range(10, 10 + n_img))
    for k, i in enumerate(ids):
        n_gt = 0 if k % 4 == 3 else int(rng.integers(1, max_gt + 1))
        n_dt = 0 if k % 5 == 4 else int(rng.integers(1, max_dt + 1))
        if k == 5:
            n_gt = n_dt = 0                                              # an image of the run that is in no pack
        gts, dts = [], []
        for _ in range(n_gt):
            side = float(rng.integers(100, 140)) if (big and k == 0) else float(rng.integers(8, 60))
            x, y = float(rng.integers(0, 200)), float(rng.integers(0, 200))
            gts.append({"bbox": [x, y, side, side], "area": side * side, "iscrowd": 0, "ignore": 0})
        for _ in range(n_dt):
            if gts and rng.random() < 0.7:
                g = gts[int(rng.integers(0, len(gts)))]["bbox"]
                b = [g[0] + float(rng.integers(-4, 5)), g[1] + float(rng.integers(-4, 5)), g[2] + float(rng.integers(-3, 4)), g[3]]
            else:
                s = float(rng.integers(8, 60))
                b = [float(rng.integers(0, 200)), float(rng.integers(0, 200)), s, s]
            score = float(np.float32(rng.integers(1, 5) / 4.0 if ties else rng.random()))
            dts.append({"bbox": b, "score": score, "area": b[2] * b[3]})
        if gts:
            gt_by[i] = gts
        if dts:
            dt_by[i] = dts
    return gt_by, dt_by, ids
