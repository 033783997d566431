"""The tiling rule (counting_detr_amd/tiling.py) on the host: geometry, exemplar ownership, the identities at 1x1, a constructed seam case with
nms.suppress behind the stitch, and the start-up checks of --tiles / --tile_margin / --tile_scale / --tile_below.  Every comparison is exact."""
import numpy as np
import pytest

from counting_detr_amd import nms, tiling
from counting_detr_amd.args import check_tile_flags, get_args_parser

SIDES = (32, 64, 96, 160, 70)
GRIDS = ((1, 1), (1, 2), (2, 2), (1, 4))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("R,C", GRIDS)
@pytest.mark.parametrize("W", SIDES)
@pytest.mark.parametrize("H", SIDES)
def test_cores_partition_the_image_and_tiles_hold_their_cores(H, W, R, C):
    for M in (0, 32, 7):
        plan = tiling.Plan(H, W, R, C, M, 1)
        nr, nc = plan.grid
        assert plan.T == nr * nc <= R * C == plan.slots and len(plan.boxes) == len(plan.cores) == plan.T
        cover = np.zeros((H, W), dtype=np.int32)
        for (x0, y0, x1, y1), (kx0, ky0, kx1, ky1) in zip(plan.boxes, plan.cores):
            cover[ky0:ky1, kx0:kx1] += 1
            assert 0 <= x0 <= kx0 < kx1 <= x1 <= W and 0 <= y0 <= ky0 < ky1 <= y1 <= H              # inside the image, around its core
            assert kx0 - x0 in (M, kx0) and x1 - kx1 in (M, W - kx1) and ky0 - y0 in (M, ky0) and y1 - ky1 in (M, H - ky1)
        assert (cover == 1).all()                                                                    # every pixel in exactly one core
        for L, n, c in ((H, R, plan.cy), (W, C, plan.cx)):
            assert c[0] == 0 and c[-1] == L and all(b % 32 == 0 for b in c[:-1]) and len(c) - 1 == min(n, max(L // 32, 1))
        assert plan.records.shape == (plan.T, 5) and plan.coef.shape == (plan.T, 8)
        assert plan.Hm == max(b[3] - b[1] for b in plan.boxes) and plan.Wm == max(b[2] - b[0] for b in plan.boxes)


def test_parts_shrink_where_the_axis_is_short():
    assert tiling.axis(32, 2, 32) == ([0, 32], [(0, 32)]) and tiling.axis(32, 4, 0)[0] == [0, 32]
    assert tiling.axis(31, 3, 5) == ([0, 31], [(0, 31)])                   # shorter than one unit: one part
    assert tiling.axis(64, 4, 0)[0] == [0, 32, 64] and tiling.axis(160, 4, 32) == ([0, 32, 64, 96, 160], [(0, 64), (0, 96), (32, 128), (64, 160)])
    assert tiling.axis(70, 2, 0) == ([0, 32, 70], [(0, 32), (32, 70)])
    plan = tiling.Plan(32, 160, 2, 2, 32, 2)
    assert plan.grid == (1, 2) and plan.T == 2 and plan.slots == 4 and (plan.Hm, plan.Wm) == (64, 2 * 128)
    assert plan.records.tolist() == [[0, 0, 96, 32, 2], [32, 0, 128, 32, 2]]


@pytest.mark.parametrize("R,C,H,W", [(2, 2, 128, 192), (1, 4, 70, 160), (2, 2, 32, 64), (1, 1, 96, 96)])
def test_every_exemplar_is_present_in_exactly_one_tile(R, C, H, W):
    rng = np.random.default_rng(R * 100 + C * 10 + H)
    plan = tiling.Plan(H, W, R, C, 32, 1)
    for _ in range(20):
        c, s = rng.uniform(0.0, 1.0, (3, 2)), rng.uniform(0.01, 0.2, (3, 2))
        rects = np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)
        rects[rng.integers(0, 3)] = -1.0 if rng.random() < 0.3 else rects[0]          # sometimes an absent row
        out = tiling.tile_rects(rects, plan)
        assert out.shape == (plan.T, 3, 4) and out.dtype == np.float32
        for k in range(3):
            present = [t for t in range(plan.T) if out[t, k, 2] >= 0]
            if rects[k, 2] < 0:
                assert present == [] and (out[:, k] == -1).all()
                continue
            assert len(present) == 1
            t = present[0]
            cx, cy = (float(rects[k, 0]) + float(rects[k, 2])) / 2 * W, (float(rects[k, 1]) + float(rects[k, 3])) / 2 * H
            kx0, ky0, kx1, ky1 = plan.cores[t]
            assert (kx0 <= cx or kx0 == 0) and (cx < kx1 or kx1 == W) and (ky0 <= cy or ky0 == 0) and (cy < ky1 or ky1 == H)
            x0, y0, x1, y1 = plan.boxes[t]                                              # the rect went into the tile's own coordinates
            want = (np.array([rects[k, 0] * W - x0, rects[k, 1] * H - y0, rects[k, 2] * W - x0, rects[k, 3] * H - y0], dtype=np.float64)
                    / [x1 - x0, y1 - y0, x1 - x0, y1 - y0])
            assert np.abs(out[t, k] - want).max() < 1e-5
            assert (np.delete(out[:, k], t, axis=0) == -1).all()


def test_a_whole_image_tile_returns_the_rects_bit_for_bit():
    rects = np.array([[0.1, 0.2, 0.3, 0.7], [-0.0, 0.0, 1.0, 0.99999994], [-1, -1, -1, -1]], dtype=np.float32)
    for plan in (tiling.Plan(96, 160, 1, 1, 32, 1), tiling.Plan(32, 32, 2, 2, 32, 1), tiling.Tiling(2, 2, below=1.0).plan_for(96, 160, rects)):
        assert plan.T == 1 and plan.whole and plan.boxes == [(0, 0, plan.W, plan.H)]
        out = tiling.tile_rects(rects, plan)
        assert out.shape == (1, 3, 4) and np.array_equal(bits(out[0]), bits(rects))
        image = np.random.default_rng(0).standard_normal((3, plan.H, plan.W)).astype(np.float32)
        tiles, mask = tiling.tile_images(image, plan)
        assert np.array_equal(bits(tiles[0]), bits(image)) and not mask.any()


def test_stitch_at_1x1_is_the_identity_on_every_bit():
    rng = np.random.default_rng(5)
    Q = 70
    prob = rng.uniform(0, 1, (1, Q)).astype(np.float32)
    boxes, points = rng.uniform(-0.2, 1.2, (1, Q, 4)).astype(np.float32), rng.uniform(0, 1, (1, Q, 2)).astype(np.float32)
    prob[0, 3], prob[0, 4] = np.nan, -0.0
    boxes[0, 5, 0], boxes[0, 6, 1], boxes[0, 7, 2], boxes[0, 8, 0] = -0.0, np.nan, -0.0, np.inf
    points[0, 9, 0], points[0, 10, 1] = -0.0, np.nan
    for H, W in ((96, 160), (70, 100), (32, 32)):
        p, b, r = tiling.stitch(prob, boxes, points, tiling.Plan(H, W, 1, 1, 32, 1))
        assert p.shape == (Q,) and b.shape == (Q, 4) and r.shape == (Q, 2)
        assert np.array_equal(bits(p), bits(prob[0])) and np.array_equal(bits(b), bits(boxes[0])) and np.array_equal(bits(r), bits(points[0]))


def test_missing_tiles_are_nan_with_zero_boxes():
    plan = tiling.Plan(32, 160, 2, 2, 0, 1)                                # one row of two tiles in four slots
    Q = 3
    prob = np.full((2, Q), 0.9, dtype=np.float32)
    boxes = np.tile(np.array([0.5, 0.5, 0.1, 0.1], dtype=np.float32), (2, Q, 1))
    p, b, r = tiling.stitch(prob, boxes, boxes[..., :2].copy(), plan)
    assert p.shape == (4 * Q,) and np.isnan(p[2 * Q:]).all() and not np.isnan(p[:2 * Q]).any()
    assert (b[2 * Q:] == 0).all() and (r[2 * Q:] == 0).all()


def _seam(centres):
    """Two tiles of a 128 x 128 image at 1x2 (cores [0, 64) and [64, 128), tiles [0, 96) and [32, 128)) each predicting one 20 x 20 box around
    an object on the seam, its centre at x = centres[t] whole-image pixels -> the stitched (prob, boxes)."""
    plan = tiling.Plan(128, 128, 1, 2, 32, 1)
    assert plan.boxes == [(0, 0, 96, 128), (32, 0, 128, 128)] and plan.cores == [(0, 0, 64, 128), (64, 0, 128, 128)]
    boxes = np.zeros((2, 1, 4), dtype=np.float32)
    for t, cx in enumerate(centres):
        x0 = plan.boxes[t][0]
        boxes[t, 0] = ((cx - x0) / 96, 0.5, 20 / 96, 20 / 128)
    prob = np.array([[0.9], [0.8]], dtype=np.float32)
    p, b, _ = tiling.stitch(prob, boxes, boxes[..., :2].copy(), plan)
    assert np.abs(b[:, 0] * 128 - np.asarray(centres)).max() < 1e-3 and np.abs(b[:, 2] * 128 - 20).max() < 1e-3
    return p, b


def test_seam_object_with_both_centres_on_one_side_survives_once():
    p, _ = _seam((62.0, 63.5))
    assert bits(p[:1]) == bits(np.float32(0.9)) and np.isnan(p[1])         # the left tile owns it, the right tile's copy is dropped
    p, _ = _seam((64.0, 66.0))                                             # exactly on the bound: the right core's
    assert np.isnan(p[0]) and bits(p[1:]) == bits(np.float32(0.8))


def test_seam_object_with_centres_on_both_sides_survives_twice_and_nms_removes_one():
    p, b = _seam((62.0, 66.0))
    assert not np.isnan(p).any()
    out, removed = nms.suppress(p[None], b[None], [[128, 128]], 0.5, 0.5)
    assert removed.tolist() == [1] and bits(out[0, :1]) == bits(np.float32(0.9)) and np.isnan(out[0, 1])


def test_small_exemplar_rule():
    rects = np.array([[0.1, 0.1, 0.2, 0.2], [0.5, 0.5, 0.6, 0.7], [-1, -1, -1, -1]], dtype=np.float32)
    r = rects.astype(np.float64)
    want = (np.sqrt((r[0, 2] - r[0, 0]) * 200 * (r[0, 3] - r[0, 1]) * 100) + np.sqrt((r[1, 2] - r[1, 0]) * 200 * (r[1, 3] - r[1, 1]) * 100)) / 2
    assert abs(tiling.exemplar_size(rects, 100, 200) - want) < 1e-9
    assert tiling.exemplar_size(np.full((3, 4), -1.0, dtype=np.float32), 100, 200) is None
    t = tiling.Tiling(2, 2, below=want + 1e-6)
    assert t.tiled(100, 200, rects) and not tiling.Tiling(2, 2, below=want).tiled(100, 200, rects)      # strictly below
    assert t.plan_for(100, 200, rects).T == 4 and tiling.Tiling(2, 2, below=1.0).plan_for(100, 200, rects).T == 1
    assert tiling.Tiling(2, 2, below=1.0).plan_for(100, 200, rects).slots == 4
    assert not t.tiled(100, 200, np.full((3, 4), -1.0, dtype=np.float32))


def test_group_feature_is_the_running_sum_over_the_group():
    rng = np.random.default_rng(9)
    h, w, C, K = 3, 5, 8, 3
    x = rng.standard_normal((4, h * w, C)).astype(np.float32)
    rects = np.full((4, K, 4), -1.0, dtype=np.float32)
    rects[0, 0], rects[0, 2], rects[2, 1] = (0.1, 0.1, 0.3, 0.3), (0.1, 0.1, 0.3, 0.3), (0.7, 0.5, 0.9, 0.9)
    extent = np.array([[3, 5], [3, 5], [2, 4], [3, 5]], dtype=np.float32)
    pf, idx = tiling.group_feature(x, rects, extent, h, w, 4)
    assert idx.tolist() == [[1, -1, 1], [-1, -1, -1], [-1, 1 * 5 + 3, -1], [-1, -1, -1]]
    acc = (x[0, 1] + x[0, 1]) + x[2, 8]
    assert np.array_equal(bits(pf), bits(np.tile(acc * (np.float32(1) / np.float32(3)), (4, 1))))
    pf1, _ = tiling.group_feature(x, rects, extent, h, w, 1)
    assert np.array_equal(bits(pf1[1]), bits(np.zeros(C))) and np.array_equal(bits(pf1[2]), bits(x[2, 8] * np.float32(1)))


# ------------------------------------------------------------------------------------------------------------------ flags
def _error(argv, capsys):
    with pytest.raises(SystemExit):
        get_args_parser().parse_args(argv)
    return capsys.readouterr().err


def test_namespace_without_the_flags_is_unchanged():
    ns = get_args_parser().parse_args([])
    assert not any(hasattr(ns, k) for k in ("tiles", "tile_margin", "tile_scale", "tile_below"))
    ns = get_args_parser().parse_args(["--tiles", "2x2", "--tile_margin", "16", "--tile_scale", "2", "--tile_below", "24.5"])
    assert ns.tiles == (2, 2) and ns.tile_margin == 16 and ns.tile_scale == 2 and ns.tile_below == 24.5
    assert get_args_parser().parse_args(["--tiles", "1x1"]).tiles == (1, 1)
    assert get_args_parser().parse_args(["--tiles", "1x4", "--tile_margin", "0"]).tile_margin == 0


def test_start_up_errors(capsys):
    for flag, value in (("--tile_margin", "8"), ("--tile_scale", "2"), ("--tile_below", "20")):
        assert flag + " needs --tiles" in _error([flag, value], capsys)
    err = _error(["--tiles", "2x3"], capsys)                               # 2 * 3 * 900 = 5400
    assert all(n in err for n in ("2", "3", "900", "5400", "4096"))
    assert "4800" in _error(["--tiles", "4x4", "--num_query_pattern", "1"], capsys)
    assert get_args_parser().parse_args(["--tiles", "2x2"]).tiles == (2, 2)                         # 3600 fits
    assert "--eval_batch_size" in _error(["--tiles", "2x2", "--eval_batch_size", "2"], capsys)
    assert "not built for tiles" in _error(["--tiles", "2x2", "--eval_every", "1"], capsys)
    for bad in ("0x2", "2x0", "2", "axb", "-1x2"):
        assert "--tiles" in _error(["--tiles", bad], capsys)
    assert "--tile_margin" in _error(["--tiles", "2x2", "--tile_margin", "-1"], capsys)
    assert "--tile_scale" in _error(["--tiles", "2x2", "--tile_scale", "3"], capsys)


def test_a_namespace_built_by_hand_meets_the_same_checks():
    import infer as infer_mod
    from counting_detr_amd.args import default_args
    assert infer_mod.build_tiling(default_args()) is None
    with pytest.raises(ValueError, match="needs --tiles"):
        infer_mod.build_tiling(default_args(tile_scale=2))
    with pytest.raises(ValueError, match="4800"):
        check_tile_flags(default_args(tiles=(4, 4)))                       # default_args: 300 queries
    with pytest.raises(ValueError, match="eval_batch_size"):
        infer_mod.build_tiling(default_args(tiles=(2, 2), eval_batch_size=4))
    t = infer_mod.build_tiling(default_args(tiles=(2, 2), tile_margin=16, tile_scale=2, tile_below=30.0))
    assert (t.R, t.C, t.margin, t.scale, t.below) == (2, 2, 16, 2, 30.0)
    t = infer_mod.build_tiling(default_args(tiles=(1, 2)))
    assert (t.margin, t.scale, t.below) == (32, 1, None)
