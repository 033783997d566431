"""coco_ap.Matching on the host route: every reading of ONE matching -- the six numbers, the six numbers per score threshold, the per-image
statistics with and without prefix lengths, row [0, 0] -- against the functions that match for themselves (`summarize`, `summarize_sweep`) and
against `stats_from_flags` on `_evaluate_image`'s flags put side by side by tests/coco_ap_cases.py.  Every comparison is ==, the average
precisions as float64 BITS.  tests/test_coco_ap_device_gpu.py holds a device matching to the same answers."""
import numpy as np
import pytest

from counting_detr_amd import coco_ap as ca

import coco_ap_cases as cc

AREAS = tuple(ca.AREA_RNG)
THRESHOLDS = (0.0, 0.25, 0.5, 0.9, 2.0)
CUTS = (5, 20, 1100)


SETS = cc.matching_sets()
same_six, same_stats = cc.same_six, cc.same_stats


def flags_of(gts, dts):
    """The flags of a set without coco_ap.Matching: (matched [A, T, D], det_ignored [A, T, D], dt_off [B + 1], npig [A, B], image ids)."""
    per = [cc.host_flags(gts, dts, a) for a in AREAS]
    ids = [i for i in sorted(set(gts) | set(dts)) if gts.get(i) or dts.get(i)]
    dt_off = np.concatenate([[0], np.cumsum([min(len(dts.get(i, [])), ca.MAX_DETS) for i in ids])]).astype(np.int64)
    return np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), dt_off, np.stack([p[3] for p in per]).reshape(len(AREAS), len(ids)), ids


@pytest.mark.parametrize("name", list(SETS))
def test_every_reading_of_a_host_matching(name):
    gts, dts = SETS[name]
    m = ca.Matching.of(gts, dts)
    matched, ignored, dt_off, npig, ids = flags_of(gts, dts)
    assert m.device is None and m.areas == AREAS and m.pack["image_ids"] == ids and 99 not in ids
    for got, want in zip(m.host(), (matched, ignored, npig)):
        assert got.shape == want.shape and np.array_equal(got, want)
    assert m.host()[0] is m.matched                                            # host flags are what they are: nothing is copied
    same_six(m.six(), ca.summarize(gts, dts))
    rows, want_rows = m.six_sweep(THRESHOLDS), ca.summarize_sweep(gts, dts, THRESHOLDS)
    assert len(rows) == len(want_rows) == len(THRESHOLDS)
    for got, want in zip(rows, want_rows):
        same_six(got, want)
    same_six(rows[0], m.six())                                                  # every score is >= 0: the lowest threshold keeps everything
    stats = m.stats(CUTS)
    same_stats(stats, ca.image_stats(gts, dts, cuts=CUTS))
    same_stats(stats, ca._stats_dict(ids, *ca.stats_from_flags(matched, ignored, dt_off, npig, CUTS), npig, CUTS))
    m50, ig50 = m.row50()
    assert np.array_equal(m50, matched[0, 0]) and np.array_equal(ig50, ignored[0, 0]) and m50.shape == (int(dt_off[-1]),)
    if name != "empty":
        assert (stats["ap"][0] > 0).any() and (stats["ap"] == -1).any() and not np.isnan(m.six()["AP"])
    else:
        assert stats["tp"].shape == (4, 0, 10, 3) and m.pack["dt_off"].tolist() == [0] and np.isnan(m.six()["AP"])


@pytest.mark.parametrize("name", ["tie", "float"])
def test_prefix_counts_equal_the_truncated_lists(name):
    """counts of 0, beyond the segment and in between, given in the pack's own order and in a caller's order (a store's)."""
    gts, dts = SETS[name]
    m = ca.Matching.of(gts, dts)
    ids = m.pack["image_ids"]
    lens = np.diff(m.pack["dt_off"]).tolist()
    counts = [0, lens[1] + 9] + [n // 2 for n in lens[2:-1]] + [lens[-1] - 1]
    assert m.pack_counts(None) is None and m.pack_counts(counts) == counts and gts[ids[0]] and 0 < counts[-1] < lens[-1]
    by_score = {i: sorted(dts[i], key=lambda d: -d["score"]) for i in ids}     # stable: the evaluation order
    cut = ca.image_stats(gts, {i: by_score[i][:c] for i, c in zip(ids, counts)}, cuts=CUTS)
    got = m.stats(CUTS, counts)
    assert got["image_ids"] == cut["image_ids"] == ids                          # an image cut to nothing keeps its ground truths
    same_stats(got, cut)
    assert not np.array_equal(got["tp"], m.stats(CUTS)["tp"])
    # a caller's order: reversed, with an image the pack does not hold and without the pack's last one
    theirs = ca.Matching(m.pack, m.areas, m.matched, m.det_ignored, m.npig, image_ids=[12345] + ids[-2::-1])
    assert theirs.pack_counts([7] + counts[-2::-1]) == counts[:-1] + [0]
    same_stats(theirs.stats(CUTS, [7] + counts[-2::-1]), m.stats(CUTS, counts[:-1] + [0]))
