"""What the box overlays cost (infer.py --render_worst), device against host, on three generated sets of seeded canvases and boxes:

  (a) 8 canvases of 384 x 576 with 60 ground truths and 120 detections each (typical FSC-147 images),
  (b) one canvas of 384 x 576 with 3731 ground truths and 1100 detections (the data set's largest object count at the evaluator's maxDets),
  (c) one canvas of 800 x 1333 with 300 ground truths and 300 detections.

  launch : cdetr_render_boxes alone on inputs already on the device, by HIP events, median of 50 launches.
  device : the whole render.render_images(device=) call (uploads of the canvases, tables and boxes, the launch, the overlays' copy back), wall
           time, best of --repeats after a warm-up.
  host   : render.render_images(device=None), the numpy host implementation, wall time, best of --repeats.
The device's overlays are asserted equal to the host's.  No threshold is set: nobody had measured either side before.

usage: python tools/render_time.py [--out profiles/render_time.json] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from counting_detr_amd import ops, render


def make_set(rng, K, H, W, G, D):
    """K canvases with G ground truths (4 .. 40 pixels a side) and D detections (jittered copies of ground truths) each, three exemplars."""
    canvases, gts, dts, exs = [], [], [], []
    for _ in range(K):
        canvases.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        g = np.concatenate([rng.uniform(0.0, [W - 8.0, H - 8.0], (G, 2)), rng.uniform(4.0, 40.0, (G, 2))], axis=1)
        d = g[rng.integers(0, G, D)] + np.concatenate([rng.normal(0.0, 2.0, (D, 2)), rng.normal(0.0, 1.5, (D, 2))], axis=1)
        gts.append(g); dts.append(d); exs.append(g[:3].copy())
    pack = {"image_ids": list(range(K)), "gt_boxes": np.concatenate(gts), "dt_boxes": np.concatenate(dts),
            "gt_off": (np.arange(K + 1) * G).astype(np.int32), "dt_off": (np.arange(K + 1) * D).astype(np.int32)}
    return canvases, pack, rng.random(K * D) < 0.6, rng.random(K * D) < 0.05, exs


def timed(fn, repeats):
    best, out = None, None
    for _ in range(repeats):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_time: no GPU here -- the device side cannot be measured (nothing is written)")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    sets = [("a: 8 canvases of 384 x 576, 60 ground truths x 120 detections each", make_set(rng, 8, 384, 576, 60, 120)),
            ("b: 1 canvas of 384 x 576, 3731 ground truths x 1100 detections", make_set(rng, 1, 384, 576, 3731, 1100)),
            ("c: 1 canvas of 800 x 1333, 300 ground truths x 300 detections", make_set(rng, 1, 800, 1333, 300, 300))]
    rows = []
    for name, (canvases, pack, matched, ignored, exs) in sets:
        K = len(canvases)
        sel = list(range(K))
        with torch.cuda.device(dev):
            kwargs, pix_off = render.device_inputs(canvases, pack, matched, ignored, sel, None, exs, render.DEFAULT_STYLE, render.DEFAULT_DOT, dev)
            out = ops.render_boxes(**kwargs)                                                        # warm-up
            ms = []
            for _ in range(a.launches):
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ops.render_boxes(**kwargs, out=out, events=ev)
                torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            call = lambda: render.render_images(canvases, pack, matched, ignored, sel, exemplars=exs, device=dev)      # noqa: E731
            call()
            got, device_s = timed(call, a.repeats)
        want, host_s = timed(lambda: render.render_images(canvases, pack, matched, ignored, sel, exemplars=exs), a.repeats)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
        drawn = sum(int((w != c).any(axis=2).sum()) for w, c in zip(want, canvases))
        row = {"set": name, "canvases": K, "pixels": int(pix_off[-1]) // 3, "ground_truths": int(pack["gt_off"][-1]),
               "detections": int(pack["dt_off"][-1]), "pixels_drawn": drawn, "launch_ms_hip_events_median": float(np.median(ms)),
               "launch_ms_hip_events_min_max": [float(min(ms)), float(max(ms))], "render_images_device_s": device_s,
               "render_images_host_numpy_s": host_s, "overlays_equal": True}
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "the box overlays (infer.py --render_worst): cdetr_render_boxes by HIP events (median of %d launches, inputs on the device), the "
                   "whole render.render_images(device=) call (uploads, the launch, the overlays' copy back; wall seconds, best of %d after a "
                   "warm-up) and render.render_images(device=None), the numpy host implementation (wall seconds, best of %d).  No threshold: "
                   "first measurement of either side" % (a.launches, a.repeats, a.repeats),
           "tile": [render.TILE_H, render.TILE_W], "chunk": render.CHUNK, "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
