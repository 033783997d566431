"""Time of the 1st-stage training step (engine.Stage1Trainer) on one MI355X -> one JSON line.

    python tools/stage1_step_time.py [--steps 20] [--warmup 5] [--out profiles/stage1_step_time.json] [--no-profile]

Measures images/s of the stream-ordered step (`train_step`) and of the graph-cached step (`step`: captured once, then replayed) at
384x576 with B=1 (the reference's batch) and B=4 (four images of one size, 3 exemplars each), seeded weights and batches.  Then, unless
--no-profile, the same workload runs again in a SEPARATE child process under `rocprofv3 --kernel-trace --stats` (--leg profile: a few
steps of each form, nothing timed) and the share of kernel time spent in this repository's kernels (libcdetr_hip.so) is read from its
kernel_stats CSV; the CSV is copied next to --out.  Each child runs under its own time limit.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((1, 384, 576), (4, 384, 576))


def _setup(B, H, W):
    import torch
    from counting_detr_amd import stage1
    from counting_detr_amd.args import get_args_parser_stage1
    from counting_detr_amd.engine import Stage1Trainer
    from oracle.weights import seeded_state_dict, stage1_schema
    args = get_args_parser_stage1().parse_args([])
    args.device = "cuda:0"
    model, crit, _ = stage1.build(args)
    model.load_state_dict(seeded_state_dict(stage1_schema()), strict=True)
    model.to(args.device).train()
    tr = Stage1Trainer(model, crit, args, device=args.device)
    g = torch.Generator().manual_seed(5000 + B)
    batch = (torch.randn(B, 3, H, W, generator=g).cuda(), (torch.rand(B, 3, 2, generator=g) * 0.6 + 0.2).cuda(),
             (torch.rand(B, 3, 2, generator=g) * 0.15 + 0.03).cuda())
    return tr, batch


def _time(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def measure(steps, warmup):
    res = {}
    for B, H, W in SHAPES:
        tr, batch = _setup(B, H, W)
        t_e, out_e = _time(lambda: tr.train_step(*batch), steps, warmup)
        t_g, out_g = _time(lambda: tr.step(*batch), steps, warmup)
        assert tr.cache_stats["captures"] == 1, tr.cache_stats
        res[f"B{B}_{H}x{W}"] = {"eager_ms": round(t_e * 1e3, 3), "eager_img_s": round(B / t_e, 1), "graph_ms": round(t_g * 1e3, 3),
                                "graph_img_s": round(B / t_g, 1), "graph_speedup": round(t_e / t_g, 2),
                                "loss_last": round(float(out_g["loss"]), 5), "nonfinite_steps": tr.nonfinite_steps()}
        del tr
    return res


def profile_leg(steps):
    for B, H, W in SHAPES:
        tr, batch = _setup(B, H, W)
        for _ in range(steps):
            tr.train_step(*batch)
            tr.step(*batch)
    import torch
    torch.cuda.synchronize()


def kernel_share(csv_path):
    rows = list(csv.DictReader(open(csv_path)))
    rows = [r for r in rows if "flag_wait_kernel" not in r["Name"] and "delay_kernel" not in r["Name"]]      # sleeping, not working
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    ours = sum(float(r["TotalDurationNs"]) for r in rows if "anonymous namespace)::" in r["Name"] and "at::native" not in r["Name"])
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]
    return {"kernel_ms_total": round(tot / 1e6, 3), "in_tree_share": round(ours / tot, 4) if tot else None,
            "top": [{"name": r["Name"][:80], "ms": round(float(r["TotalDurationNs"]) / 1e6, 3), "calls": int(r["Calls"])} for r in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--leg", default="time", choices=["time", "profile"])
    a = ap.parse_args()
    if a.leg == "profile":
        profile_leg(3)
        return
    line = {"what": "stage-1 training step (engine.Stage1Trainer), seeded weights, 3 exemplars per image",
            "steps": a.steps, "warmup": a.warmup, "shapes": measure(a.steps, a.warmup)}
    if not a.no_profile:
        work = tempfile.mkdtemp(prefix="stage1_prof_")
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "-o", "stage1", "--",
               sys.executable, os.path.abspath(__file__), "--leg", "profile"]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        found = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode == 0 and found:
            line["profile"] = kernel_share(found[0])
            line["profile"]["legs"] = "3 eager + 3 graph steps per shape (captures and warm-ups included)"
            if a.out:
                shutil.copy(found[0], os.path.splitext(a.out)[0] + "_kernel_stats.csv")
        else:
            line["profile"] = {"error": f"rocprofv3 exit {p.returncode}", "tail": (p.stdout + p.stderr)[-800:]}
        shutil.rmtree(work, ignore_errors=True)
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
