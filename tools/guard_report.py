#!/usr/bin/env python3
"""Cost of the guarded optimiser step (FusedRAdam max_grad_norm / skip_nonfinite) at the headline training shape.

    python tools/guard_report.py [--out profiles/guarded_step.json] [--modes f32 bf16] [--warmup 40] [--blocks 8] [--steps 10]

Per --mma mode, on ONE model and ray batch (bench.py's train set-up: 4096 rays x (128 + 128 + 64 + 64), 8 x 256, past the loss
warm-up): parallel.train_step with an unguarded FusedRAdam (A) and with a guarded one (B: max_grad_norm 1.0, skip_nonfinite on),
interleaved A B A B ... in blocks of --steps steps, each block between two HIP events, after --warmup steps per arm (the clocks
settle over the first seconds of load: blocks timed before that drift by several ms).  Reported: ms per step of every block, the
median per arm, the arm's spread (max - min over its blocks), B - A of the medians, and the median of the per-pair differences
B_i - A_i (neighbouring blocks: what drift is left cancels).  Then the optimiser launches alone, each between two
events on the gradients the last step left: rsn_radam_step, rsn_grad_sumsq, rsn_radam_step_guarded (median of --kernel-reps calls;
an event pair around one short launch includes the launch gap, so these are upper bounds of the kernels' own time).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import _abi, ops, train_ops  # noqa: E402
from reflect_sampling_nerf_amd.parallel import train_step  # noqa: E402
from reflect_sampling_nerf_amd.synthetic import synthetic_rays  # noqa: E402


def setup(dev, mma, rays, samples, layers, width):
    torch.manual_seed(0)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=samples[0], num_importance_samples=samples[1],
                                            num_reflect_coarse_samples=samples[2], num_reflect_importance_samples=samples[3],
                                            base_mlp_num_layers=layers, base_mlp_layer_width=width)
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 2.0
    model.to(dev).train()
    model.field.set_mma_mode(mma)
    o, d, pa = synthetic_rays(rays, seed=0)
    rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.reshape(rays, 1).to(dev),
                       nears=torch.full((rays, 1), 2.0, device=dev), fars=torch.full((rays, 1), 6.0, device=dev))
    batch = {"image": torch.rand(rays, 3, generator=torch.Generator().manual_seed(1234)).to(dev)}
    return model, rb, batch


def timed_block(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / steps


def kernel_times(opt_plain, opt_guard, reps):
    """Each optimiser launch alone between two events, on the gradients the parameters hold.  Parameters and moments move with
    every call; no timing depends on their values."""
    lib = _abi.load_library()
    params = opt_guard.params
    n = len(params)
    grads = [None if p.grad is None else ops._f32c(p.grad) for p in params]
    g = train_ops._ptr_array(grads)
    p_arr = train_ops._ptr_array([p.data for p in params])
    stream = ops._stream()
    ws, ws_bytes = _abi.ptr(opt_guard._guard_ws), opt_guard._guard_ws.numel() * 8
    stats = _abi.ptr(opt_guard._guard_stats)

    def plain():
        _abi.check(lib.rsn_radam_step(n, p_arr, g, train_ops._ptr_array(opt_plain.exp_avg), train_ops._ptr_array(opt_plain.exp_avg_sq),
                                      opt_plain._sizes, 200, 1e-3, 0.9, 0.999, 1e-15, stream))

    def sumsq():
        _abi.check(lib.rsn_grad_sumsq(n, g, opt_guard._sizes, ws, ws_bytes, stream))

    def guarded():
        _abi.check(lib.rsn_radam_step_guarded(n, p_arr, g, train_ops._ptr_array(opt_guard.exp_avg),
                                              train_ops._ptr_array(opt_guard.exp_avg_sq), opt_guard._sizes, 200, 1e-3, 0.9, 0.999,
                                              1e-15, 1.0, 1, ws, ws_bytes, stats, stream))

    out = {}
    for name, fn in (("rsn_radam_step", plain), ("rsn_grad_sumsq", sumsq), ("rsn_radam_step_guarded", guarded)):
        fn()
        torch.cuda.synchronize()
        spans = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            spans.append((s, e))
        torch.cuda.synchronize()
        us = sorted(1e3 * s.elapsed_time(e) for s, e in spans)
        out[name] = {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "calls": reps}
    out["gradient_bytes"] = int(sum(4 * t.numel() for t in grads if t is not None))
    out["gradient_tensors"] = int(sum(t is not None for t in grads))
    return out


def measure(dev, mma, args):
    model, rb, batch = setup(dev, mma, args.rays, args.samples, args.layers, args.width)
    params = model.get_param_groups()["fields"]
    kw = dict(lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)
    arms = {"off": pkg.FusedRAdam(params, **kw), "on": pkg.FusedRAdam(params, max_grad_norm=1.0, skip_nonfinite=True, **kw)}
    it = [100]

    def step_with(opt):
        def fn():
            train_step(model, rb, batch, opt, None, it[0])
            it[0] += 1
        return fn

    for opt in arms.values():
        for _ in range(args.warmup):
            step_with(opt)()
    torch.cuda.synchronize()
    blocks = {"off": [], "on": []}
    for _ in range(args.blocks):
        for name, opt in arms.items():
            blocks[name].append(timed_block(step_with(opt), args.steps))
    med = {k: statistics.median(v) for k, v in blocks.items()}
    paired = [b - a for a, b in zip(blocks["off"], blocks["on"])]
    stats = arms["on"].guard_stats()
    rec = {"mma": mma, "ms_per_step_blocks": {k: [round(x, 4) for x in v] for k, v in blocks.items()},
           "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
           "spread_ms": {k: round(max(v) - min(v), 4) for k, v in blocks.items()},
           "guard_cost_paired_ms": {"median": round(statistics.median(paired), 4), "min": round(min(paired), 4), "max": round(max(paired), 4)},
           "guard_cost_ms": round(med["on"] - med["off"], 4), "guard_cost_percent": round(100.0 * (med["on"] - med["off"]) / med["off"], 3),
           "last_guard_stats": {k: stats[k] for k in ("last_norm", "last_coef", "last_skipped", "skipped_total")},
           "optimiser_launches": kernel_times(arms["off"], arms["on"], args.kernel_reps)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "guarded_step.json"))
    ap.add_argument("--modes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16x6", "bf16"])
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, nargs=4, default=[128, 128, 64, 64])
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=40, help="untimed steps per arm before the first block")
    ap.add_argument("--blocks", type=int, default=8, help="A/B block pairs per mode")
    ap.add_argument("--steps", type=int, default=10, help="steps per block")
    ap.add_argument("--kernel-reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("guard_report needs a GPU", file=sys.stderr)
        return 2
    pkg.load_library()
    dev = torch.device("cuda:0")
    res = {"tool": "tools/guard_report.py", "device": torch.cuda.get_device_name(dev),
           "shape": {"rays": args.rays, "samples": args.samples, "layers": args.layers, "width": args.width},
           "method": f"A/B interleaved blocks of {args.steps} train steps between HIP events, {args.blocks} blocks per arm after {args.warmup} untimed steps per arm, "
                     "one model and batch; guard on = max_grad_norm 1.0 + skip_nonfinite; optimiser launches: one event pair per call",
           "modes": [measure(dev, m, args) for m in args.modes]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
