#!/usr/bin/env python3
"""Soak for intermittent errors (GPU box): the SAME headline-size training step -- same weights (lr 0), same rays, same random draws --
repeated N times per MMA mode.  The loss must repeat BIT FOR BIT (forward sweeps, compositing and the fixed-order loss reduction are
deterministic); every parameter gradient must repeat to the order of the weight-gradient atomics (fp32 atomic adds in varying order:
~1e-6 of the tensor's largest entry) -- an intermittent hazard of the kind round 4 found in the ring kernels' stores shows
as a 1e-2-size outlier.  With --deterministic the step runs with Model.set_deterministic(True) (ordered weight-gradient reduction) and
every gradient must repeat BIT FOR BIT as well.
Usage: python tools/soak_repeat.py [--repeats 40] [--modes f32,bf16x6,bf16] [--deterministic] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd.parallel import train_step  # noqa: E402
from reflect_sampling_nerf_amd.synthetic import synthetic_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--modes", default="f32,bf16x6,bf16")
    ap.add_argument("--json", default="")
    ap.add_argument("--deterministic", action="store_true", help="ordered weight-gradient reduction: demand bitwise-equal gradients")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    R = args.rays
    out = {"rays": R, "repeats": args.repeats, "deterministic": args.deterministic, "modes": {}}
    bad = 0
    for mode in args.modes.split(","):
        torch.manual_seed(0)
        cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=128, num_importance_samples=128, num_reflect_coarse_samples=64,
                                                num_reflect_importance_samples=64)
        model = cfg.setup(scene_box=None, num_train_data=1)
        with torch.no_grad():
            model.field.field_output_density.net.bias += 2.0
        model.to(dev).train()
        model.field.set_mma_mode(mode)
        model.set_deterministic(args.deterministic)
        o, d, pa = synthetic_rays(R, seed=0)
        rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.reshape(R, 1).to(dev),
                           nears=torch.full((R, 1), 2.0, device=dev), fars=torch.full((R, 1), 6.0, device=dev))
        batch = {"image": torch.rand(R, 3, generator=torch.Generator().manual_seed(1)).to(dev)}
        params = model.get_param_groups()["fields"]
        opt = pkg.FusedRAdam(params, lr=0.0, eps=1e-15)
        names = [n for n, _ in model.field.named_parameters()]
        ref_loss, ref_grads, worst, loss_flips, grad_flips = None, None, 0.0, 0, 0
        for k in range(args.repeats):
            torch.manual_seed(123)
            loss = train_step(model, rb, batch, opt, None, 100)
            torch.cuda.synchronize()
            bits = loss.detach().reshape(1).view(torch.int32).item()
            grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
            if ref_loss is None:
                ref_loss, ref_grads = bits, grads
                continue
            loss_flips += int(bits != ref_loss)
            for n, g, g0 in zip(names, grads, ref_grads):
                if g is None:
                    continue
                rel = float((g - g0).abs().max()) / max(float(g0.abs().max()), 1e-30)
                worst = max(worst, rel)
                grad_flips += int(not torch.equal(g, g0))
        rec = {"loss": float(torch.tensor([ref_loss], dtype=torch.int32).view(torch.float32)), "loss_bit_flips": loss_flips,
               "worst_gradient_deviation_rel_to_tensor_max": worst, "gradient_tensors_not_bitwise_equal": grad_flips}
        out["modes"][mode] = rec
        ok = loss_flips == 0 and (grad_flips == 0 if args.deterministic else worst <= 1e-4)
        bad += int(not ok)
        print(mode, json.dumps(rec), "ok" if ok else "DEVIATION", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
