"""trainer.train(resume=...): N steps, a save, a load and M more steps against N + M uninterrupted steps.  Deterministic mode: the same
bits everywhere (parameters, moments, generators, losses), across the 50-step loss warm-up boundary and across an intermediate save.
Default mode: the first resumed step's loss.  Also: settings taken from the checkpoint, a checkpoint as the reference's ns-train
writes it, the directory form and eval.  "Equal" is torch.equal throughout; nothing here has a tolerance."""
import math
import os

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import parallel, trainer
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager
from reflect_sampling_nerf_amd.train_ops import exponential_decay_lr
from tests.data_reference import camera_rays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ scene and runs
def _look_at(pos):
    back = pos / np.linalg.norm(pos)
    right = np.cross(np.array([0.0, 0.0, 1.0]), back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return np.concatenate([np.stack([right, up, back], 1), pos[:, None]], 1).astype(np.float32)


def _sphere_scene(n, H=48, W=48):
    """The Lambert sphere of test_data_gpu._sphere_scene (radius 0.8, white background) seen from a radius-4 shell."""
    k = np.arange(n) + 0.5
    z = np.clip(0.8 * (1 - 2 * k / (n + 1)), -0.8, 0.8)
    phi = k * math.pi * (3 - math.sqrt(5))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1)
    poses = np.stack([_look_at(4.0 * d) for d in dirs])
    focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    light = np.array([0.5, 0.8, 0.3]) / np.linalg.norm([0.5, 0.8, 0.3])
    base = np.array([0.85, 0.35, 0.25])
    ims = []
    for p in poses:
        o, d, _ = camera_rays(p.astype(np.float64), focal, focal, W / 2, H / 2, yy, xx)
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - 0.8 ** 2)
        t = -b - np.sqrt(np.clip(disc, 0, None))
        nrm = o + t[..., None] * d
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        shade = 0.25 + 0.75 * np.clip(nrm @ light, 0, None)
        ims.append(np.where((disc > 0)[..., None], shade[..., None] * base, 1.0))
    return BlenderScene.from_arrays(np.stack(ims), poses, focal=focal)


def _cfg(layers=4, width=64):
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=16, num_importance_samples=16, num_reflect_coarse_samples=8,
                                             num_reflect_importance_samples=8, base_mlp_num_layers=layers, base_mlp_layer_width=width)


class _Run:
    """One trainer.train call: its checkpoints (step -> file), per-step loss tensors and log lines."""

    def __init__(self, scene, out, layers=4, width=64, **kw):
        self.out, self.losses, self.logs = str(out), {}, []
        self.last = trainer.train(scene, self.out, device=DEV, model_config=_cfg(layers, width), log=self.logs.append, log_every=0,
                                  on_step=lambda step, loss: self.losses.__setitem__(step, loss.detach().clone()), **kw)

    def ckpt(self, step):
        return trainer.checkpoint_path(self.out, step)

    def saved_steps(self):
        return sorted(int(n[5:-5]) for n in os.listdir(self.out) if n.endswith(".ckpt"))


@pytest.fixture(scope="module")
def scene():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return _sphere_scene(6)


@pytest.fixture(scope="module")
def run_a(scene, tmp_path_factory):
    """Run A of the 4 x 64 fp32 case (56 deterministic steps, saves at 24, 48, 55): trained once, read by several tests."""
    return _Run(scene, tmp_path_factory.mktemp("a_f32"), steps=56, save_every=24, rays=96, mma="f32", seed=0, deterministic=True)


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def _state_tensors(ck):
    """Everything the bit-exact contract covers, by name."""
    out = {"pipeline/" + k: v for k, v in ck["pipeline"].items()}
    opt = ck["optimizers"]["fields"]
    for i, st in opt["state"].items():
        for k in ("exp_avg", "exp_avg_sq", "step"):
            out[f"optimizer/{i}/{k}"] = torch.as_tensor(st[k])
    out["run/cuda_rng_state"] = ck["rsn_run"]["cuda_rng_state"]
    out["run/cpu_rng_state"] = ck["rsn_run"]["cpu_rng_state"]
    return out


def _differing(path_a, path_b):
    a, b = _state_tensors(_load(path_a)), _state_tensors(_load(path_b))
    assert sorted(a) == sorted(b) and len([k for k in a if k.startswith("optimizer/")]) >= 3
    return [k for k in a if not torch.equal(a[k], b[k])]


def _strip_run_state(src, dst, edit=None):
    ck = _load(src)
    del ck["rsn_run"]
    if edit is not None:
        edit(ck)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    torch.save(ck, dst)
    return dst


# ------------------------------------------------------------------------------------------------ 1. bit-exact continuation
@pytest.mark.parametrize("layers,width,mma,rays,steps,save_every", [
    (4, 64, "f32", 96, 56, 24), (4, 64, "bf16x6", 96, 56, 24), (4, 64, "bf16", 96, 56, 24), (8, 256, "bf16x6", 64, 14, 6)])
def test_deterministic_resume_is_bit_exact(scene, run_a, tmp_path, layers, width, mma, rays, steps, save_every):
    """A: uninterrupted.  B: resumed from A's first save, passes A's second save point (writes it again) and ends.  C: resumed from A's
    second save (4 x 64: step 48, so it crosses step 50 where four loss coefficients switch on).  Every checkpoint two runs share is
    equal in every pipeline tensor, every moment and step count and both generator states; every loss two runs share is equal.
    D, the control: B's start with `rsn_run` removed, i.e. the generators NOT restored (same settings passed by hand) -- compared by
    the same function over the same tensors, its last checkpoint must differ from A's in pipeline tensors."""
    kw = dict(layers=layers, width=width, steps=steps, save_every=save_every)
    settings = dict(rays=rays, mma=mma, seed=0, deterministic=True)
    a = run_a if (layers, mma) == (4, "f32") else _Run(scene, tmp_path / "a", **kw, **settings)
    s1, s2, end = save_every, 2 * save_every, steps - 1
    assert a.saved_steps() == [s1, s2, end] and sorted(a.losses) == list(range(steps))
    b = _Run(scene, tmp_path / "b", resume=a.ckpt(s1), **kw)
    c = _Run(scene, tmp_path / "c", resume=a.ckpt(s2), **kw)
    assert b.saved_steps() == [s2, end] and sorted(b.losses) == list(range(s1 + 1, steps))
    assert c.saved_steps() == [end] and sorted(c.losses) == list(range(s2 + 1, steps))
    assert b.logs[0].startswith(f"train: resumed from {a.ckpt(s1)} at step {s1}") and b.last == b.ckpt(end)
    for r in (b, c):
        assert len(r.logs) == 1 + len(r.saved_steps()), r.logs  # nothing departed from the record, nothing was "not bit-exact"
        for step in r.saved_steps():
            assert _differing(a.ckpt(step), r.ckpt(step)) == [], f"checkpoint {step} of a run resumed at {min(r.losses) - 1}"
        for step, loss in r.losses.items():
            assert torch.equal(loss, a.losses[step]), f"loss of step {step} of a run resumed at {min(r.losses) - 1}"
    d = _Run(scene, tmp_path / "d", resume=_strip_run_state(a.ckpt(s1), str(tmp_path / "stripped" / f"step-{s1:09d}.ckpt")),
             **kw, **settings)
    diff = _differing(a.ckpt(end), d.ckpt(end))
    print(f"{layers} x {width} {mma}: without the generator restore {len(diff)} tensors of step {end} differ")
    assert any(k.startswith("pipeline/") for k in diff)
    assert not torch.equal(d.losses[s1 + 1], a.losses[s1 + 1])


# ------------------------------------------------------------------------------------------------ 2. default mode
def test_default_mode_first_resumed_step_is_exact(scene, tmp_path):
    """Atomic weight gradients: parameters differ from run to run, but a checkpoint holds exactly the parameters and generator state
    its run went on with, and forward plus loss have no order-dependent operation: step 25's loss repeats bit for bit."""
    a = _Run(scene, tmp_path / "a", steps=27, save_every=24, rays=96, mma="f32", seed=0, deterministic=False)
    b = _Run(scene, tmp_path / "b", steps=27, save_every=24, resume=a.ckpt(24))
    assert "deterministic False" in b.logs[0] and sorted(b.losses) == [25, 26]
    assert torch.equal(b.losses[25], a.losses[25])


# ------------------------------------------------------------------------------------------------ 3. settings
class _Spy:
    """parallel.train_step with a record of what the trainer handed it on the first call."""

    def __init__(self, monkeypatch):
        self.first = None
        inner = parallel.train_step

        def train_step(model, ray_bundle, batch, optimizer, reducer, step, **kw):
            if self.first is None:
                self.first = dict(model=model, step=step, rays=ray_bundle.origins.shape[0], indices=batch["indices"].clone(),
                                  lr=optimizer.current_lr(), step_count=optimizer.step_count, mma_mode=int(model.field.mma_mode),
                                  deterministic=model.deterministic, training=model.training)
            return inner(model, ray_bundle, batch, optimizer, reducer, step, **kw)

        monkeypatch.setattr(parallel, "train_step", train_step)


def test_settings_come_from_the_checkpoint(scene, tmp_path, monkeypatch):
    modes = type(trainer.make_model(_cfg()).field).MMA_MODES
    a = _Run(scene, tmp_path / "a", steps=6, save_every=3, rays=96, mma="bf16x6", seed=3, deterministic=True)
    spy = _Spy(monkeypatch)
    b = _Run(scene, tmp_path / "b", steps=6, save_every=3, resume=a.ckpt(3))
    f = spy.first
    assert (f["step"], f["step_count"], f["rays"], f["mma_mode"], f["deterministic"], f["training"]) == \
        (4, 4, 96, modes["bf16x6"], True, True)
    want = RayDataManager(scene, DEV, num_rays_per_batch=96, seed=3).next_train(4)[1]["indices"]
    other = RayDataManager(scene, DEV, num_rays_per_batch=96, seed=0).next_train(4)[1]["indices"]
    assert torch.equal(f["indices"], want) and not torch.equal(f["indices"], other)
    assert b.logs[0].endswith("steps 6 rays 96 mma bf16x6 seed 3 deterministic True") and len(b.logs) == 2
    assert _differing(a.ckpt(5), b.ckpt(5)) == []
    # an explicit value wins, and says so once
    spy.first = None
    c = _Run(scene, tmp_path / "c", steps=6, save_every=3, resume=a.ckpt(3), mma="f32")
    assert (spy.first["mma_mode"], spy.first["rays"], spy.first["deterministic"]) == (modes["f32"], 96, True)
    assert torch.equal(spy.first["indices"], want)
    noted = [s for s in c.logs if "mma" in s and "bf16x6" in s and "'f32'" in s]
    assert len(noted) == 1 and "not bit-exact" in noted[0] and c.logs.index(noted[0]) == 1
    assert c.logs[0].endswith("steps 6 rays 96 mma f32 seed 3 deterministic True")
    assert _load(c.ckpt(5))["rsn_run"]["mma"] == "f32"


# ------------------------------------------------------------------------------------------------ 4. foreign checkpoint
def test_foreign_checkpoint_resumes_at_the_schedulers_rate(scene, run_a, tmp_path, monkeypatch):
    """A step-24 checkpoint as the reference's trainer writes it: no `rsn_run`; the optimiser's `lr` is LambdaLR's decayed rate (after
    25 optimiser steps: that of step 25) and `initial_lr` the base rate."""
    def as_torch(ck):
        g = ck["optimizers"]["fields"]["param_groups"][0]
        g["initial_lr"], g["lr"] = 1e-3, exponential_decay_lr(25)

    src = _strip_run_state(run_a.ckpt(24), str(tmp_path / "ns" / "step-000000024.ckpt"), as_torch)
    assert set(_load(src)) == {"step", "pipeline", "optimizers", "scalers"}
    spy = _Spy(monkeypatch)
    r = _Run(scene, tmp_path / "out", steps=28, save_every=24, resume=src, rays=96, mma="f32", seed=0, deterministic=True)
    assert sorted(r.losses) == [25, 26, 27] and r.saved_steps() == [27] and r.last == r.ckpt(27)
    assert all(bool(torch.isfinite(v)) for v in r.losses.values())
    assert (spy.first["step"], spy.first["step_count"]) == (25, 25)
    assert spy.first["lr"] == exponential_decay_lr(25)
    assert len([s for s in r.logs if "not bit-exact" in s]) == 1
    assert "rsn_run" in _load(r.ckpt(27))  # what it writes is a checkpoint of this trainer again


# ------------------------------------------------------------------------------------------------ 5. directory form, eval
def test_run_directory_resumes_and_evaluates_its_latest(scene, run_a, tmp_path):
    with pytest.raises(ValueError, match=r"step 55\b.*steps is 56\b"):
        trainer.train(scene, str(tmp_path / "none"), steps=56, resume=run_a.out, device=DEV, model_config=_cfg(), log=None)
    assert not (tmp_path / "none").exists()
    r = _Run(scene, tmp_path / "more", steps=60, save_every=24, resume=run_a.out)
    assert r.logs[0].startswith(f"train: resumed from {run_a.ckpt(55)} at step 55") and sorted(r.losses) == [56, 57, 58, 59]
    assert r.saved_steps() == [59] and _load(r.ckpt(59))["step"] == 59
    assert _load(r.ckpt(59))["optimizers"]["fields"]["state"][0]["step"] == 60.0
    res = trainer.evaluate(scene, run_a.out, max_images=1, device=DEV, model_config=_cfg())
    assert res["checkpoint"] == run_a.ckpt(55) and res["step"] == 55 and len(res["per_image"]) == 1
    assert math.isfinite(res["results"]["psnr"])
