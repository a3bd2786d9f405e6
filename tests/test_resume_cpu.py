"""Resume, the parts that need no GPU: FusedRAdam.load_state_dict under a schedule (base rate from `initial_lr`, validation before any
change), the optional `rsn_run` checkpoint entry, latest_checkpoint, the argument check of train(resume=...) and the parser."""
import os

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import trainer
from reflect_sampling_nerf_amd.train_ops import exponential_decay_lr

SHAPES = [(5, 3), (7,), (2, 4)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]


def _scheduled_torch_radam(n_steps):
    """torch RAdam as the reference runs it: under LambdaLR with nerfstudio's ExponentialDecayScheduler (no warm-up) as the factor."""
    ps = _params()
    opt = torch.optim.RAdam(ps, lr=1e-3, eps=1e-15)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: (1e-4 / 1e-3) ** min(step / 50000.0, 1.0))
    g = torch.Generator().manual_seed(1)
    for _ in range(n_steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
        sched.step()
    return ps, opt, sched


def _scheduled_fused(seed=2):
    return pkg.FusedRAdam(_params(seed), lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)


def _snapshot(opt):
    return (opt.lr, opt.betas, opt.eps, opt.step_count, [m.clone() for m in opt.exp_avg], [v.clone() for v in opt.exp_avg_sq])


def _assert_untouched(opt, snap):
    lr, betas, eps, step_count, m0, v0 = snap
    assert (opt.lr, opt.betas, opt.eps, opt.step_count) == (lr, betas, eps, step_count)
    for a, b in zip(opt.exp_avg + opt.exp_avg_sq, m0 + v0):
        assert torch.equal(a, b)


def test_scheduled_torch_state_gives_the_schedulers_rate():
    """A torch RAdam stepped 37 times under LambdaLR: its state dict holds the decayed rate in `lr` and the base rate in `initial_lr`.
    A scheduled FusedRAdam that loaded it is at the scheduler's rate, not at a rate decayed twice."""
    n = 37
    _, ref, sched = _scheduled_torch_radam(n)
    sd = ref.state_dict()
    assert sd["param_groups"][0]["initial_lr"] == 1e-3 and sd["param_groups"][0]["lr"] < 1e-3
    mine = _scheduled_fused()
    mine.load_state_dict(sd)
    want = sched.get_last_lr()[0]
    assert mine.step_count == n and mine.lr == 1e-3
    assert abs(mine.current_lr() - want) <= 1e-12 * want, (mine.current_lr(), want)
    assert abs(want - exponential_decay_lr(n)) <= 1e-12 * want
    for k in range(len(SHAPES)):
        assert torch.equal(mine.exp_avg[k], sd["state"][k]["exp_avg"]) and torch.equal(mine.exp_avg_sq[k], sd["state"][k]["exp_avg_sq"])


def test_unscheduled_optimiser_still_takes_lr():
    _, ref, _ = _scheduled_torch_radam(5)
    mine = pkg.FusedRAdam(_params(2), lr=5e-2, eps=1e-15)
    mine.load_state_dict(ref.state_dict())
    assert mine.lr == ref.state_dict()["param_groups"][0]["lr"] == mine.current_lr()


@pytest.mark.parametrize("defect", ["shape", "shape_sq", "steps", "weight_decay", "count"])
def test_rejected_state_dict_changes_nothing(defect):
    _, ref, _ = _scheduled_torch_radam(9)
    sd = ref.state_dict()
    sd["param_groups"][0]["betas"] = (0.8, 0.99)  # would be taken over if the load went through
    sd["param_groups"][0]["eps"] = 1e-7
    if defect == "shape":  # the LAST parameter: everything before it is valid
        sd["state"][2]["exp_avg"] = torch.zeros(4, 2)
    elif defect == "shape_sq":
        sd["state"][2]["exp_avg_sq"] = torch.zeros(8)
    elif defect == "steps":
        sd["state"][2]["step"] = torch.tensor(4.0)
    elif defect == "weight_decay":
        sd["param_groups"][0]["weight_decay"] = 0.01
    else:
        sd["param_groups"][0]["params"] = [0, 1]
    mine = _scheduled_fused()
    for p in mine.params:  # non-trivial moments and step count to protect
        p.grad = torch.ones_like(p)
    mine.exp_avg = [torch.full_like(p, 0.5) for p in mine.params]
    mine.exp_avg_sq = [torch.full_like(p, 0.25) for p in mine.params]
    mine.step_count = 3
    snap = _snapshot(mine)
    with pytest.raises(ValueError):
        mine.load_state_dict(sd)
    _assert_untouched(mine, snap)


def test_own_scheduled_state_round_trips():
    src = _scheduled_fused()
    src.step_count = 1234
    src.exp_avg = [torch.full_like(p, 0.5) for p in src.params]
    src.exp_avg_sq = [torch.full_like(p, 0.25) for p in src.params]
    sd = src.state_dict()
    assert "initial_lr" not in sd["param_groups"][0] and sd["param_groups"][0]["lr"] == 1e-3
    dst = _scheduled_fused(seed=5)
    dst.load_state_dict(sd)
    assert dst.step_count == 1234 and dst.current_lr() == src.current_lr() == exponential_decay_lr(1234)
    assert all(torch.equal(a, b) for a, b in zip(dst.exp_avg + dst.exp_avg_sq, src.exp_avg + src.exp_avg_sq))


# ------------------------------------------------------------------------------------------------ checkpoints
def _small_cfg():
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=8, num_importance_samples=8, num_reflect_coarse_samples=4,
                                             num_reflect_importance_samples=4, base_mlp_num_layers=4, base_mlp_layer_width=64)


def _save(tmp_path, step, run_state=None):
    model = trainer.make_model(_small_cfg(), seed=3)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)
    return trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path), step), model, opt, step, run_state=run_state)


def test_run_state_is_a_fifth_key_only_when_given(tmp_path):
    torch.manual_seed(11)
    cpu_state = torch.get_rng_state()
    rs = trainer.make_run_state(seed=4, rays=96, mma="bf16x6", deterministic=True, device="cpu")
    ck = torch.load(_save(tmp_path, 7, rs), map_location="cpu", weights_only=False)
    assert set(ck) == {"step", "pipeline", "optimizers", "scalers", "rsn_run"}
    run = ck["rsn_run"]
    assert set(run) == {"version", "seed", "rays", "mma", "deterministic", "cuda_rng_state", "cpu_rng_state"}
    assert (run["version"], run["seed"], run["rays"], run["mma"], run["deterministic"]) == (trainer.RUN_STATE_VERSION, 4, 96, "bf16x6", True)
    assert torch.equal(run["cpu_rng_state"], cpu_state) and run["cuda_rng_state"] is None  # no CUDA device asked for
    assert "rsn_run" not in torch.load(_save(tmp_path, 8), map_location="cpu", weights_only=False)


def test_latest_checkpoint(tmp_path):
    with pytest.raises(FileNotFoundError):
        trainer.latest_checkpoint(str(tmp_path))
    for name in ("step-000000900.ckpt", "step-000001000.ckpt", "step-000000024.ckpt", "step-000002000.ckpt.tmp", "notes.txt",
                 "step-000003000.ckpt.bak", "step-best.ckpt", "xstep-000009000.ckpt"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "step-000005000.ckpt.d").mkdir()
    assert trainer.latest_checkpoint(str(tmp_path)) == str(tmp_path / "step-000001000.ckpt")
    assert trainer.resolve_checkpoint(str(tmp_path)) == str(tmp_path / "step-000001000.ckpt")
    assert trainer.resolve_checkpoint(str(tmp_path / "step-000000024.ckpt")) == str(tmp_path / "step-000000024.ckpt")
    only_tmp = tmp_path / "sub"
    only_tmp.mkdir()
    (only_tmp / "step-000000001.ckpt.tmp").write_bytes(b"")
    with pytest.raises(FileNotFoundError):
        trainer.latest_checkpoint(str(only_tmp))


@pytest.mark.parametrize("steps", [8, 5, 1])
def test_resume_with_nothing_left_to_train_is_an_error(tmp_path, steps):
    """A checkpoint of step 7 and steps <= 8: the last step of the run is steps - 1 <= 7.  Raised before any device work (device and
    scene are never looked at), for the file and for its directory, naming both numbers."""
    path = _save(tmp_path, 7)
    for where in (path, str(tmp_path)):
        with pytest.raises(ValueError, match=rf"step 7\b.*steps is {steps}\b"):
            trainer.train(None, str(tmp_path / "out"), steps=steps, model_config=_small_cfg(), device="no-such-device", log=None,
                          resume=where)
    assert not (tmp_path / "out").exists()


def test_parser_resume_and_directory_checkpoint(tmp_path):
    ap = trainer.build_parser()
    a = ap.parse_args(["train", "--data", "D", "--out", "O", "--resume", "RUN/step-000001000.ckpt"])
    assert a.resume == "RUN/step-000001000.ckpt"
    d = ap.parse_args(["train", "--data", "D", "--out", "O"])
    assert d.resume is None and (d.rays, d.mma, d.seed, d.deterministic) == (1024, "f32", 0, False)
    assert ap.parse_args(["eval", "--data", "D", "--ckpt", str(tmp_path)]).ckpt == str(tmp_path)
    # what main() hands to train(): None where the user typed nothing, so that a resumed run's checkpoint decides
    given = trainer.build_parser(run_defaults=False)
    g = given.parse_args(["train", "--data", "D", "--out", "O", "--resume", "R", "--mma", "bf16"])
    assert (g.rays, g.mma, g.seed, g.resume) == (None, "bf16", None, "R")
    g = given.parse_args(["train", "--data", "D", "--out", "O", "--rays", "1024", "--seed", "0"])
    assert (g.rays, g.mma, g.seed) == (1024, None, 0)


def test_run_settings_resolution():
    """given > recorded > fresh-run default; one line per departure from the record."""
    rec = {"rays": 96, "mma": "bf16x6", "seed": 3, "deterministic": True}
    none = dict.fromkeys(rec)
    assert trainer._resolve_run_settings(none, rec) == (rec, [])
    assert trainer._resolve_run_settings(none, None) == ({"rays": 1024, "mma": "f32", "seed": 0, "deterministic": None}, [])
    got, notes = trainer._resolve_run_settings({"rays": 96, "mma": "f32", "seed": None, "deterministic": False}, rec)
    assert got == {"rays": 96, "mma": "f32", "seed": 3, "deterministic": False}
    assert len(notes) == 2 and "mma" in notes[0] and "bf16x6" in notes[0] and "deterministic" in notes[1]
