"""Guarded optimiser step, the parts that need no GPU: the additive ABI (still version 18), the trainer's two settings through the
parser, the resume rule and the checkpoint entry, FusedRAdam's constructor on CPU parameters, and the reference's clip factor
against torch.nn.utils.clip_grad_norm_."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, train_ops, trainer
from reflect_sampling_nerf_amd._build import build_library
from tests import guard_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rsn_grad_sumsq_workspace_bytes", "rsn_grad_sumsq", "rsn_radam_step_guarded")


def test_abi_is_additive_and_still_version_18():
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    declared = set(re.findall(r"\b(rsn_[a-z_0-9]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _abi.EXPORTED_SYMBOLS, name
    assert "typedef struct rsn_guard_stats" in header and re.search(r"#define RSN_ABI_VERSION 18\b", header)
    build_library()
    lib = pkg.load_library()
    assert lib.rsn_abi_version() == _abi.RSN_ABI_VERSION == 18
    # the struct of the binding is the header's: 6 words, then 2 x 48 doubles
    assert C.sizeof(_abi.GuardStats) == 24 + 2 * 48 * 8 and _abi.GuardStats.per_tensor_sq.offset == 24
    assert f"#define RSN_GUARD_MAX_TENSORS {_abi.RSN_GUARD_MAX_TENSORS}\n" in header
    # argument errors are answered before any launch
    sizes = (C.c_int32 * 2)(5, 7)
    assert lib.rsn_grad_sumsq_workspace_bytes(2, sizes) == 2 * train_ops.GUARD_SLOTS * 8
    assert lib.rsn_grad_sumsq_workspace_bytes(49, sizes) == 0 and b"n_tensors=49" in lib.rsn_last_error()
    assert lib.rsn_grad_sumsq(2, None, sizes, None, 0, None) == -1
    assert lib.rsn_radam_step_guarded(2, None, None, None, None, sizes, 1, 1e-3, 0.9, 0.999, 1e-15, 1.0, 1, None, 0, None, None) == -1


def test_python_grid_constants_are_the_kernels():
    src = open(os.path.join(REPO, "reflect_sampling_nerf_amd", "csrc", "rsn_train_ops.hip")).read()
    got = {k: int(v) for k, v in re.findall(r"^#define (GUARD_THREADS|GUARD_VEC|GUARD_SLOTS) (\d+)\b", src, flags=re.M)}
    assert got == {"GUARD_THREADS": train_ops.GUARD_THREADS, "GUARD_VEC": train_ops.GUARD_VEC, "GUARD_SLOTS": train_ops.GUARD_SLOTS}
    assert re.search(r"^#define RADAM_MAX_TENSORS 48\b", src, flags=re.M) and _abi.RSN_GUARD_MAX_TENSORS == 48


def test_parser_and_run_settings_round_trip():
    base = ["train", "--data", "D", "--out", "O"]
    for ap in (trainer.build_parser(), trainer.build_parser(run_defaults=False)):
        a = ap.parse_args(base)
        assert a.max_grad_norm is None and a.skip_nonfinite is False
        a = ap.parse_args(base + ["--max-grad-norm", "0.5", "--skip-nonfinite"])
        assert a.max_grad_norm == 0.5 and a.skip_nonfinite is True
    none = dict.fromkeys(("rays", "mma", "seed", "deterministic", "max_grad_norm", "skip_nonfinite"))
    fresh, notes = trainer._resolve_run_settings(none, None)
    assert (fresh["max_grad_norm"], fresh["skip_nonfinite"], notes) == (None, None, [])
    rec = trainer.make_run_state(seed=3, rays=96, mma="f32", deterministic=True, device="cpu", max_grad_norm=0.5, skip_nonfinite=True)
    got, notes = trainer._resolve_run_settings(none, rec)  # --resume without restating them
    assert (got["max_grad_norm"], got["skip_nonfinite"], got["rays"], notes) == (0.5, True, 96, [])
    got, notes = trainer._resolve_run_settings({**none, "max_grad_norm": 2.0}, rec)  # a given value wins and says so
    assert got["max_grad_norm"] == 2.0 and got["skip_nonfinite"] is True and len(notes) == 1 and "max_grad_norm" in notes[0]
    unguarded = trainer.make_run_state(seed=3, rays=96, mma="f32", deterministic=True, device="cpu")
    got, notes = trainer._resolve_run_settings({**none, "skip_nonfinite": True}, unguarded)
    assert (got["max_grad_norm"], got["skip_nonfinite"], notes) == (None, True, [])


def test_run_state_of_an_unguarded_run_keeps_its_keys():
    keys = {"version", "seed", "rays", "mma", "deterministic", "cuda_rng_state", "cpu_rng_state"}
    assert set(trainer.make_run_state(seed=0, rays=8, mma="f32", deterministic=False, device="cpu")) == keys
    assert set(trainer.make_run_state(0, 8, "f32", False, "cpu", max_grad_norm=None, skip_nonfinite=False)) == keys
    rs = trainer.make_run_state(0, 8, "f32", False, "cpu", max_grad_norm=1.5)
    assert set(rs) == keys | {"max_grad_norm"} and rs["max_grad_norm"] == 1.5 and rs["version"] == trainer.RUN_STATE_VERSION == 1
    assert set(trainer.make_run_state(0, 8, "f32", False, "cpu", skip_nonfinite=True)) == keys | {"skip_nonfinite"}


def test_guarded_optimiser_constructs_on_cpu_parameters():
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(4, 3, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g))]
    plain = pkg.FusedRAdam(ps, lr=1e-3, eps=1e-15)
    guarded = pkg.FusedRAdam(ps, lr=1e-3, eps=1e-15, max_grad_norm=1.0, skip_nonfinite=True, names=["a", "b"])
    assert guarded.guarded and not plain.guarded and guarded.names == ["a", "b"]
    assert guarded.guard_stats() is None  # nothing was allocated, nothing is read
    for opt in (plain, guarded):
        opt.step_count = 3
    a, b = plain.state_dict(), guarded.state_dict()
    assert a["param_groups"] == b["param_groups"] and sorted(a["state"]) == sorted(b["state"])
    for i in a["state"]:
        assert sorted(a["state"][i]) == sorted(b["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        assert all(torch.equal(torch.as_tensor(a["state"][i][k]), torch.as_tensor(b["state"][i][k])) for k in a["state"][i])
    assert pkg.FusedRAdam(ps, max_grad_norm=float("inf")).guarded
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            pkg.FusedRAdam(ps, max_grad_norm=bad)
    with pytest.raises(ValueError):
        pkg.FusedRAdam(ps, names=["only one"])


def test_guard_log_line():
    stats = {"last_norm": 12.5, "last_coef": 0.08, "last_skipped": False, "skipped_total": 2, "last_skipped_step": 10,
             "nonfinite_at_last_skip": ["field.mlp_base.layers.0.weight"]}
    line = trainer._guard_log(stats, 1)
    assert "gnorm 1.2500e+01 clip 0.08 skipped 2" in line and "step 9: non-finite gradients in field.mlp_base.layers.0.weight" in line
    assert "non-finite" not in trainer._guard_log(stats, 2)


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e3])
def test_reference_coefficient_is_clip_grad_norms(max_norm):
    g = torch.Generator().manual_seed(7)
    ps = [torch.nn.Parameter(torch.zeros(*s)) for s in ((17, 9), (33,), (256, 99), (1,))]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g) * 0.05
    before = [p.grad.clone() for p in ps]
    sq = ref.sumsq_fp64([p.grad for p in ps])
    coef = ref.clip_coef(ref.norm_fp32(sq), max_norm)
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    want = float(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    assert abs(float(ref.norm_fp32(sq)) - float(total)) <= 4 * np.spacing(np.float32(total))  # torch's norm is an fp32 sum
    assert abs(float(coef) - want) <= 1e-6 * want
    assert (want == 1.0) == (max_norm == 1e3)
    for p, b in zip(ps, before):  # and torch did scale by that factor
        assert torch.allclose(p.grad, b * want, rtol=1e-6, atol=0)
    assert ref.clip_coef(np.float32(np.nan), 1.0) != ref.clip_coef(np.float32(np.nan), 1.0)  # NaN stays NaN, as torch's clamp
    assert ref.clip_coef(np.float32(np.inf), 1.0) == 0.0 and ref.clip_coef(np.float32(5.0), None) == 1.0
