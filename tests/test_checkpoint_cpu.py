"""checkpoint.py, the parts that need no GPU: the names the trainer re-exports are the module's own objects, open_checkpoint resolves,
loads and (only when asked) sets the matrix-core mode, and the tool modules import without the trainer."""
import os
import re
import subprocess
import sys

import pytest

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import checkpoint, trainer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("make_model", "checkpoint_path", "latest_checkpoint", "resolve_checkpoint", "make_run_state", "RUN_STATE_KEY",
         "RUN_STATE_VERSION", "save_checkpoint", "config_for_checkpoint", "_Pipeline", "_load_pipeline", "load_checkpoint",
         "open_checkpoint")


@pytest.mark.parametrize("name", MOVED)
def test_the_trainer_reexports_the_modules_own_objects(name):
    assert getattr(trainer, name) is getattr(checkpoint, name)
    assert getattr(checkpoint, name) is checkpoint.__dict__[name]
    if callable(getattr(checkpoint, name)):
        assert getattr(checkpoint, name).__module__ == checkpoint.__name__


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """step 3, step 12 and an unfinished save of step 20, of a 2 x 32 model."""
    run = tmp_path_factory.mktemp("run")
    cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=2, base_mlp_layer_width=32)
    model = checkpoint.make_model(cfg, seed=5)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    for step in (3, 12):
        checkpoint.save_checkpoint(checkpoint.checkpoint_path(str(run), step), model, opt, step)
    (run / "step-000000020.ckpt.tmp").write_bytes(b"")
    return run, model


@pytest.fixture
def mma_calls(monkeypatch, run_dir):
    calls = []
    monkeypatch.setattr(type(run_dir[1].field), "set_mma_mode", lambda self, mode: calls.append(mode))
    return calls


def test_open_checkpoint_takes_the_newest_finished_save_of_a_directory(run_dir, mma_calls):
    run, saved = run_dir
    path, model, step = checkpoint.open_checkpoint(str(run), device="cpu")
    assert (path, step) == (str(run / "step-000000012.ckpt"), 12)
    assert not model.training and len(model.field.mlp_base.layers) == 2 and model.field.mlp_base.layers[0].weight.shape[0] == 32
    want = saved.state_dict()
    got = model.state_dict()
    assert set(got) == set(want) and all(got[k].device.type == "cpu" and (got[k] == want[k]).all() for k in want)
    assert mma_calls == []  # mma=None leaves the mode alone
    path3, _, step3 = checkpoint.open_checkpoint(str(run / "step-000000003.ckpt"), device="cpu")  # a file is taken as it is
    assert (path3, step3) == (str(run / "step-000000003.ckpt"), 3)


def test_open_checkpoint_sets_the_mode_only_when_given_one(run_dir, mma_calls):
    checkpoint.open_checkpoint(str(run_dir[0]), None, "cpu", "bf16x6")
    assert mma_calls == ["bf16x6"]
    checkpoint.open_checkpoint(str(run_dir[0]), None, "cpu", None)
    assert mma_calls == ["bf16x6"]


def test_a_directory_without_checkpoints_is_the_same_error(tmp_path):
    (tmp_path / "step-000000001.ckpt.tmp").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="^" + re.escape(f"no step-*.ckpt in {tmp_path}") + "$"):
        checkpoint.open_checkpoint(str(tmp_path), device="cpu")


@pytest.mark.parametrize("module", ["mesh", "pointcloud", "render", "texture", "occupancy"])
def test_the_tool_modules_import_without_the_trainer(module):
    code = (f"import sys, reflect_sampling_nerf_amd.{module}; "
            "assert 'reflect_sampling_nerf_amd.checkpoint' in sys.modules; "
            "sys.exit(int('reflect_sampling_nerf_amd.trainer' in sys.modules))")
    assert subprocess.run([sys.executable, "-c", code], cwd=REPO).returncode == 0
