"""CPU-side checks of the deterministic-training switch: ABI 18 declares and binds the ordered weight-gradient entry points, the
workspace size is a host computation, and the switch reaches the Model, the environment and the trainer's command line."""
import ctypes as C
import os
import re
import subprocess
import sys

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, trainer
from reflect_sampling_nerf_amd._build import build_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rsn_weight_grad_workspace_bytes", "rsn_weight_grad_multi_dev_ordered", "rsn_weight_grad_jobs_ordered")


def _small_model():
    cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=4, base_mlp_layer_width=64)
    return cfg.setup(scene_box=None, num_train_data=1)


def test_abi_18_declares_and_binds_the_ordered_entry_points():
    assert _abi.RSN_ABI_VERSION == 18
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    assert re.search(r"#define\s+RSN_ABI_VERSION\s+18\b", header)
    declared = set(re.findall(r"\b(rsn_[a-z_0-9]+)\s*\(", header))
    build_library()
    lib = pkg.load_library()
    assert lib.rsn_abi_version() == 18
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/rsn.h"
        assert name in _abi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None, f"{name} is not bound"
    # the two ordered calls take the atomic calls' arguments plus (workspace, workspace_bytes) in front of the stream
    for name in ("rsn_weight_grad_multi_dev", "rsn_weight_grad_jobs"):
        old, new = _abi._SIGNATURES[name][1], _abi._SIGNATURES[name + "_ordered"][1]
        assert new == old[:-1] + [C.c_void_p, C.c_size_t, C.c_void_p]


def test_workspace_bytes_is_a_host_side_upper_bound():
    """4 slots of 192 + 2048 * NKB floats per workgroup, at most one workgroup per CU and job: no device is needed to ask, a larger
    problem never needs less, and bad arguments give 0 with a message."""
    build_library()
    lib = pkg.load_library()
    f = lib.rsn_weight_grad_workspace_bytes

    def bytes_for(lens, n_jobs, n_out, k_in, mode=0):
        return int(f(len(lens), (C.c_int64 * len(lens))(*lens), n_jobs, n_out, k_in, mode, 0))

    small, large = bytes_for([1000, 0, 37, 5003, 3], 1, 256, 256), bytes_for([10 ** 6], 1, 256, 256)
    slot = 4 * (192 + 2048 * 8) * 4
    assert 0 < small <= large and small % slot == 0 and large % slot == 0
    narrow = bytes_for([8], 1, 3, 40)  # one stage, NKB = 2: a few workgroups at the most
    assert 0 < narrow <= 4 * 4 * (192 + 2048 * 2) * 4 and narrow % (4 * (192 + 2048 * 2) * 4) == 0
    assert bytes_for([10 ** 6], 8, 256, 256) <= large  # the jobs share the CUs
    assert bytes_for([10 ** 6], 1, 256, 256, mode=1) >= slot
    assert bytes_for([100], 1, 300, 256) == 0 and b"n_out=300" in lib.rsn_last_error()
    assert bytes_for([100], 9, 256, 256) == 0 and bytes_for([-1], 1, 256, 256) == 0


def test_trainer_accepts_deterministic_flag():
    ap = trainer.build_parser()
    assert ap.parse_args(["train", "--data", "d", "--out", "o", "--deterministic"]).deterministic is True
    assert ap.parse_args(["train", "--data", "d", "--out", "o"]).deterministic is False


def test_model_set_deterministic_toggles_the_read_only_property(monkeypatch):
    monkeypatch.delenv("RSN_DETERMINISTIC", raising=False)
    model = _small_model()
    assert model.deterministic is False
    model.set_deterministic(True)
    assert model.deterministic is True
    model.set_deterministic(False)
    assert model.deterministic is False
    try:
        model.deterministic = True
    except AttributeError:
        pass
    else:
        raise AssertionError("Model.deterministic must be read-only (set_deterministic is the setter)")


def test_environment_variable_turns_the_default_on():
    code = ("import reflect_sampling_nerf_amd as pkg\n"
            "cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=4, base_mlp_layer_width=64)\n"
            "print('deterministic', cfg.setup(scene_box=None, num_train_data=1).deterministic)\n")
    for value, want in (("1", "True"), ("0", "False"), (None, "False")):
        env = {k: v for k, v in os.environ.items() if k != "RSN_DETERMINISTIC"}
        if value is not None:
            env["RSN_DETERMINISTIC"] = value
        res = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        assert f"deterministic {want}" in res.stdout, (value, res.stdout)
