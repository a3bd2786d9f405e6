"""CPU checks of the standalone data path: the Blender parser, the host restatements the GPU tests compare against
(Philox4x32-10 known answers, the ray recipe), the trainer's checkpoint layout and its command line."""
import json
import math
import os

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import trainer
from reflect_sampling_nerf_amd.data import BlenderScene, load_blender_split
from tests.data_reference import camera_rays, philox4x32_10, sample_indices

ANGLE_X = 0.6911112070083618  # the NeRF-synthetic scenes' camera_angle_x


def _pose(k):
    c, s = math.cos(0.3 * k), math.sin(0.3 * k)
    return [[c, 0.0, s, 1.5 * k], [0.0, 1.0, 0.0, -2.0], [-s, 0.0, c, 4.0 + k], [0.0, 0.0, 0.0, 1.0]]


def _write_scene(root, H=6, W=9):
    from PIL import Image

    rng = np.random.default_rng(0)
    want = {}
    for split, n in (("train", 3), ("test", 2)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames, ims = [], []
        for k in range(n):
            im = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
            Image.fromarray(im, "RGBA").save(os.path.join(root, split, f"r_{k}.png"))
            frames.append({"file_path": f"./{split}/r_{k}", "rotation": 0.0, "transform_matrix": _pose(k)})
            ims.append(im)
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as fh:
            json.dump({"camera_angle_x": ANGLE_X, "frames": frames}, fh)
        want[split] = (np.stack(ims), np.array([_pose(k) for k in range(n)], dtype=np.float32))
    return want


def test_blender_parser_pixels_intrinsics_and_scaled_poses(tmp_path):
    want = _write_scene(str(tmp_path))
    for split in ("train", "test"):
        sc = load_blender_split(str(tmp_path), split, scale_factor=0.5)
        ims, poses = want[split]
        assert sc.images.dtype == np.uint8 and np.array_equal(sc.images, ims)
        focal = 0.5 * 9 / math.tan(0.5 * ANGLE_X)
        assert sc.fx == pytest.approx(focal, rel=1e-12) and sc.fy == pytest.approx(focal, rel=1e-12)
        assert (sc.cx, sc.cy) == (4.5, 3.0)
        assert sc.c2w.shape == (len(ims), 3, 4) and sc.c2w.dtype == np.float32
        assert np.array_equal(sc.c2w[:, :, :3], poses[:, :3, :3])
        assert np.array_equal(sc.c2w[:, :, 3], poses[:, :3, 3] * np.float32(0.5))
        assert (sc.num_images, sc.height, sc.width) == (len(ims), 6, 9)


def test_blender_parser_rgb_sources_get_opaque_alpha(tmp_path):
    from PIL import Image

    os.makedirs(tmp_path / "train")
    rgb = np.random.default_rng(1).integers(0, 256, size=(6, 9, 3), dtype=np.uint8)
    Image.fromarray(rgb, "RGB").save(tmp_path / "train" / "a.png")
    (tmp_path / "transforms_train.json").write_text(json.dumps(
        {"camera_angle_x": ANGLE_X, "frames": [{"file_path": "./train/a", "transform_matrix": _pose(0)}]}))
    sc = load_blender_split(str(tmp_path), "train")
    assert np.array_equal(sc.images[0, :, :, :3], rgb) and (sc.images[0, :, :, 3] == 255).all()


def test_blender_parser_errors(tmp_path):
    _write_scene(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="transforms_val.json"):
        load_blender_split(str(tmp_path), "val")
    os.remove(tmp_path / "test" / "r_1.png")
    with pytest.raises(FileNotFoundError, match="r_1.png"):
        load_blender_split(str(tmp_path), "test")
    from PIL import Image

    Image.fromarray(np.zeros((7, 9, 4), np.uint8), "RGBA").save(tmp_path / "train" / "r_2.png")
    with pytest.raises(ValueError, match="differs"):
        load_blender_split(str(tmp_path), "train")


def test_from_arrays():
    ims = np.random.default_rng(2).random((2, 5, 7, 3))
    poses = np.array([_pose(0), _pose(1)], dtype=np.float32)
    sc = BlenderScene.from_arrays(ims, poses, focal=6.0)
    assert sc.images.shape == (2, 5, 7, 4) and sc.images.dtype == np.uint8 and (sc.images[..., 3] == 255).all()
    assert np.array_equal(sc.images[..., :3], np.rint(ims * 255).astype(np.uint8))
    assert sc.c2w.shape == (2, 3, 4) and (sc.fx, sc.fy, sc.cx, sc.cy) == (6.0, 6.0, 3.5, 2.5)
    with pytest.raises(ValueError):
        BlenderScene.from_arrays(ims, poses[:1], focal=6.0)


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_restatement_known_answers(ctr, key, out):
    """Random123's kat_vectors for philox4x32_10."""
    assert tuple(int(v) for v in philox4x32_10(np.array(ctr, dtype=np.uint64), key)) == out


def test_sample_indices_restatement_in_range():
    idx = sample_indices(3, 5, 7, 4096, seed=1, rank=0, step=0)
    assert idx.min(0).tolist() == [0, 0, 0] and idx.max(0).tolist() == [2, 4, 6]
    assert not np.array_equal(idx, sample_indices(3, 5, 7, 4096, seed=1, rank=0, step=1))


def test_ray_restatement_principal_point():
    fx, fy = 40.0, 30.0
    o, d, area = camera_rays(np.eye(4)[:3], fx, fy, 9.5, 7.5, 7.0, 9.0)  # pixel centre (9.5, 7.5) = principal point
    assert np.allclose(o, 0.0) and np.allclose(d, [0.0, 0.0, -1.0], atol=1e-15)
    assert area == pytest.approx(1.0 / (fx * fy), rel=2e-3)
    # a rotated, translated camera: the direction rotates with it, the area does not change
    c, s = math.cos(0.7), math.sin(0.7)
    c2w = np.array([[c, -s, 0, 1.0], [s, c, 0, 2.0], [0, 0, 1, 3.0]])
    o2, d2, area2 = camera_rays(c2w, fx, fy, 9.5, 7.5, 3.0, 12.0)
    o1, d1, area1 = camera_rays(np.eye(4)[:3], fx, fy, 9.5, 7.5, 3.0, 12.0)
    assert np.allclose(o2, [1.0, 2.0, 3.0]) and np.allclose(d2, c2w[:, :3] @ d1) and area2 == pytest.approx(area1, rel=1e-12)


def _small_cfg():
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=8, num_importance_samples=8, num_reflect_coarse_samples=4,
                                             num_reflect_importance_samples=4, base_mlp_num_layers=4, base_mlp_layer_width=64)


def test_checkpoint_layout_loads_strictly(tmp_path):
    model = trainer.make_model(_small_cfg(), seed=3)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.25)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)
    path = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path), 7), model, opt, 7)
    assert os.path.basename(path) == "step-000000007.ckpt"
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"step", "pipeline", "optimizers", "scalers"} and ck["step"] == 7 and ck["scalers"] == {}
    assert set(ck["pipeline"]) == {"_model." + k for k in model.state_dict()}
    assert set(ck["optimizers"]) == {"fields"} and set(ck["optimizers"]["fields"]) == {"state", "param_groups"}

    class Pipe(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._model = trainer.make_model(_small_cfg(), seed=4)

    dst = Pipe()
    res = dst.load_state_dict(ck["pipeline"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (n, a), (_, b) in zip(model.named_parameters(), dst._model.named_parameters()):
        assert torch.equal(a, b), n
    # the trainer's own loader: depth and width read off the checkpoint, strict
    cfg = trainer.config_for_checkpoint(ck["pipeline"])
    assert (cfg.base_mlp_num_layers, cfg.base_mlp_layer_width) == (4, 64)
    loaded, step = trainer.load_checkpoint(path, _small_cfg(), device="cpu")
    assert step == 7 and not loaded.training
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), loaded.parameters()))


def test_cli_parser_accepts_documented_flags():
    ap = trainer.build_parser()
    a = ap.parse_args(["train", "--data", "D", "--out", "O", "--steps", "5", "--rays", "4096", "--mma", "bf16",
                       "--save-every", "2", "--log-every", "1", "--seed", "9"])
    assert (a.command, a.data, a.out, a.steps, a.rays, a.mma, a.save_every, a.log_every, a.seed) == \
        ("train", "D", "O", 5, 4096, "bf16", 2, 1, 9)
    d = ap.parse_args(["train", "--data", "D", "--out", "O"])
    assert (d.rays, d.mma, d.save_every, d.log_every, d.seed) == (1024, "f32", 1000, 100, 0)
    for m in ("f32", "bf16x6", "bf16"):
        assert ap.parse_args(["train", "--data", "D", "--out", "O", "--mma", m]).mma == m
    e = ap.parse_args(["eval", "--data", "D", "--ckpt", "C", "--split", "val", "--max-images", "3", "--out", "m.json",
                       "--save-images", "I"])
    assert (e.command, e.data, e.ckpt, e.split, e.max_images, e.out, e.save_images) == \
        ("eval", "D", "C", "val", 3, "m.json", "I")
    assert ap.parse_args(["eval", "--data", "D", "--ckpt", "C"]).split == "test"
    with pytest.raises(SystemExit):
        ap.parse_args(["train", "--data", "D", "--out", "O", "--mma", "fp16"])
