"""Depth supervision without a GPU: the loader's depth files, the float64 references of tests/depth_reference.py against finite
differences and float64 autograd, the mutations the GPU tests must be able to see, and the host side of the feature -- ABI, argument
errors (no launch), names and switches, the loss dictionary's refusal to drop the term, the trainer's flags and run state."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, parallel, train_graph, train_ops, trainer
from reflect_sampling_nerf_amd._build import build_library
from reflect_sampling_nerf_amd.data import BlenderScene, load_nerfstudio_split
from tests import capture_reference as cr
from tests import depth_reference as dz

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


# ------------------------------------------------------------------------------------------------------------- loader
H, W, N = 6, 8, 4


def _raw_depths(seed=0):
    """uint16 [N,H,W] with zeros (no measurement) in it."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(300, 5000, size=(N, H, W)).astype(np.uint16)
    raw[:, 0, 0] = 0
    raw[1, 2, 3] = 65535
    return raw


def _capture(root, raw=None, kind="png", folder="depths", keys=range(N), extra_dirs=(), raw_f=None):
    """A four-frame capture with depth files of `kind` under `folder`/ for the frames in `keys`."""
    from PIL import Image

    rng = np.random.default_rng(5)
    images = rng.integers(0, 255, size=(N, H, W, 3)).astype(np.uint8)
    rows = [cr.camera_row(W, H, coeffs=(0.0,) * 5) for _ in range(N)]
    poses = cr.shell_poses(N)
    raw = _raw_depths() if raw is None else raw
    frame_extra = {}
    os.makedirs(os.path.join(root, folder), exist_ok=True)
    for i in keys:
        name = f"{folder}/frame_{i:05d}.{kind}"
        if kind == "png":
            Image.fromarray(raw[i]).save(os.path.join(root, name))
        elif kind == "tiff":  # a container that keeps Pillow's 32-bit integer mode "I"
            Image.fromarray(raw[i].astype(np.int32)).save(os.path.join(root, name))
        else:
            np.save(os.path.join(root, name), raw[i].astype(np.float32) if raw_f is None else raw_f[i])
        frame_extra[i] = {"depth_file_path": name}
    cr.write_capture(root, images, poses, rows, frame_extra=frame_extra)
    for d in extra_dirs:
        os.makedirs(os.path.join(root, d), exist_ok=True)
    return raw


ALL = dict(eval_mode="all")  # every frame in the split: the order of the frames is the order of the files


def test_png_and_npy_give_the_same_array_and_the_scales_compose(tmp_path):
    """A 16-bit PNG (Pillow mode I;16) and a float .npy of the same numbers load to the same bits; the stored value is
    float32(raw * depth_unit_scale * s) with s the factor the translations got, the product formed in float64."""
    raw = _capture(str(tmp_path / "png"))
    _capture(str(tmp_path / "npy"), kind="npy")
    for unit, scale_factor, auto in ((1e-3, 1.0, True), (0.25e-3, 0.7, True), (1e-3, 2.5, False)):
        kw = dict(depths=True, depth_unit_scale=unit, scale_factor=scale_factor, auto_scale=auto, **ALL)
        a = load_nerfstudio_split(str(tmp_path / "png"), "train", **kw)
        b = load_nerfstudio_split(str(tmp_path / "npy"), "train", **kw)
        assert a.depths.dtype == np.float32 and a.depths.shape == (N, H, W) and np.array_equal(a.depths, b.depths)
        plain = load_nerfstudio_split(str(tmp_path / "png"), "train", scale_factor=scale_factor, auto_scale=auto, **ALL)
        s = a.dataparser_scale
        assert s == plain.dataparser_scale and (auto or s == scale_factor)
        assert np.array_equal(a.depths, (raw.astype(np.float64) * unit * s).astype(np.float32))
        assert float(a.depths[0, 0, 0]) == 0.0 and float(a.depths[1, 2, 3]) == np.float32(65535.0 * unit * s)
        # the poses got the same factor: the depth of a point and the camera's distance from it stay in proportion
        assert np.array_equal(a.c2w, plain.c2w)
    train = load_nerfstudio_split(str(tmp_path / "png"), "train", depths=True)  # a proper split keeps the frames' own maps
    keep = cr.split_indices(N)[0]
    assert np.array_equal(train.depths, (raw[keep].astype(np.float64) * 1e-3 * train.dataparser_scale).astype(np.float32))


def test_mode_I_png_is_read(tmp_path):
    from PIL import Image

    raw = _capture(str(tmp_path), kind="tiff")
    with Image.open(str(tmp_path / "depths/frame_00000.tiff")) as img:
        assert img.mode == "I"
    a = load_nerfstudio_split(str(tmp_path), "train", depths=True, **ALL)
    assert np.array_equal(a.depths, (raw.astype(np.float64) * 1e-3 * a.dataparser_scale).astype(np.float32))


def test_depths_false_loads_a_capture_with_depth_keys_exactly_as_before(tmp_path):
    """The default ignores the key: the same scene as from the same capture without any depth_file_path, and no file is opened (the
    depth files are deleted before the load)."""
    _capture(str(tmp_path / "with"))
    _capture(str(tmp_path / "without"), keys=())
    for name in os.listdir(str(tmp_path / "with" / "depths")):
        os.remove(str(tmp_path / "with" / "depths" / name))
    a = load_nerfstudio_split(str(tmp_path / "with"), "train", **ALL)
    b = load_nerfstudio_split(str(tmp_path / "without"), "train", **ALL)
    assert a.depths is None and b.depths is None
    for f in ("images", "c2w", "cameras", "dataparser_transform"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.fx, a.fy, a.cx, a.cy, a.dataparser_scale, a.file_paths, a.masks) == (b.fx, b.fy, b.cx, b.cy, b.dataparser_scale, b.file_paths, b.masks)
    none = load_nerfstudio_split(str(tmp_path / "without"), "train", depths=True, **ALL)  # asked for, and no frame has one
    assert none.depths is None


def test_downscaled_sets_read_depths_K(tmp_path):
    """downscale_factor = 2 reads depths_2/ (nerfstudio's folder rule, as for images_2/): nothing is resampled."""
    from PIL import Image

    root = str(tmp_path)
    _capture(root)
    small = np.random.default_rng(3).integers(1, 4000, size=(N, H // 2, W // 2)).astype(np.uint16)
    os.makedirs(os.path.join(root, "images_2"))
    for i in range(N):
        Image.fromarray(np.zeros((H // 2, W // 2, 3), np.uint8)).save(os.path.join(root, f"images_2/frame_{i:05d}.png"))
    with pytest.raises(FileNotFoundError, match="depths_2"):
        load_nerfstudio_split(root, "train", depths=True, downscale_factor=2, **ALL)
    os.makedirs(os.path.join(root, "depths_2"))
    for i in range(N):
        Image.fromarray(small[i]).save(os.path.join(root, f"depths_2/frame_{i:05d}.png"))
    a = load_nerfstudio_split(root, "train", depths=True, downscale_factor=2, **ALL)
    assert a.depths.shape == (N, H // 2, W // 2)
    assert np.array_equal(a.depths, (small.astype(np.float64) * 1e-3 * a.dataparser_scale).astype(np.float32))


def test_every_refusal_names_its_frame(tmp_path):
    from PIL import Image

    # a missing key on one frame of a split that has it on others
    root = str(tmp_path / "key")
    _capture(root, keys=(0, 1, 3))
    with pytest.raises(ValueError, match=r"frame images/frame_00002\.png has no depth_file_path"):
        load_nerfstudio_split(root, "train", depths=True, **ALL)
    # a missing file
    root = str(tmp_path / "file")
    _capture(root)
    os.remove(os.path.join(root, "depths/frame_00001.png"))
    with pytest.raises(FileNotFoundError, match=r"frame images/frame_00001\.png"):
        load_nerfstudio_split(root, "train", depths=True, **ALL)
    with pytest.raises(FileNotFoundError, match=r"frame images/frame_00001\.png"):
        load_nerfstudio_split(root, "train", depths=True, pixels=False, **ALL)
    # another size than the image's
    root = str(tmp_path / "size")
    _capture(root)
    Image.fromarray(np.ones((H, W + 1), np.uint16)).save(os.path.join(root, "depths/frame_00003.png"))
    with pytest.raises(ValueError, match=r"frame images/frame_00003\.png.*9 x 6 pixels"):
        load_nerfstudio_split(root, "train", depths=True, **ALL)
    # an 8-bit image is not a depth file
    root = str(tmp_path / "mode")
    _capture(root)
    Image.fromarray(np.ones((H, W), np.uint8)).save(os.path.join(root, "depths/frame_00000.png"))
    with pytest.raises(ValueError, match=r"frame images/frame_00000\.png.*mode L"):
        load_nerfstudio_split(root, "train", depths=True, **ALL)
    # negative and non-finite values
    for bad, at in ((-1.0, 1), (float("nan"), 2), (float("inf"), 0)):
        root = str(tmp_path / f"bad{at}")
        raw_f = _raw_depths().astype(np.float32)
        raw_f[at, 3, 3] = bad
        _capture(root, kind="npy", raw_f=raw_f)
        with pytest.raises(ValueError, match=rf"frame images/frame_0000{at}\.png.*negative or non-finite"):
            load_nerfstudio_split(root, "train", depths=True, **ALL)


def test_from_arrays_takes_depths():
    im = np.zeros((2, 4, 5, 3), np.uint8)
    c2w = np.tile(np.eye(4)[None, :3], (2, 1, 1))
    d = np.random.default_rng(0).random((2, 4, 5))
    s = BlenderScene.from_arrays(im, c2w, focal=5.0, depths=d)
    assert s.depths.dtype == np.float32 and np.array_equal(s.depths, d.astype(np.float32))
    assert BlenderScene.from_arrays(im, c2w, focal=5.0).depths is None
    assert np.array_equal(BlenderScene.from_arrays(im, c2w, focal=5.0, depths=torch.from_numpy(d)).depths, s.depths)
    with pytest.raises(ValueError, match="depths must be"):
        BlenderScene.from_arrays(im, c2w, focal=5.0, depths=d[:, :3])
    for bad in (-0.5, float("nan")):
        e = d.copy()
        e[1, 2, 2] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            BlenderScene.from_arrays(im, c2w, focal=5.0, depths=e)


# ------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("S", [1, 2, 5, 13])
def test_reference_gradient_matches_finite_differences_autograd_and_the_closed_form(S):
    """float64 autograd through w(sigma) against the closed form coded on its own (1e-12 of the scale) and against a central
    difference of the ray's float64 loss, ray by ray, for every ray whose largest gradient entry is at least 1.  The step moves the
    sample's optical depth by 1e-10, i.e. an empty sample's weight by a thousandth of EPS (log(w + EPS) is smooth only on that
    scale: truncation 1e-6 relative); the rounding is 1e-16 |L_ray| / h <= 6e-5 l absolute.  Asserted: 1e-4 of the ray's largest
    entry.  The saturated ray, whose entries behind the opaque sample are below the rounding, is held to the closed form alone."""
    inp = dz.depth_inputs(12, S, dz.depth_seed(S) + 1)
    grad, scale = dz.depth_backward_reference(inp)
    closed = dz.g_sigma_closed_form(inp)
    assert bool(torch.isfinite(grad).all()) and bool(((closed - grad).abs() <= 1e-12 * scale + 1e-300).all())
    eb, g_ray = inp["eb"].double(), inp["g_loss_ray"].double()
    l = eb[:, 1:] - eb[:, :-1]

    def ray_loss(r, sigma):
        with torch.no_grad():
            w, _, _, k = dz._terms(inp, dz.DEPTH_SIGMA, sigma, None)
            return float(g_ray[r] * (-torch.log(w + dz.LOSS_EPS) * k)[r].sum())

    base = inp["sigma"].double()
    checked, worst = 0, 0.0
    for r in range(12):
        top = float(grad[r].abs().max())
        if r == dz.RAY_SATURATED or top < 1.0:
            continue
        fd = torch.zeros(S, dtype=torch.float64)
        for k in range(S):
            if float(l[r, k]) == 0.0:
                continue
            h = 1e-10 / float(l[r, k])
            e = torch.zeros_like(base)
            e[r, k] = h
            fd[k] = (ray_loss(r, base + e) - ray_loss(r, base - e)) / (2 * h)
        checked += 1
        worst = max(worst, float((fd - grad[r]).abs().max()) / top)
    print(f"S={S}: finite difference vs autograd {worst:.3e} of a ray's largest entry over {checked} rays")
    assert checked >= 4 and worst <= 1e-4
    assert float(grad[dz.RAY_NO_TARGET].abs().max()) == 0.0


def test_planted_rays_are_what_their_description_says():
    S = 16
    inp = dz.depth_inputs(37, S, dz.depth_seed(S))
    eb, D = inp["eb"].double(), inp["target"].double()
    w, _, l = dz.weights64(eb, inp["sigma"].double())
    loss, scale = dz.loss_ray_reference(inp)
    assert float(D[dz.RAY_NO_TARGET]) == 0.0 and float(loss[dz.RAY_NO_TARGET]) == 0.0
    assert float(D[dz.RAY_BEFORE]) < float(eb[dz.RAY_BEFORE, 0]) and float(D[dz.RAY_BEYOND]) > float(eb[dz.RAY_BEYOND, -1])
    assert float(loss[dz.RAY_BEFORE]) != 0.0 and float(loss[dz.RAY_BEYOND]) != 0.0
    assert bool((eb[dz.RAY_ON_EDGE] == D[dz.RAY_ON_EDGE]).any())
    assert float(w[dz.RAY_EMPTY].abs().max()) == 0.0 and float(loss[dz.RAY_EMPTY]) == float(loss.max())
    assert float(w[dz.RAY_SATURATED, 0]) == 1.0 and 0.0 < float(w[dz.RAY_SATURATED, 1:].max()) < 1e-25
    assert bool((l[dz.RAY_ZERO_WIDTH] == 0).any()) and float(w[dz.RAY_THIN].max()) < dz.LOSS_EPS
    assert int((D[dz.PLANTED:] == 0).sum()) >= 1 and int((D[dz.PLANTED:] > 0).sum()) >= 20
    tiny, _ = dz.loss_ray_reference(inp, s=dz.TINY_SIGMA)
    assert float(tiny.abs().max()) == 0.0 and float(dz.g_sigma_closed_form(inp, s=dz.TINY_SIGMA).abs().max()) == 0.0


# which planted ray each mutation must move, in the loss ("L") or the gradient ("g"), by more than ten bounds
MUTATION_CASES = {"no_eps": ("L", dz.RAY_EMPTY), "two_s": ("L", dz.RAY_ON_EDGE), "no_lengths": ("L", dz.RAY_ON_EDGE),
                  "no_mask": ("L", dz.RAY_NO_TARGET), "bin_starts": ("L", dz.RAY_ON_EDGE), "fp32_weights": ("g", dz.RAY_THIN),
                  "total_minus_prefix": ("g", dz.RAY_SATURATED)}


@pytest.mark.parametrize("mutation", dz.MUTATIONS)
def test_each_mutation_moves_its_planted_ray_by_more_than_ten_bounds(mutation):
    """A kernel with this mistake in it would fail test_depth_gpu.py on the named ray: the mutated float64 value lies more than
    10 x BOUND x scale from the reference (BOUND = 4 x 2^-24, the GPU tests' bound, scale as they form it)."""
    S = 16
    inp = dz.depth_inputs(37, S, dz.depth_seed(S))
    what, ray = MUTATION_CASES[mutation]
    if what == "L":
        ref, scale = dz.loss_ray_reference(inp)
        got, _ = dz.loss_ray_reference(inp, mutation=mutation)
        moved = float(((got - ref).abs() / scale)[ray])
    else:
        ref, scale = dz.depth_backward_reference(inp)
        got = dz.g_sigma_closed_form(inp, mutation=mutation)
        moved = float(((got - ref).abs() / scale)[ray].max())
    print(f"{mutation}: ray {ray} moves by {moved / dz.BOUND:.3g} bounds")
    assert moved > 10 * dz.BOUND or moved != moved  # (NaN: the mutated value is not a number at all)
    if mutation == "fp32_weights":  # "tens of percent"
        assert moved > 0.1


def test_ray_depth_and_depth_error_references():
    """The host restatements against hand-made numbers."""
    depths = np.zeros((1, 4, 6), np.float32)
    depths[0, 1, 2], depths[0, 3, 5] = 2.0, 3.0
    idx = [(0, 1, 2), (0, 3, 5), (0, 0, 0), (0, 1, 2)]
    k = (4.0, 5.0, 3.0, 2.0)
    t = dz.ray_depth_reference(idx, [0, 0, 0, 1], depths, None, k, False)
    X, Y = (2.5 - 3.0) / 4.0, (1.5 - 2.0) / 5.0
    assert t[0] == 2.0 * np.sqrt(X * X + Y * Y + 1.0) and t[2] == 0.0 and t[3] == 0.0 and t[1] > 3.0
    assert list(dz.ray_depth_reference(idx, None, depths, None, k, True)) == [2.0, 3.0, 0.0, 2.0]
    fish = np.array([[4.0, 5.0, 3.0, 2.0, 0.01, 0, 0, 0, 0, 0, 1.0, 0]])
    assert list(dz.ray_depth_reference(idx, None, depths, fish, None, False)) == [0.0] * 4
    a, b, n = dz.depth_error_reference([1.0, 2.0, 5.0, 7.0], [1.5, 0.0, 3.0, 7.0], [1, 1, 1, 0])
    assert (a, b, n) == (2.5, 4.25, 2)


# ------------------------------------------------------------------------------------------------------------- ABI
NEW_CALLS = ("rsn_gather_ray_depth", "rsn_depth_loss_forward", "rsn_depth_loss_backward", "rsn_depth_error")


def test_entry_points_are_declared_bound_and_exported(lib):
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/rsn.h"
        assert name in _abi._SIGNATURES and name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "#define RSN_ABI_VERSION 18" in header and _abi.RSN_ABI_VERSION == 18 and lib.rsn_abi_version() == 18


def test_loss_argument_errors_come_back_without_a_launch(lib):
    """This test runs without a GPU: every call returns before a launch."""
    p = C.c_void_p(256)  # never dereferenced
    fwd, bwd = lib.rsn_depth_loss_forward, lib.rsn_depth_loss_backward
    assert fwd(4, None, 0, p, p, p, 0.1, p, None) == -1 and b"n_samples=0" in lib.rsn_last_error()
    assert fwd(-1, None, 8, p, p, p, 0.1, p, None) == -1 and b"n_rays=-1" in lib.rsn_last_error()
    assert fwd(4, None, 4097, p, p, p, 0.1, p, None) == -2 and b"n_samples=4097" in lib.rsn_last_error()
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert fwd(4, None, 8, p, p, p, s, p, None) == -1 and b"depth_sigma" in lib.rsn_last_error()
        assert bwd(4, None, 8, p, p, p, s, p, p, 1, None) == -1 and b"depth_sigma" in lib.rsn_last_error()
    for hole in range(4):
        args = [p, p, p, 0.1, p]
        args[hole if hole < 3 else 4] = None
        assert fwd(4, None, 8, *args, None) == -1 and b"NULL" in lib.rsn_last_error()
    assert fwd(0, None, 8, None, None, None, 0.1, None, None) == 0
    assert bwd(4, None, 0, p, p, p, 0.1, p, p, 1, None) == -1 and b"n_samples=0" in lib.rsn_last_error()
    assert bwd(-1, None, 8, p, p, p, 0.1, p, p, 0, None) == -1 and b"n_rays=-1" in lib.rsn_last_error()
    assert bwd(4, None, 4097, p, p, p, 0.1, p, p, 1, None) == -2 and b"n_samples=4097" in lib.rsn_last_error()
    for hole in range(5):
        args = [p, p, p, 0.1, p, p]
        args[hole if hole < 3 else hole + 1] = None
        assert bwd(4, None, 8, *args, 1, None) == -1 and b"NULL" in lib.rsn_last_error()
    assert bwd(0, None, 8, None, None, None, 0.1, None, None, 1, None) == 0


def test_gather_and_error_argument_errors_come_back_without_a_launch(lib):
    p = C.c_void_p(256)
    gather, err = lib.rsn_gather_ray_depth, lib.rsn_depth_error
    ok = dict(n_images=2, height=4, width=5)

    def g(n_rays=3, indices=p, level=None, depths=p, cameras=p, stride=9, k=(1.0, 1.0, 0.0, 0.0), fisheye=0, euclidean=0, t=p, **size):
        s = dict(ok, **size)
        return gather(n_rays, indices, level, depths, s["n_images"], s["height"], s["width"], cameras, stride, *k, fisheye, euclidean, t, None)

    assert g(n_rays=-1) == -1 and b"n_rays=-1" in lib.rsn_last_error()
    assert g(height=0) == -1 and b"height=0" in lib.rsn_last_error()
    assert g(stride=10) == -1 and b"camera_stride=10" in lib.rsn_last_error()
    assert g(cameras=None, k=(0.0, 1.0, 0.0, 0.0)) == -1 and b"fx=0" in lib.rsn_last_error()
    for hole in ("indices", "depths", "t"):
        assert g(**{hole: None}) == -1 and b"NULL" in lib.rsn_last_error()
    # a fisheye row has no z-plane: refused on the host, with the reason, whatever else is passed
    assert g(stride=12, fisheye=1, euclidean=0) == -1 and b"fisheye" in lib.rsn_last_error() and b"euclidean" in lib.rsn_last_error()
    assert g(stride=9, fisheye=1, euclidean=1) == -1 and b"12 columns" in lib.rsn_last_error()
    assert g(cameras=None, fisheye=1, euclidean=1) == -1 and b"without a camera table" in lib.rsn_last_error()
    assert g(n_rays=0, indices=None, depths=None, t=None) == 0 and g(n_rays=0, stride=12, fisheye=1, euclidean=1) == 0
    assert err(0, p, p, None, p, 64, p, None) == -1 and b"n_pixels=0" in lib.rsn_last_error()
    assert err((1 << 24) + 1, p, p, None, p, 1 << 20, p, None) == -1
    for hole in (1, 2, 4, 6):
        args = [100, p, p, None, p, 64, p, None]
        args[hole] = None
        assert err(*args) == -1 and b"NULL" in lib.rsn_last_error()
    assert err(100, p, p, None, p, 31, p, None) == -4 and b"31 bytes, 32 needed" in lib.rsn_last_error()
    assert err(100, p, p, None, C.c_void_p(4100), 64, p, None) == -1 and b"aligned" in lib.rsn_last_error()


# ------------------------------------------------------------------------------------------------------------- switches and names
def test_the_term_is_off_by_default_and_the_names_stand():
    model = trainer.make_model()
    coef = model.config.loss_coefficients
    assert "depth_loss_coarse" not in coef and "depth_loss_fine" not in coef and len(coef) == 12
    assert train_graph.depth_levels(model) == (False, False) and model.depth_sigma == 0.1
    coef["depth_loss_fine"] = 0.0
    assert train_graph.depth_levels(model) == (False, False)
    coef["depth_loss_fine"] = 0.01
    assert train_graph.depth_levels(model) == (False, True)
    coef["depth_loss_coarse"] = 0.002
    assert train_graph.depth_levels(model) == (True, True)
    assert len(train_graph.DIFF_KEYS) == 9 and len(train_graph.FUSED_KEYS) == 4 and len(train_graph.DIST_KEYS) == 2
    assert train_graph.DEPTH_KEYS == ("depth_loss_ray_coarse", "depth_loss_ray_fine")
    assert train_graph.DEPTH_COEF_KEYS == tuple(k for k, _ in train_ops.DEPTH_TERMS)
    assert train_graph.DEPTH_KEYS == tuple(k for _, k in train_ops.DEPTH_TERMS)
    assert {"depth_loss_coarse", "depth_loss_fine"} <= set(parallel._MEAN_TERMS)
    assert len(train_ops.LOSS_TERMS) == 8


def test_a_set_coefficient_without_its_fused_term_raises():
    off = {"depth_loss_fine": 0.0}
    assert train_ops.depth_loss_dict(None, {}) == {} and train_ops.depth_loss_dict(None, off) == {}
    with pytest.raises(_abi.RsnError, match="depth_loss_ray_fine"):
        train_ops.depth_loss_dict(None, {"depth_loss_fine": 0.01})
    with pytest.raises(_abi.RsnError, match="depth_loss_ray_coarse"):
        train_ops.depth_loss_dict({"depth_loss_ray_fine": torch.ones(3)}, {"depth_loss_fine": 0.01, "depth_loss_coarse": 0.1})
    got = train_ops.depth_loss_dict({"depth_loss_ray_fine": torch.tensor([1.0, 0.0, 5.0])}, {"depth_loss_fine": 0.5})
    assert list(got) == ["depth_loss_fine"] and float(got["depth_loss_fine"]) == 1.0  # the mean over all rays, supervised or not
    model = trainer.make_model()
    model.config.loss_coefficients["depth_loss_coarse"] = 0.01
    with pytest.raises(_abi.RsnError, match="depth_loss_coarse"):
        model.get_loss_dict({}, {"image": torch.zeros(4, 3)})


def test_ray_bundle_metadata_travels_with_the_rays():
    """The chunked step slices the bundle: the per-ray target must be sliced with it."""
    R = 10
    rb = pkg.RayBundle(origins=torch.zeros(R, 3), directions=torch.zeros(R, 3), pixel_area=torch.zeros(R, 1),
                       metadata={"depth": torch.arange(R, dtype=torch.float32).view(R, 1)})
    assert rb[3:7].metadata["depth"].flatten().tolist() == [3.0, 4.0, 5.0, 6.0]
    assert rb.get_row_major_sliced_ray_bundle(8, 10).metadata["depth"].flatten().tolist() == [8.0, 9.0]
    plain = pkg.RayBundle(origins=torch.zeros(R, 3), directions=torch.zeros(R, 3), pixel_area=torch.zeros(R, 1))
    assert plain[2:4].metadata is None


def test_parser_flags_and_defaults(capsys):
    base = ["train", "--data", "d", "--out", "o"]
    for run_defaults in (True, False):
        ap = trainer.build_parser(run_defaults)
        a = ap.parse_args(base)
        assert (a.depth_loss, a.depth_loss_coarse, a.depth_sigma, a.depth_unit_scale, a.depth_euclidean) == (None,) * 5
        a = ap.parse_args(base + ["--depth-loss", "0.01", "--depth-loss-coarse", "0.002", "--depth-sigma", "0.05",
                                  "--depth-unit-scale", "0.0005", "--depth-euclidean"])
        assert (a.depth_loss, a.depth_loss_coarse, a.depth_sigma, a.depth_unit_scale, a.depth_euclidean) == (0.01, 0.002, 0.05, 0.0005, True)
        e = ap.parse_args(["eval", "--data", "d", "--ckpt", "c"])
        assert e.depth is False and e.depth_unit_scale is None and e.depth_euclidean is None
        assert ap.parse_args(["eval", "--data", "d", "--ckpt", "c", "--depth"]).depth is True
    with pytest.raises(SystemExit):
        trainer.build_parser().parse_args(["train", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--depth-loss" in text and "--depth-sigma" in text and text.count("a starting point, not measured on a scene") >= 2


def test_run_state_records_the_settings_only_when_set():
    plain = trainer.make_run_state(0, 1024, "f32", False, "cpu")
    none = dict(depth_loss=None, depth_loss_coarse=None, depth_sigma=None, depth_euclidean=None)
    assert set(trainer.make_run_state(0, 1024, "f32", False, "cpu", **none)) == set(plain)
    assert set(trainer.make_run_state(0, 1024, "f32", False, "cpu", **dict(none, depth_loss=0.0, depth_sigma=0.2))) == set(plain)
    fine = trainer.make_run_state(0, 1024, "f32", False, "cpu", **dict(none, depth_loss=0.01))
    assert set(fine) - set(plain) == {"depth_loss"} and fine["depth_loss"] == 0.01 and fine["version"] == 1
    full = trainer.make_run_state(0, 1024, "f32", False, "cpu", **dict(depth_loss=0.01, depth_loss_coarse=0.002, depth_sigma=0.05,
                                                                         depth_euclidean=True))
    assert set(full) - set(plain) == {"depth_loss", "depth_loss_coarse", "depth_sigma", "depth_euclidean"}
    assert (full["depth_loss_coarse"], full["depth_sigma"], full["depth_euclidean"]) == (0.002, 0.05, True)
    with pytest.raises(KeyError):
        trainer.make_run_state(0, 1024, "f32", False, "cpu", **{"depth": 1})
    cfg, notes = trainer._resolve_run_settings(none, {"depth_loss": 0.01, "depth_sigma": 0.05})
    assert cfg == dict(none, depth_loss=0.01, depth_sigma=0.05) and notes == []   # recorded, not given: restored


def test_the_loader_is_asked_for_depths_only_by_a_depth_flag(tmp_path):
    """capture_load_args: without a depth flag the keyword arguments and the record are the ones they always were."""
    ap = trainer.build_parser()
    args = ap.parse_args(["train", "--data", "d", "--out", "o"])
    kwargs, settings = trainer.capture_load_args(args, None)
    assert "depths" not in kwargs and "depth_unit_scale" not in kwargs and "depth_unit_scale" not in settings
    kwargs, settings = trainer.capture_load_args(args, None, True)
    assert kwargs["depths"] is True and kwargs["depth_unit_scale"] == 1e-3 == settings["depth_unit_scale"] and "depths" not in settings
    args = ap.parse_args(["train", "--data", "d", "--out", "o", "--depth-loss", "1", "--depth-unit-scale", "0.002"])
    assert trainer.capture_load_args(args, None, True)[0]["depth_unit_scale"] == 0.002
    args = ap.parse_args(["eval", "--data", "d", "--ckpt", "c", "--depth"])
    assert trainer.capture_load_args(args, {"data": {"depth_unit_scale": 0.004}}, True)[0]["depth_unit_scale"] == 0.004



def test_load_scene_reads_the_depth_files_only_when_asked(tmp_path):
    """trainer.load_scene on a written capture: without the argument scene.depths is None and nothing about depth is recorded; with
    it the maps are loaded at the flag's unit, which is recorded, and a Blender-format scene is refused."""
    root = str(tmp_path / "capture")
    raw = _capture(root)
    ap = trainer.build_parser()
    args = ap.parse_args(["train", "--data", root, "--out", str(tmp_path / "run"), "--eval-mode", "all"])
    scene, settings = trainer.load_scene(ap, args, "train")
    assert scene.depths is None and "depth_unit_scale" not in settings
    args = ap.parse_args(["train", "--data", root, "--out", str(tmp_path / "run"), "--eval-mode", "all", "--depth-loss", "0.01",
                          "--depth-unit-scale", "0.002"])
    scene, settings = trainer.load_scene(ap, args, "train", depths=True)
    assert settings["depth_unit_scale"] == 0.002 and "depths" not in settings
    assert np.array_equal(scene.depths, (raw.astype(np.float64) * 0.002 * scene.dataparser_scale).astype(np.float32))
    # eval of that run: the unit comes from the checkpoint's record
    ev = ap.parse_args(["eval", "--data", root, "--ckpt", "c", "--depth"])
    held, _ = trainer.load_scene(ap, ev, "train", {"data": settings}, depths=True)
    assert np.array_equal(held.depths, scene.depths)
    blender = tmp_path / "blender"
    blender.mkdir()
    (blender / "transforms_train.json").write_text('{"camera_angle_x": 0.6, "frames": []}')
    args = ap.parse_args(["train", "--data", str(blender), "--out", "o", "--depth-loss", "0.01"])
    with pytest.raises(SystemExit):
        trainer.load_scene(ap, args, "train", depths=True)
