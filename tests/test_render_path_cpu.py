"""CPU-side checks of the render path: camera paths (orbit, slerp interpolation, pose files), the `render` command line, the turbo
table, the fp64 reference the GPU tests compare against (tests/visualize_reference.py: how many of its bytes it declares
ambiguous), and the argument errors of rsn_visualize, which are raised before any launch."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, render, trainer
from reflect_sampling_nerf_amd._build import build_library
from tests import visualize_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def _pose(R, p):
    return np.concatenate([np.asarray(R, dtype=np.float64), np.asarray(p, dtype=np.float64).reshape(3, 1)], axis=1)


# ---------------------------------------------------------------------------------------------- orbit
@pytest.mark.parametrize("frames,center,radius,elevation,azimuth0", [(7, (0.0, 0.0, 0.0), 4.0, 30.0, 0.0),
                                                                       (12, (0.3, -0.2, 0.5), 2.5, -40.0, 75.0),
                                                                       (1, (1.0, 2.0, 3.0), 0.5, 0.0, -120.0),
                                                                       (5, (0.0, 0.0, 0.0), 3.0, 89.0, 10.0)])
def test_orbit_poses(frames, center, radius, elevation, azimuth0):
    c2w = render.orbit_path(frames, center, radius, elevation, azimuth0)
    assert c2w.shape == (frames, 3, 4) and c2w.dtype == np.float32
    # the properties hold to 1e-12 for the fp64 construction; the fp32 result is that construction rounded once
    c = np.asarray(center, dtype=np.float64)
    th = math.radians(elevation)
    ph = math.radians(azimuth0) + 2.0 * math.pi * np.arange(frames) / frames
    pos = c + radius * np.stack([math.cos(th) * np.cos(ph), math.cos(th) * np.sin(ph), np.full(frames, math.sin(th))], 1)
    f = (c - pos) / np.linalg.norm(c - pos, axis=1, keepdims=True)
    right = np.cross(f, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    want = np.stack([right, np.cross(right, f), -f, pos], axis=2)
    assert np.array_equal(c2w, want.astype(np.float32))
    R, p = want[:, :, :3], want[:, :, 3]
    assert np.abs(np.einsum("fij,fik->fjk", R, R) - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12
    rel = p - c
    assert np.abs(np.linalg.norm(rel, axis=1) - radius).max() <= 1e-12 * max(1.0, radius)
    assert np.abs(np.degrees(np.arcsin(rel[:, 2] / radius)) - elevation).max() <= 1e-9
    assert np.abs(-R[:, :, 2] - (c - p) / radius).max() <= 1e-12       # looks at the centre
    assert np.all(R[:, 2, 1] >= 0.0)                                   # up has a non-negative world-z component
    az = np.degrees(np.arctan2(rel[:, 1], rel[:, 0]))
    assert abs((az[0] - azimuth0 + 180.0) % 360.0 - 180.0) <= 1e-9     # frame 0 at azimuth0
    if frames > 1:
        step = (np.diff(np.concatenate([az, az[:1]])) + 360.0) % 360.0  # including the step from the last frame back to the first
        assert np.abs(step - 360.0 / frames).max() <= 1e-9             # evenly spaced: no repeated end frame
        assert len({tuple(np.round(q, 9)) for q in p}) == frames


def test_orbit_rejects_the_poles_and_bad_arguments():
    for e in (89.9, -89.9, 90.0, 120.0, float("nan")):
        with pytest.raises(ValueError, match="elevation"):
            render.orbit_path(4, (0, 0, 0), 1.0, e)
    render.orbit_path(4, (0, 0, 0), 1.0, 89.89)
    with pytest.raises(ValueError):
        render.orbit_path(0, (0, 0, 0), 1.0, 10.0)
    with pytest.raises(ValueError):
        render.orbit_path(4, (0, 0, 0), 0.0, 10.0)


# ---------------------------------------------------------------------------------------------- interpolation
def _orthonormal(c2w, tol):
    R = c2w[:, :, :3].astype(np.float64)
    return np.abs(np.einsum("fij,fik->fjk", R, R) - np.eye(3)).max() <= tol and np.abs(np.linalg.det(R) - 1.0).max() <= tol


def test_interpolate_identity_and_pass_through():
    rng = np.random.default_rng(0)
    poses = np.stack([_pose(_rot(rng.normal(size=3), rng.uniform(0, 360)), rng.normal(size=3)) for _ in range(5)]).astype(np.float32)
    same = render.interpolate_path(poses, 0)
    assert same.dtype == np.float32 and same.tobytes() == poses.tobytes()
    for steps in (1, 3):
        out = render.interpolate_path(poses, steps)
        assert out.shape == ((len(poses) - 1) * (steps + 1) + 1, 3, 4) and out.dtype == np.float32
        assert out[:: steps + 1].tobytes() == poses.tobytes()  # the given poses, bit for bit
        assert _orthonormal(out, 1e-6)  # fp32 storage of an fp64-orthonormal matrix
        for a in range(len(poses) - 1):  # translation linear
            for s in range(steps + 2):
                t = s / (steps + 1.0)
                want = (1 - t) * poses[a, :, 3].astype(np.float64) + t * poses[a + 1, :, 3].astype(np.float64)
                assert np.abs(out[a * (steps + 1) + s, :, 3] - want).max() <= 1e-6
    one = render.interpolate_path(poses[:1], 4)
    assert one.tobytes() == poses[:1].tobytes()
    assert render.interpolate_path(np.concatenate([poses, np.zeros((5, 1, 4), np.float32)], 1), 0).shape == (5, 3, 4)  # [F,4,4] in


def test_interpolate_midpoint_of_a_quarter_turn_is_an_eighth_turn():
    axis = (0.3, -0.5, 0.8)
    R0 = _rot((1, 2, 3), 25.0)
    poses = np.stack([_pose(R0, (0, 0, 0)), _pose(_rot(axis, 90.0) @ R0, (2, 4, 6))])
    mid = render.interpolate_path(poses, 1)[1]
    assert np.abs(mid[:, :3] - _rot(axis, 45.0) @ R0).max() <= 1e-6
    assert np.abs(mid[:, 3] - np.array([1, 2, 3])).max() <= 1e-6
    thirds = render.interpolate_path(poses, 2)
    assert np.abs(thirds[1][:, :3] - _rot(axis, 30.0) @ R0).max() <= 1e-6 and np.abs(thirds[2][:, :3] - _rot(axis, 60.0) @ R0).max() <= 1e-6


def test_interpolate_takes_the_short_arc_when_the_quaternions_disagree_in_sign():
    """Rotations by 170 and 190 degrees about z are 20 degrees apart, but the quaternions the matrices convert to, (cos 85, sin 85 z)
    and (cos 95, sin 95 z) = (-0.087, 0.996 z) -- or its negative -- may differ in sign: the midpoint must be 180 degrees, not 0."""
    poses = np.stack([_pose(_rot((0, 0, 1), 170.0), (0, 0, 0)), _pose(_rot((0, 0, 1), 190.0), (0, 0, 0))])
    qa, qb = render._quaternion(poses[0][:, :3]), render._quaternion(poses[1][:, :3])
    mid = render.interpolate_path(poses, 1)[1]
    assert np.abs(mid[:, :3] - _rot((0, 0, 1), 180.0)).max() <= 1e-6
    # and explicitly with opposite signs
    assert np.abs(render._rotation(render._slerp(qa, -qb, 0.5)) - render._rotation(render._slerp(qa, qb, 0.5))).max() <= 1e-12
    assert min(np.dot(qa, qb), np.dot(qa, -qb)) < 0.0
    # every branch of the matrix -> quaternion conversion gives the matrix back
    for axis, deg in (((1, 0, 0), 179.0), ((0, 1, 0), 179.0), ((0, 0, 1), 179.0), ((1, 1, 1), 10.0), ((1, -2, 0.5), 120.0)):
        R = _rot(axis, deg)
        assert np.abs(render._rotation(render._quaternion(R)) - R).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- pose files
def _write_transforms(path, n=3, with_size=False, fov=0.7):
    rng = np.random.default_rng(5)
    frames = []
    for i in range(n):
        m = np.eye(4)
        m[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 360))
        m[:3, 3] = rng.normal(size=3) * 3
        frames.append({"file_path": f"./nowhere/r_{i}", "transform_matrix": m.tolist()})
    meta = {"camera_angle_x": fov, "frames": frames}
    if with_size:
        meta.update(w=20, h=10)
    with open(path, "w") as fh:
        json.dump(meta, fh)
    return np.stack([np.asarray(f["transform_matrix"])[:3] for f in frames])


def test_load_poses_without_images_and_scale(tmp_path):
    path = str(tmp_path / "transforms_test.json")
    want = _write_transforms(path)
    got = render.load_poses(path)
    assert got["c2w"].shape == (3, 3, 4) and got["c2w"].dtype == np.float32 and np.array_equal(got["c2w"], want.astype(np.float32))
    assert got["camera_angle_x"] == 0.7 and got["width"] is None and got["height"] is None
    scaled = render.load_poses(path, scale_factor=0.5)
    assert np.array_equal(scaled["c2w"][:, :, :3], got["c2w"][:, :, :3])
    assert np.array_equal(scaled["c2w"][:, :, 3], got["c2w"][:, :, 3] * np.float32(0.5))
    _write_transforms(path, with_size=True)
    sized = render.load_poses(path)
    assert (sized["width"], sized["height"]) == (20, 10)
    with open(path, "w") as fh:
        json.dump({"frames": []}, fh)
    with pytest.raises(ValueError):
        render.load_poses(path)


# ---------------------------------------------------------------------------------------------- command line
def test_render_parses_with_documented_defaults():
    a = trainer.build_parser().parse_args(["render", "--ckpt", "run", "--out", "frames"])
    assert a.command == "render" and a.ckpt == "run" and a.out == "frames"
    assert a.channels == ["rgb", "diffuse", "tint", "roughness", "normals", "depth", "accumulation"]
    assert a.channels == list(render.DEFAULT_CHANNELS)
    assert a.frames == 120 and tuple(a.center) == (0.0, 0.0, 0.0) and a.radius is None and a.elevation is None
    assert a.chunk == 4096 == render.DEFAULT_CHUNK and a.mma == "f32" and a.tiles is False and a.interpolate == 0
    assert a.depth_range is None and a.split == "test" and a.path is None and a.poses is None and a.data is None
    assert a.width is None and a.height is None and a.fov_x is None
    b = trainer.build_parser().parse_args(["render", "--ckpt", "r", "--out", "o", "--channels", "mask", "rgb_direct", "--tiles",
                                           "--depth-range", "1", "9", "--center", "1", "2", "3", "--mma", "bf16", "--chunk", "1024"])
    assert b.channels == ["mask", "rgb_direct"] and b.tiles and b.depth_range == [1.0, 9.0] and b.center == [1.0, 2.0, 3.0]
    assert b.mma == "bf16" and b.chunk == 1024
    assert set(render.CHANNELS) == {"rgb", "rgb_direct", "diffuse", "tint", "roughness", "normals", "depth", "accumulation", "mask"}


def _cameras(argv):
    ap = trainer.build_parser()
    return trainer.resolve_render_args(ap, ap.parse_args(["render", "--ckpt", "r", "--out", "o", *argv]))


@pytest.mark.parametrize("missing", ["--width", "--height", "--fov-x"])
def test_missing_intrinsics_are_an_argparse_error_that_names_them(missing, capsys):
    given = {"--width": "12", "--height": "8", "--fov-x": "40"}
    del given[missing]
    argv = ["--radius", "4"] + [v for kv in given.items() for v in kv]
    with pytest.raises(SystemExit) as e:
        _cameras(argv)
    assert e.value.code == 2 and missing in capsys.readouterr().err
    with pytest.raises(SystemExit):  # the same through main, before it asks for a device
        trainer.main(["render", "--ckpt", "r", "--out", "o", *argv])
    assert missing in capsys.readouterr().err


def test_unknown_channel_and_missing_radius_are_argparse_errors(capsys):
    with pytest.raises(SystemExit) as e:
        trainer.build_parser().parse_args(["render", "--ckpt", "r", "--out", "o", "--channels", "rgb", "albedo"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "albedo" in err and all(name in err for name in render.CHANNELS)
    with pytest.raises(SystemExit):
        _cameras(["--width", "12", "--height", "8", "--fov-x", "40"])
    assert "--radius" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _cameras(["--width", "12", "--height", "8", "--fov-x", "40", "--radius", "4", "--elevation", "89.95"])
    assert "elevation" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _cameras(["--width", "12", "--height", "8", "--fov-x", "40", "--path", "poses"])
    assert "--poses" in capsys.readouterr().err


def test_cameras_from_the_command_line_and_from_files(tmp_path):
    cam = _cameras(["--width", "12", "--height", "8", "--fov-x", "40", "--radius", "4", "--frames", "5"])
    assert cam["c2w"].shape == (5, 3, 4) and (cam["width"], cam["height"]) == (12, 8)
    assert cam["fx"] == cam["fy"] == 0.5 * 12 / math.tan(0.5 * math.radians(40.0)) and (cam["cx"], cam["cy"]) == (6.0, 4.0)
    assert np.array_equal(cam["c2w"], render.orbit_path(5, (0, 0, 0), 4.0, 30.0))
    # --poses: its cameras, field of view and size; --interpolate inserts poses; the images it names do not exist
    path = str(tmp_path / "cams.json")
    want = _write_transforms(path, with_size=True).astype(np.float32)
    cam = _cameras(["--poses", path])
    assert np.array_equal(cam["c2w"], want) and (cam["width"], cam["height"]) == (20, 10)
    assert cam["fx"] == 0.5 * 20 / math.tan(0.35)
    cam = _cameras(["--poses", path, "--interpolate", "2", "--width", "40"])
    assert cam["c2w"].shape == (7, 3, 4) and cam["width"] == 40 and cam["fx"] == 0.5 * 40 / math.tan(0.35)
    # --data: an orbit at the mean distance and elevation of the split's cameras; the size is still open (no image, no w / h)
    scene = tmp_path / "scene"
    scene.mkdir()
    src = _write_transforms(str(scene / "transforms_val.json"))
    cam = _cameras(["--data", str(scene), "--split", "val", "--width", "16", "--height", "16", "--frames", "3"])
    p = src[:, :, 3]
    dist = np.linalg.norm(p, axis=1)
    want = render.orbit_path(3, (0, 0, 0), float(dist.mean()), float(np.degrees(np.arcsin(p[:, 2] / dist)).mean()))
    assert np.abs(cam["c2w"] - want).max() <= 1e-5
    with pytest.raises(SystemExit):
        _cameras(["--data", str(scene), "--split", "val"])
    cam = _cameras(["--data", str(scene), "--split", "val", "--width", "16", "--height", "16", "--path", "poses"])
    assert np.array_equal(cam["c2w"], src.astype(np.float32))


def test_data_gives_the_size_of_the_splits_first_image(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    scene = tmp_path / "scene"
    (scene / "nowhere").mkdir(parents=True)
    _write_transforms(str(scene / "transforms_test.json"))
    Image.new("RGBA", (14, 6)).save(scene / "nowhere" / "r_0.png")  # only the first frame's image exists; its header is all that is read
    cam = _cameras(["--data", str(scene), "--frames", "2"])
    assert (cam["width"], cam["height"]) == (14, 6) and cam["fx"] == 0.5 * 14 / math.tan(0.35) and (cam["cx"], cam["cy"]) == (7.0, 3.0)
    assert cam["c2w"].shape == (2, 3, 4)


# ---------------------------------------------------------------------------------------------- the reference and the table
def test_reference_declares_few_bytes_ambiguous():
    """At most 1 % of the pixels of any randomised GPU case (about 0.1 % is expected of uniform inputs: 3 channels x a band of 2e-4
    per unit of v*255), none of a special-value case: there the expected bytes are exact."""
    flagged = 0
    for kind in (ref.RGB, ref.UNIT, ref.GRAY, ref.LUT):
        lut = render.TURBO if kind == ref.LUT else None
        for h, w in ref.SHAPES:
            for with_alpha in (False, True):
                x, alpha = ref.random_case(kind, h, w, with_alpha)
                code, amb, alt, joint = ref.expected(kind, x, alpha, *ref.RANGE, lut)
                assert code.shape == amb.shape == alt.shape == (h * w, 3) and code.dtype == alt.dtype == np.uint8
                assert ref.ambiguous_pixels(amb) <= ref.MAX_AMBIGUOUS_SHARE * h * w, (kind, h, w, with_alpha)
                assert np.array_equal(alt[~amb], code[~amb]) and np.all(np.abs(alt[amb].astype(int) - code[amb]) >= 0)
                flagged += ref.ambiguous_pixels(amb)
        x, alpha = ref.special_values(kind)
        for table in ((render.TURBO, ref.ramp_lut()) if kind == ref.LUT else (None,)):
            code, amb, _, _ = ref.expected(kind, x, alpha, *ref.SPECIAL_RANGE, table)
            assert not amb.any(), kind
            a = np.asarray(alpha)
            with np.errstate(invalid="ignore"):
                clear = np.isnan(a) | (a <= 0)
            assert clear.any() and np.all(code[clear] == 255)  # nothing there: white, whatever x holds
    assert flagged <= 8


def test_reference_hand_values():
    code, amb, _, _ = ref.expected(ref.RGB, np.float32([[0.0, 0.25, 1.0], [np.nan, -np.inf, np.inf], [0.2, 0.3, 0.6]]), np.float32([1, 1, 0.5]))
    assert code.tolist() == [[0, 64, 255], [0, 0, 255], [153, 166, 204]] and not amb.any()  # over white at 1/2: .6, .65, .8 -> 153.5, 166.25, 204.5
    code, _, _, _ = ref.expected(ref.UNIT, np.float32([[-1.0, 0.0, 1.0]]))
    assert code.tolist() == [[0, 128, 255]]
    code, _, _, _ = ref.expected(ref.GRAY, np.float32([2.0, 4.0, 6.0, 7.0, 1.0]), None, 2.0, 6.0)
    assert code[:, 0].tolist() == [0, 128, 255, 255, 0]
    lut = np.zeros((256, 3), np.float32)
    lut[63] = (1.0, 0.25, 0.0)
    code, amb, _, _ = ref.expected(ref.LUT, np.float32([3.0]), None, 2.0, 6.0, lut)  # t = .25, t*255 = 63.75: entry 63
    assert code.tolist() == [[255, 64, 0]] and not amb.any()
    code, amb, alt, joint = ref.expected(ref.LUT, np.float32([63.0 / 255.0]), None, 0.0, 1.0, lut)  # on the edge between entries 62 and 63
    assert amb.all() and {tuple(code[0]), tuple(alt[0])} == {(255, 64, 0), (0, 0, 0)}
    assert ref.check(np.uint8([[255, 64, 0]]), code, amb, alt, joint) is None and ref.check(np.uint8([[0, 0, 0]]), code, amb, alt, joint) is None
    assert joint.all() and ref.check(np.uint8([[255, 0, 0]]), code, amb, alt, joint) is not None  # one entry for all channels


def test_turbo_table_shape_and_range():
    assert render.TURBO.shape == (256, 3) and render.TURBO.dtype == np.float32
    assert render.TURBO.min() >= 0.0 and render.TURBO.max() <= 1.0
    assert np.allclose(render.TURBO[0], (0.18995, 0.07176, 0.23217)) and np.allclose(render.TURBO[255], (0.4796, 0.01583, 0.01055))


def test_turbo_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    want = np.asarray(matplotlib.colormaps["turbo"].colors, dtype=np.float64)
    assert want.shape == (256, 3) and np.array_equal(render.TURBO, want.astype(np.float32))


# ---------------------------------------------------------------------------------------------- rsn_visualize without a device
def test_symbol_is_bound_and_abi_is_18(lib):
    assert "rsn_visualize" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "rsn_visualize")
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    assert re.search(r"#define RSN_ABI_VERSION 18\b", header) and _abi.RSN_ABI_VERSION == 18 and lib.rsn_abi_version() == 18
    for name, value in (("RSN_VIS_RGB", ref.RGB), ("RSN_VIS_UNIT", ref.UNIT), ("RSN_VIS_GRAY", ref.GRAY), ("RSN_VIS_LUT", ref.LUT)):
        assert re.search(rf"#define {name} {value}\b", header) and getattr(_abi, name) == value
    assert [c.kind for c in render.CHANNELS.values()].count(_abi.RSN_VIS_LUT) == 1


def test_argument_errors_return_before_any_launch(lib):
    """Made-up pointers: a call that reached the device would fault, and there is no device here anyway."""
    p = C.c_void_p(0x1000)

    def vis(h=4, w=6, kind=ref.RGB, x=p, alpha=None, lo=0.0, hi=1.0, lut=None, out=p, pitch=6, x0=0):
        rc = lib.rsn_visualize(h, w, kind, x, alpha, lo, hi, lut, out, pitch, x0, None)
        return rc, (lib.rsn_last_error() or b"").decode()

    for kwargs, word in ((dict(pitch=5), "row"), (dict(pitch=8, x0=3), "row"), (dict(x0=-1, pitch=9), "row"),
                         (dict(kind=ref.GRAY, lo=1.0, hi=1.0), "hi"), (dict(kind=ref.LUT, lut=p, lo=2.0, hi=1.0), "hi"),
                         (dict(kind=ref.GRAY, lo=float("nan")), "finite"), (dict(kind=ref.LUT, lut=p, hi=float("inf")), "finite"),
                         (dict(kind=4), "kind"), (dict(kind=-1), "kind"), (dict(kind=ref.LUT, lut=None), "lut"),
                         (dict(x=None), "NULL"), (dict(out=None), "NULL"), (dict(h=0), "height"), (dict(w=0), "height"),
                         (dict(h=-3), "height"), (dict(h=65536, w=32768, pitch=32768), "2^31")):
        rc, msg = vis(**kwargs)
        assert rc == INVALID and word in msg, (kwargs, rc, msg)
    # the python wrapper refuses what the C call cannot see
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        render.visualize(torch.zeros(4, 6, 3, dtype=torch.float64), ref.RGB, torch.zeros(4, 6, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        render.visualize(torch.zeros(4, 6), ref.RGB, torch.zeros(4, 6, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        render.visualize(torch.zeros(4, 6), ref.GRAY, torch.zeros(5, 6, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="channel"):
        render.check_channels(["rgb", "albedo"])
