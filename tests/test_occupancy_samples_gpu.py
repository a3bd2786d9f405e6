"""GPU checks of per-sample empty-space skipping: rsn_occupancy_compact_samples between the two predicates of
tests/occupancy_samples_reference.py at edge shapes, its footprint rule, rsn_scatter_level, Field.evaluate_frustums_skipping
against evaluate_frustums (live samples keep their bits), the model's pipeline against an emulation built from evaluate_frustums
and the device's own `live`, no host read, the quality on the trained fixture, and the two commands."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, occupancy, ops, render, trainer
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import occupancy_reference as ref
from tests import occupancy_samples_reference as sref
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAD = 4  # guard elements in front of and behind every output (bins_c has to stay 8-byte aligned: an even count)
GUARD_F = -7.25e11
GUARD_I = -5
GUARD_B = 0xA5
INF = float("inf")


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _c3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Guarded:
    """A device buffer with PAD guard elements at either end; `body` is what the kernel gets."""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * PAD,), fill, device=DEV, dtype=dtype)
        self.body = self.buf[PAD:PAD + n]

    def host(self):
        h = self.buf.cpu().numpy()
        guards = np.concatenate([h[:PAD], h[PAD + self.n:]])
        assert np.all(guards == np.asarray(self.fill, dtype=h.dtype)), "a guard word was written"
        return h[PAD:PAD + self.n]


def device_compact(dims, origin, spacing, bits, outside, o, d, pa, bins, max_radius, n_dev=None):
    """One rsn_occupancy_compact_samples with guarded outputs -> host arrays (live [N], n_live, sample_index [N], the four compact
    arrays with their unwritten rows still holding GUARD_F)."""
    lib = _abi.load_library()
    R, S = bins.shape[0], bins.shape[1] - 1
    N = R * S
    nbytes = int(lib.rsn_occupancy_samples_workspace_bytes(R, S))
    assert nbytes >= 4 * ((N + 255) // 256 + 1)
    ws = Guarded(nbytes // 4, torch.int32, GUARD_I)
    live, n_live, idx = Guarded(N, torch.uint8, GUARD_B), Guarded(1, torch.int32, GUARD_I), Guarded(N, torch.int32, GUARD_I)
    oc, dc, pc, bc = (Guarded(N * k, torch.float32, GUARD_F) for k in (3, 3, 1, 2))
    ins = [_dev(a) for a in (o, d, pa, bins)]  # held until the launches have run
    nd = None if n_dev is None else torch.tensor([n_dev], device=DEV, dtype=torch.int32)
    check(lib.rsn_occupancy_compact_samples(R, ptr(nd), S, *[ptr(a) for a in ins], *dims, _c3(origin), _c3(spacing), ptr(bits), int(outside),
                                            float(max_radius), ptr(live.body), ptr(n_live.body), ptr(idx.body), ptr(oc.body), ptr(dc.body),
                                            ptr(pc.body), ptr(bc.body), ptr(ws.body), ops._stream()))
    torch.cuda.synchronize()
    ws.host()
    return {"live": live.host(), "n_live": int(n_live.host()[0]), "index": idx.host(), "o": oc.host().reshape(N, 3),
            "d": dc.host().reshape(N, 3), "pa": pc.host(), "bins": bc.host().reshape(N, 2)}


def check_compaction(got, o, d, pa, bins):
    """The properties that hold whatever the predicate decided: counts, the permutation, the compact rows bit for bit, and the rows
    past n_live untouched."""
    S = bins.shape[1] - 1
    live, n = got["live"], got["n_live"]
    assert set(np.unique(live)) <= {0, 1}
    assert n == int(live.sum())
    assert np.array_equal(got["index"], ref.expected_index(live))
    p = got["index"][:n]
    r, i = p // S, p % S
    assert np.array_equal(_bits(got["o"][:n]), _bits(o[r])) and np.array_equal(_bits(got["d"][:n]), _bits(d[r]))
    assert np.array_equal(_bits(got["pa"][:n]), _bits(pa[r]))
    assert np.array_equal(_bits(got["bins"][:n]), _bits(np.stack([bins[r, i], bins[r, i + 1]], axis=1)))
    for k in ("o", "d", "pa", "bins"):
        assert np.all(got[k][n:] == np.float32(GUARD_F)), k  # left unwritten


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint8) if isinstance(a[k], np.ndarray) else a[k], b[k].view(np.uint8) if isinstance(b[k], np.ndarray) else b[k])
               for k in a)


# ------------------------------------------------------------------------------------------------ 1. the mark, between the predicates
@pytest.mark.parametrize("outside", [False, True], ids=["inside_only", "outside_occupied"])
@pytest.mark.parametrize("share", [0.05, 0.5])
@pytest.mark.parametrize("gi", range(len(ref.DIMS)), ids=["x".join(map(str, d)) for d in ref.DIMS])
def test_mark_lies_between_the_two_predicates_and_compaction_is_exact(gi, share, outside):
    """Shapes (R, S) with R*S = 1, 63, 64, 65, 3075 and 70400, S in (1, 3, 64); 70400 samples are 275 blocks, more than the 256 the
    offset scan takes per round.  At 70400 the fp64 predicates are evaluated on a fixed random 4096 of the samples (the mark is
    per sample; every other property is checked on all of them)."""
    dims = ref.DIMS[gi]
    si = (0.05, 0.5).index(share)
    origin, spacing = ref.grid_frame(dims, gi)
    occ = ref.grid_case(dims, share, 2 * gi + si)
    bits = _dev(ref.pack_bits(occ).view(np.int32), np.int32)
    assert {R * S for R, S in sref.SHAPES} == {1, 63, 64, 65, 3075, 70400} and {S for _, S in sref.SHAPES} == {1, 3, 64}
    for R, S in sref.SHAPES:
        N = R * S
        seed = 100 * gi + 10 * si + R + S
        o, d, near, far, fam = ref.ray_cases(dims, origin, spacing, R, seed)
        bins = sref.make_bins(near, far, S, seed)
        pa = np.random.default_rng(seed).uniform(1e-7, 1e-5, size=R).astype(np.float32)
        got = device_compact(dims, origin, spacing, bits, outside, o, d, pa, bins, INF)
        check_compaction(got, o, d, pa, bins)
        subset = None if N <= 4096 else np.sort(np.random.default_rng(seed).choice(N, size=4096, replace=False))
        must, may, bad = sref.sample_predicates(o, d, bins, occ, origin, spacing, outside, subset)
        live = got["live"] if subset is None else got["live"][subset]
        skipped_wrongly, kept_wrongly = np.flatnonzero(must & (live == 0)), np.flatnonzero(~may & (live == 1))
        assert len(skipped_wrongly) == 0, (R, S, skipped_wrongly[:5])
        assert len(kept_wrongly) == 0, (R, S, kept_wrongly[:5])
        assert live[bad].all()
        again = device_compact(dims, origin, spacing, bits, outside, o, d, pa, bins, INF)
        assert same(got, again)
        if N == 70400:
            print(f"{dims} share {share} outside {outside}: {got['n_live']} of {N} live, {int(bad.sum())} of 4096 invalid, "
                  f"{int((must != may).sum())} undecided")
        if R >= 21:  # a device-side count, and NaN in every input of the rays behind it
            for nd in (0, R // 2):
                o2, d2, pa2, bins2 = o.copy(), d.copy(), pa.copy(), bins.copy()
                o2[nd:], d2[nd:], pa2[nd:], bins2[nd:] = np.nan, np.nan, np.nan, np.nan
                part = device_compact(dims, origin, spacing, bits, outside, o2, d2, pa2, bins2, INF, n_dev=nd)
                assert not part["live"][nd * S:].any()
                assert np.array_equal(part["live"][:nd * S], got["live"][:nd * S])
                check_compaction(part, o, d, pa, bins)  # the live rows hold the rays in front of the count: never a NaN of ours
            over = device_compact(dims, origin, spacing, bits, outside, o, d, pa, bins, INF, n_dev=R + 7)  # clamped to R
            assert same(over, got)


def test_compact_samples_argument_errors_and_the_empty_call():
    lib = _abi.load_library()
    bits = torch.zeros(1, device=DEV, dtype=torch.int32)
    n_live = torch.full((3,), GUARD_I, device=DEV, dtype=torch.int32)
    grid = (3, 3, 3, _c3((0, 0, 0)), _c3((1, 1, 1)))
    none = [None] * 7

    def call(R, S, radius=INF, n_live_ptr=ptr(n_live[1:]), g=grid):
        return lib.rsn_occupancy_compact_samples(R, None, S, None, None, None, None, *g, ptr(bits), 1, radius, None, n_live_ptr, *none[:6],
                                                 ops._stream())
    assert call(0, 4) == 0
    torch.cuda.synchronize()
    assert n_live.tolist() == [GUARD_I, 0, GUARD_I]  # n_rays == 0: nothing launched, the count set
    assert call(-1, 4) == -1 and call(4, 0) == -1 and call(715827883, 1) == -1 and b"n_rays" in lib.rsn_last_error()
    assert call(0, 4, float("nan")) == -1 and b"max_radius" in lib.rsn_last_error()
    assert call(0, 4, n_live_ptr=None) == -1
    assert call(0, 4, g=(1, 3, 3, _c3((0, 0, 0)), _c3((1, 1, 1)))) == -1
    assert call(0, 4, g=(3, 3, 3, _c3((0, 0, 0)), _c3((1, 0, 1)))) == -1 and b"spacing" in lib.rsn_last_error()
    assert call(4, 4) == -1 and b"NULL" in lib.rsn_last_error()  # rays, but no arrays
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the footprint rule
def test_footprint_rule_keeps_exactly_the_wide_samples():
    """An all-empty 5^3 grid over [-1, 1]^3, outside not occupied.  |d| = 2 and pixel_area = pi * 0.01 give a cone radius of
    0.2 * t; bins 0, 0.5, ..., 4 and max_radius 0.45: t_i+1 = 2.0 gives 0.40 (skipped), 2.5 gives 0.50 (live) -- samples 4 .. 7."""
    dims, origin, spacing = (5, 5, 5), np.float32([-1, -1, -1]), np.float32([0.5, 0.5, 0.5])
    bits = torch.zeros(ref.n_words(dims), device=DEV, dtype=torch.int32)
    S = 8
    o = np.float32([[-0.9, 0.1, -0.9]] * 5)
    d = np.float32([[0.0, 0.0, 2.0]] * 5)
    bins = np.tile(np.arange(S + 1, dtype=np.float32) * 0.5, (5, 1))
    pa = np.float32([np.pi * 0.01, np.inf, np.nan, 1e-9, -np.inf])
    got = device_compact(dims, origin, spacing, bits, False, o, d, pa, bins, 0.45)
    live = got["live"].reshape(5, S)
    assert live[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert live[1].all() and live[2].all() and live[4].all()  # a pixel area that is not finite: all live
    assert not live[3].any()
    assert np.array_equal(live != 0, sref.footprint(d, pa, bins, 0.45))
    check_compaction(got, o, d, pa, bins)
    off = device_compact(dims, origin, spacing, bits, False, o, d, pa, bins, INF)  # +inf switches the rule off
    assert off["live"].reshape(5, S).any(axis=1).tolist() == [False, True, True, False, True]
    zero = device_compact(dims, origin, spacing, bits, False, o, d, pa, bins, 0.0)  # t_1 = 0.5 is already wider than 0
    assert zero["live"].reshape(5, S)[[0, 3]].all()


# ------------------------------------------------------------------------------------------------ 3. rsn_scatter_level
def _level_struct(tensors):
    return ops.field_outputs_struct(tensors)


@pytest.mark.parametrize("names", [tuple(n for n, _ in sref.MEMBERS), ("sigma", "color"), ("tint",)], ids=["all", "sigma_color", "tint"])
@pytest.mark.parametrize("n", [1, 1000])
def test_scatter_level(n, names):
    lib = _abi.load_library()
    rows = dict(sref.MEMBERS)
    case = sref.level_case(n, n)
    rng = np.random.default_rng(n)
    for n_live in sorted({0, 1, n // 3, n}):
        flags = np.zeros(n, dtype=bool)
        flags[rng.permutation(n)[:n_live]] = True
        index = ref.expected_index(flags)
        src, dst = {}, {}
        for k in names:
            s = case[k].copy()
            s[n_live:] = np.nan  # never read
            src[k] = _dev(s)
            dst[k] = Guarded(n * rows[k], torch.float32, GUARD_F)
        idx_dev, count = _dev(index, np.int32), torch.tensor([n_live], device=DEV, dtype=torch.int32)
        check(lib.rsn_scatter_level(n, ptr(count), ptr(idx_dev), C.byref(_level_struct(src)),
                                    C.byref(_level_struct({k: v.body for k, v in dst.items()})), ops._stream()))
        torch.cuda.synchronize()
        for k in names:
            got = dst[k].host().reshape((n,) if rows[k] == 1 else (n, rows[k]))
            want = np.zeros_like(case[k])
            want[index[:n_live]] = case[k][:n_live]
            assert np.array_equal(_bits(got), _bits(want)), (k, n_live)  # every row written: no guard value, no NaN; skipped rows +0.0
    # a member set on one side only is refused; so is a NULL struct
    a, b = torch.zeros(n, device=DEV), torch.zeros(n, 3, device=DEV)
    idx_dev, count = torch.arange(n, device=DEV, dtype=torch.int32), torch.tensor([n], device=DEV, dtype=torch.int32)
    one, two = _level_struct({"sigma": a}), _level_struct({"sigma": a, "color": b})
    assert lib.rsn_scatter_level(n, ptr(count), ptr(idx_dev), C.byref(one), C.byref(two), ops._stream()) == -1 and b"member" in lib.rsn_last_error()
    assert lib.rsn_scatter_level(n, ptr(count), ptr(idx_dev), C.byref(two), C.byref(one), ops._stream()) == -1
    assert lib.rsn_scatter_level(n, ptr(count), ptr(idx_dev), None, C.byref(one), ops._stream()) == -1
    assert lib.rsn_scatter_level(-1, ptr(count), ptr(idx_dev), C.byref(one), C.byref(one), ops._stream()) == -1
    assert lib.rsn_scatter_level(n, None, ptr(idx_dev), C.byref(one), C.byref(one), ops._stream()) == -1
    assert lib.rsn_scatter_level(0, None, None, C.byref(one), C.byref(one), ops._stream()) == 0
    # an index outside 0 .. n - 1 writes nothing
    if n > 1:
        wild = torch.arange(n, device=DEV, dtype=torch.int32)
        wild[5], wild[6] = -1, n
        out = Guarded(n, torch.float32, GUARD_F)
        srcs = torch.ones(n, device=DEV)
        check(lib.rsn_scatter_level(n, ptr(count), ptr(wild), C.byref(_level_struct({"sigma": srcs})), C.byref(_level_struct({"sigma": out.body})),
                                    ops._stream()))
        torch.cuda.synchronize()
        got = out.host()
        assert got[5] == np.float32(GUARD_F) and got[6] == np.float32(GUARD_F) and np.all(np.delete(got, [5, 6]) == 1.0)


# ------------------------------------------------------------------------------------------------ models and grids
H, W = 10, 33
INTR = render.pinhole(W, H, 0.7)
POSES = render.orbit_path(2, (0.0, 0.0, 0.0), 4.0, 20.0)


def make_model(layers, width, seed=4, samples=(16, 16, 8, 8), chunk=64):
    """A small model whose collider keeps the near plane in eval mode (2 .. 6): the segments of cameras at radius 4 lie inside
    [-3, 3]^3."""
    torch.manual_seed(seed)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=samples[0], num_importance_samples=samples[1],
                                            num_reflect_coarse_samples=samples[2], num_reflect_importance_samples=samples[3],
                                            base_mlp_num_layers=layers, base_mlp_layer_width=width, eval_num_rays_per_chunk=chunk)
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 1.5
    model.collider.reset_near_plane = False
    return model.to(DEV).eval()


def volume_grid(inside):
    """33^3 vertices over [-3, 3]^3, outside counted as occupied; `inside`: a predicate of the vertex coordinates."""
    n = 33
    ax = np.linspace(-3.0, 3.0, n)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    _, origin, spacing = pkg.mesh.grid_frame((-3, -3, -3, 3, 3, 3), n)
    return occupancy.occupancy_from_volume(_dev(inside(x, y, z).astype(np.float32)), origin, spacing, 0.5, 1, True)


def ball_grid():
    return volume_grid(lambda x, y, z: x * x + y * y + z * z <= 0.36)


def full_grid():
    grid = volume_grid(lambda x, y, z: np.ones_like(x, dtype=bool))
    assert grid.occupied_share() == 1.0
    return grid


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool((a == b).all())


def random_level(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g) * 0.5
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1)
    pa = torch.rand(R, generator=g) * 1e-5 + 1e-7
    bins = 0.5 + 2.0 * torch.sort(torch.rand(R, S + 1, generator=g), dim=1).values
    return [t.to(DEV).contiguous() for t in (o, d, pa, bins)]


# ------------------------------------------------------------------------------------------------ 4. live samples keep their bits
def check_skipping_equals_plain(field, grid, R, S, label):
    o, d, pa, bins = random_level(R, S, R + S)
    for full in (True, False):
        for nd in (None, 0, 20):
            n_dev = None if nd is None else torch.tensor([nd], device=DEV, dtype=torch.int32)
            rows = R if nd is None else nd
            plain = field.evaluate_frustums(o, d, pa, bins, n_dev, full)
            skip = field.evaluate_frustums_skipping(grid, 0, o, d, pa, bins, n_dev, full)
            assert set(skip) == set(plain) | {"live"}
            live = skip["live"]
            assert live.shape == (R, S) and live.dtype == torch.uint8
            assert bool((live[:rows] == 1).all()) and not bool(live[rows:].any())  # every cell is occupied
            for k, v in plain.items():
                assert skip[k].shape == v.shape and skip[k].dtype == v.dtype
                assert same_bits(skip[k][:rows], v[:rows]), f"{label} full={full} n_dev={nd}: {k} differs"
                assert bool((skip[k][rows:] == 0).all()), k  # the rays behind the count: zeros
    return R * S


def test_live_samples_keep_their_bits_small_field():
    model = make_model(2, 32)
    grid = full_grid()
    check_skipping_equals_plain(model.field, grid, 37, 5, "2 x 32")
    assert grid.samples_seen[0] == 6 * 37 * 5 and grid.samples_seen[1:] == [0, 0, 0]
    assert grid.samples_live_dev.tolist() == [2 * (37 + 0 + 20) * 5, 0, 0, 0]


@pytest.mark.parametrize("mma", ["f32", "bf16x6", "bf16"])
def test_live_samples_keep_their_bits_full_width(mma):
    model = make_model(8, 256, seed=5)
    model.field.set_mma_mode(mma)
    check_skipping_equals_plain(model.field, full_grid(), 37, 32, f"8 x 256 {mma}")


# ------------------------------------------------------------------------------------------------ 5. the pipeline against an emulation
def emulated_skipping(self, grid, level_id, origins, directions, pixel_area, euclid_bins, n_dev=None, full=True):
    """evaluate_frustums, then zero in every member where the device's own `live` is 0."""
    c = occupancy.mark_and_compact(grid, origins, directions, pixel_area, euclid_bins, n_dev)
    level = self.evaluate_frustums(origins, directions, pixel_area, euclid_bins, n_dev, full)
    live = c["live"] != 0
    out = {k: torch.where(live if v.dim() == 2 else live.unsqueeze(-1), v, torch.zeros_like(v)) for k, v in level.items()}
    out["live"] = c["live"]
    return out


def flat_rays(model, pose):
    n = H * W
    return model.collider(render.camera_rays(pose, H, W, *INTR, DEV).get_row_major_sliced_ray_bundle(0, n))


def assert_outputs_equal(a, b, label):
    assert set(a) == set(b), label
    for k in a:
        assert same_bits(a[k], b[k]), f"{label}: {k} differs"


def test_pipeline_equals_the_emulation_and_the_full_grid_changes_nothing(monkeypatch):
    model = make_model(4, 64, chunk=150)  # 330 rays: three chunks, the last one ragged
    grid = ball_grid()
    model.occupancy, model.occupancy_samples = grid, True
    flat = flat_rays(model, POSES[0])
    image = render.camera_rays(POSES[0], H, W, *INTR, DEV)
    n_hit = int(occupancy.cull(grid, flat.origins.contiguous(), flat.directions.contiguous(), flat.nears.reshape(-1).contiguous(),
                               flat.fars.reshape(-1).contiguous())["n_hit"])
    assert 0 < n_hit <= 300, n_hit  # so the third chunk runs with a device count of 0
    seen0 = list(grid.samples_seen)
    real_one = dict(model(flat).items())  # items(): with the lazy [M, 1] entry
    real_img = model.get_outputs_for_camera_ray_bundle(image)
    seen = [b - a for a, b in zip(seen0, grid.samples_seen)]
    assert seen == [2 * 330 * 16, 2 * 330 * 16, 2 * 330 * 8, 2 * 330 * 8]  # one bundle of 330 rays, then chunks of 150, 150 and 30
    live = grid.samples_live_dev.tolist()
    print(f"ball grid: {n_hit} of 330 rays hit; samples seen {grid.samples_seen}, live {live}, mask {int(real_img['mask'].sum())}")
    assert all(0 < live[k] < 2 * n_hit * 16 for k in (0, 1))  # some samples of the hit rays skipped, some kept
    monkeypatch.setattr(type(model.field), "evaluate_frustums_skipping", emulated_skipping)
    emu_one = dict(model(flat).items())
    emu_img = model.get_outputs_for_camera_ray_bundle(image)
    monkeypatch.undo()
    assert_outputs_equal(real_one, emu_one, "get_outputs")
    assert_outputs_equal(real_img, emu_img, "get_outputs_for_camera_ray_bundle")
    assert real_one["mask"].dtype == torch.bool and torch.equal(real_one["mask"], emu_one["mask"])
    # sample skipping changed something here (else the comparison above shows nothing) ...
    model.occupancy_samples = False
    rays_only = model.get_outputs_for_camera_ray_bundle(image)
    assert not same_bits(rays_only["weights_coarse"], real_img["weights_coarse"])
    # ... and with every cell occupied it changes nothing: the bits of the culled path
    model.occupancy = full_grid()
    want = model.get_outputs_for_camera_ray_bundle(image)
    want_one = dict(model(flat).present())
    model.occupancy_samples = True
    got = model.get_outputs_for_camera_ray_bundle(image)
    got_one = dict(model(flat).present())
    assert_outputs_equal(got, want, "full grid, image")
    assert_outputs_equal(got_one, want_one, "full grid, bundle")
    # training never uses it
    model.train()
    seen = list(model.occupancy.samples_seen)
    model(flat[:32])
    assert model.occupancy.samples_seen == seen
    model.eval()


# ------------------------------------------------------------------------------------------------ 6. no host read
def test_render_path_with_sample_skipping_issues_no_host_read():
    model = make_model(4, 64)
    channels = tuple(render.CHANNELS)
    model.occupancy, model.occupancy_samples = ball_grid(), True
    render.render_path(model, POSES[:1], H, W, *INTR, channels)  # warm-up: streams, packed weights and the per-stream counters exist
    torch.cuda.synchronize()
    seen = list(model.occupancy.samples_seen)
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = render.render_path(model, POSES, H, W, *INTR, channels)
        flat = flat_rays(model, POSES[1])
        model(flat)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(frames) == 2 and all(b > a for a, b in zip(seen, model.occupancy.samples_seen))


# ------------------------------------------------------------------------------------------------ 7. the trained fixture
def trained_model():
    meta, g = load_golden("eval_trained_l8_w256")
    s = meta["samples"]
    assert list(s) == [32, 32, 16, 16] and (meta["layers"], meta["width"]) == (8, 256)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=s[0], num_importance_samples=s[1], num_reflect_coarse_samples=s[2],
                                            num_reflect_importance_samples=s[3], base_mlp_num_layers=8, base_mlp_layer_width=256)
    model = cfg.setup(scene_box=None, num_train_data=1)
    model.field.load_state_dict(g["param"], strict=True)
    return model.to(DEV).eval()


FIXTURE_PSNR_DB = 62.984  # measured on the device: profiles/occupancy_samples.json, "fixture_view" / "sample_skipping" / "psnr_db"
FIXTURE_PSNR_FLOOR_DB = FIXTURE_PSNR_DB - 3.0


def test_quality_on_the_trained_fixture():
    """The 40 x 40 view of tests/test_occupancy_gpu.py (radius 4, azimuth 30, elevation 25 degrees, horizontal field of view 50
    degrees, near 2, far 6), the 96^3 grid over [-3, 3]^3 at the defaults: some samples of the hit rays are skipped and some kept
    at both primary levels, the culled rays hold what the ray cull alone gives them, and the final colour stays within 3 dB of
    the PSNR against the plain render that was measured on the device (the margin: the float order of the reflect branch may move
    the odd pixel)."""
    model = trained_model()
    S = 40
    rays = render.camera_rays(render.orbit_path(1, (0.0, 0.0, 0.0), 4.0, 25.0, 30.0)[0], S, S, *render.pinhole(S, S, np.radians(50.0)), DEV)
    rays.nears = torch.full((S, S, 1), 2.0, device=DEV)
    rays.fars = torch.full((S, S, 1), 6.0, device=DEV)
    plain = model.get_outputs_for_camera_ray_bundle(rays)
    grid = occupancy.build_occupancy(model.field, (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0), 96)
    model.occupancy = grid
    culled = model.get_outputs_for_camera_ray_bundle(rays)
    model.occupancy_samples = True
    skipped = model.get_outputs_for_camera_ray_bundle(rays)
    flat = rays.get_row_major_sliced_ray_bundle(0, S * S)
    c = occupancy.cull(grid, flat.origins.contiguous(), flat.directions.contiguous(), flat.nears.reshape(-1).contiguous(),
                       flat.fars.reshape(-1).contiguous())
    gone, n_hit = c["hit"] == 0, int(c["n_hit"])
    seen, live = grid.samples_seen, grid.samples_live_dev.tolist()
    print(f"{n_hit} of {S * S} rays hit; samples seen {seen}, live {live}; live share of the hit rays' samples: "
          f"coarse {live[0] / (n_hit * 32):.4f}, fine {live[1] / (n_hit * 32):.4f}")
    for level in (0, 1):
        assert 0 < live[level] < n_hit * 32  # strictly between none and all of the hit rays' samples
        assert live[level] <= seen[level]
    assert set(skipped) == set(culled) == set(plain)
    for k in culled:  # culled rays: unchanged
        assert same_bits(skipped[k].reshape(S * S, -1)[gone], culled[k].reshape(S * S, -1)[gone]), k
    diff = (skipped["mid_reflect_fine"].clamp(0, 1) - plain["mid_reflect_fine"].clamp(0, 1)).reshape(S * S, 3)
    psnr = float(10.0 * torch.log10(1.0 / diff.double().pow(2).mean().clamp_min(1e-12)))
    worst = diff.abs().amax(dim=1)
    print(f"final colour against the plain render: PSNR {psnr:.3f} dB, worst pixel {float(worst.max()):.5f} at {int(worst.argmax())}, "
          f"{float((worst > 0.03).float().mean()):.5f} of the pixels off by more than 0.03")
    assert psnr >= FIXTURE_PSNR_FLOOR_DB, (psnr, FIXTURE_PSNR_DB)  # 62.984 dB measured, less 3 dB


# ------------------------------------------------------------------------------------------------ 8. the commands
PARENT_KEYS = {"resolution", "sigma", "dilate", "outside_occupied", "bounds", "occupied_share", "culled_share", "rays"}


def test_render_and_eval_commands_with_skip_empty_samples(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image

    model = trained_model()
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    ckpt = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path / "run"), 3), model, opt, 3)
    Hc, Wc = 12, 16
    base = ["render", "--ckpt", ckpt, "--width", str(Wc), "--height", str(Hc), "--fov-x", "50", "--radius", "4", "--elevation", "25",
            "--frames", "2", "--chunk", "64", "--channels", "rgb", "accumulation", "--occupancy-resolution", "64"]
    outs = {}
    for name, flag in (("rays_a", "--skip-empty"), ("samples", "--skip-empty-samples"), ("rays_b", "--skip-empty")):
        outs[name] = tmp_path / name
        assert trainer.main(base + ["--out", str(outs[name]), flag]) == 0
    metas = {k: json.loads((v / "frames.json").read_text()) for k, v in outs.items()}
    # without the flag: what --skip-empty alone gives, before and after a run with it
    assert metas["rays_a"] == {**metas["rays_b"], "frames": metas["rays_a"]["frames"]} and set(metas["rays_a"]["occupancy"]) == PARENT_KEYS
    for i in range(2):
        assert (outs["rays_a"] / "panel" / f"{i:04d}.png").read_bytes() == (outs["rays_b"] / "panel" / f"{i:04d}.png").read_bytes()
    occ = metas["samples"]["occupancy"]
    print("render --skip-empty-samples:", occ)
    assert set(occ) == PARENT_KEYS | {"samples"} and {k: occ[k] for k in PARENT_KEYS} == metas["rays_a"]["occupancy"]
    levels = occ["samples"]["levels"]
    assert list(levels) == list(occupancy.LEVELS) and occ["samples"]["max_radius"] > 0.0
    for name, v in levels.items():
        assert 0 <= v["live"] <= v["seen"] and v["seen"] > 0, name
    assert 0 < levels["coarse"]["live"] < levels["coarse"]["seen"]
    assert np.asarray(Image.open(outs["samples"] / "panel" / "0000.png")).shape == np.asarray(Image.open(outs["rays_a"] / "panel" / "0000.png")).shape
    # eval on a two-view scene
    scene = tmp_path / "scene"
    (scene / "test").mkdir(parents=True)
    rng = np.random.default_rng(0)
    frames = []
    for k, pose in enumerate(render.orbit_path(2, (0.0, 0.0, 0.0), 4.0, 25.0, 30.0)):
        Image.fromarray(rng.integers(0, 256, size=(Hc, Wc, 4), dtype=np.uint8), "RGBA").save(scene / "test" / f"r_{k}.png")
        frames.append({"file_path": f"./test/r_{k}", "transform_matrix": np.vstack([pose, [0, 0, 0, 1]]).tolist()})
    (scene / "transforms_test.json").write_text(json.dumps({"camera_angle_x": float(np.radians(50.0)), "frames": frames}))
    ev = ["eval", "--data", str(scene), "--ckpt", ckpt, "--occupancy-resolution", "64"]
    assert trainer.main(ev + ["--out", str(tmp_path / "m1.json"), "--skip-empty"]) == 0
    assert trainer.main(ev + ["--out", str(tmp_path / "m2.json"), "--skip-empty-samples"]) == 0
    m1, m2 = json.loads((tmp_path / "m1.json").read_text()), json.loads((tmp_path / "m2.json").read_text())
    print("eval --skip-empty-samples:", m2["occupancy"])
    assert set(m1["occupancy"]) == PARENT_KEYS and set(m2) == set(m1) and set(m2["occupancy"]) == PARENT_KEYS | {"samples"}
    for name, v in m2["occupancy"]["samples"]["levels"].items():
        assert 0 <= v["live"] <= v["seen"] and v["seen"] > 0, name
