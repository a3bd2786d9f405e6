"""Shared helpers for the tests (fixture loading, tolerant comparisons)."""
import contextlib
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    groups = {}
    for k in z.files:
        if k == "meta":
            continue
        grp, key = k.split("/", 1)
        groups.setdefault(grp, {})[key] = torch.from_numpy(z[k])
    if meta.get("param_file"):  # parameters shared by several cases live in their own file
        pz = np.load(os.path.join(GOLDEN, meta["param_file"] + ".npz"), allow_pickle=False)
        groups["param"] = {k: torch.from_numpy(pz[k]) for k in pz.files}
    return meta, groups


def field_spec_from_meta(meta):
    from oracle.cpu_ref import FieldSpec

    return FieldSpec(num_layers=meta["layers"], width=meta["width"])


def model_spec_from_meta(meta):
    from oracle.cpu_ref import ModelSpec

    s = meta["samples"]
    return ModelSpec(num_coarse=s[0], num_fine=s[1], num_reflect_coarse=s[2], num_reflect_fine=s[3])


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


# ---------------------------------------------------------------------------------------------- the fog model of the export tests
FOG_DEPTH = 3.5


def fog_model(device):
    """A 4 x 64 model (seed 3) in eval mode on `device` whose density head is a constant: a fog of sigma = ln 2 / 3.5, so every eval
    ray (near plane 0) has its median depth about 3.5 from its camera and an accumulation of about 0.69, wherever it looks."""
    import reflect_sampling_nerf_amd as pkg
    from reflect_sampling_nerf_amd import trainer

    cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=4, base_mlp_layer_width=64)
    model = trainer.make_model(cfg, seed=3).to(device).eval()
    sigma = math.log(2.0) / FOG_DEPTH
    with torch.no_grad():
        model.field.field_output_density.net.weight.zero_()
        model.field.field_output_density.net.bias.fill_(math.log(math.expm1(sigma)) - model.field.density_bias)
    return model


def fog_checkpoint(run, device):
    """The fog model saved as step 5 of the run directory `run` -> (the checkpoint's path, str(run))."""
    import reflect_sampling_nerf_amd as pkg
    from reflect_sampling_nerf_amd import trainer

    model = fog_model(device)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    return trainer.save_checkpoint(trainer.checkpoint_path(str(run), 5), model, opt, 5), str(run)


# ---------------------------------------------------------------------------------------------- persistent-kernel coverage
@contextlib.contextmanager
def default_dtype(dt):
    """Run the oracle at another precision (oracle/cpu_ref.py builds its constants in torch's default dtype)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def multitile_geometry(label, job_points, tile, cus, min_per_wg=3, fixed_size=False):
    """Tile space of one persistent field launch: every job's points in `tile`-point tiles, grid = min(tiles, cus) (the
    launchers' rule).  Asserts that every workgroup walks at least `min_per_wg` tiles, that each job ends in a ragged tile,
    that the tile count is not a multiple of the grid and that job boundaries fall inside a round after the first.
    fixed_size: a BASELINE workload's size, not chosen by the test -- only the tiles-per-workgroup floor is asserted.
    -> (tiles, grid, first tile of each job)."""
    tiles, base = 0, []
    for p in job_points:
        base.append(tiles)
        tiles += -(-p // tile)
    grid = min(tiles, cus)
    per = tiles / grid
    print(f"[{label}] {tiles} tiles of {tile} points on {grid} workgroups: {per:.2f} tiles per workgroup")
    assert tiles // grid >= min_per_wg, f"{label}: {per:.2f} tiles per workgroup, the test needs >= {min_per_wg}"
    if fixed_size:
        return tiles, grid, base
    assert all(p % tile for p in job_points), f"{label}: every job must end in a ragged tile ({job_points}, tile {tile})"
    assert tiles % grid, f"{label}: {tiles} tiles are a multiple of the grid ({grid})"
    for b in base[1:]:
        assert b > grid and b % grid, f"{label}: job boundary at tile {b} is not inside a later round ({grid} workgroups)"
    return tiles, grid, base


def locate(err, tile, grid, base_tile=0):
    """err: per-point errors [N] of a job whose first tile is `base_tile` -> (worst, point, tile, loop iteration, worst of
    iteration 0, worst of iterations >= 1); `tile // grid` is the iteration of the persistent loop that wrote the point."""
    err = err.double().reshape(-1).cpu()
    it = (base_tile + torch.arange(err.numel()) // tile) // grid
    i = int(err.argmax())
    t = base_tile + i // tile
    e0 = float(err[it == 0].max()) if bool((it == 0).any()) else 0.0
    e1 = float(err[it >= 1].max()) if bool((it >= 1).any()) else 0.0
    return float(err[i]), i, t, t // grid, e0, e1


def check_points(label, name, err, bound, tile, grid, base_tile=0):
    """Assert max(err) <= bound for per-point errors [N]; print and report the worst point's tile and loop iteration."""
    e, i, t, it, e0, e1 = locate(err, tile, grid, base_tile)
    print(f"[{label}] {name}: worst {e:.3e} (bound {bound:.1e}) at point {i}, tile {t}, iteration {it}; "
          f"iteration 0 {e0:.2e}, iterations >= 1 {e1:.2e}")
    assert e <= bound, (f"{label} {name}: {e:.3e} > {bound:.1e} at point {i} (tile {t}, persistent-loop iteration {it}); "
                        f"worst in iteration 0 {e0:.3e}, in iterations >= 1 {e1:.3e}")
    return e


def point_err(got, ref, n):
    """max |got - ref| per point of [n, ...] tensors, in float64 on the host."""
    return (got.detach().double().cpu().reshape(n, -1) - ref.detach().double().cpu().reshape(n, -1)).abs().amax(dim=1)


def tile_rel_err(got, ref, tile):
    """Relative L2 error of each `tile`-row block of [n, C] rows: one corrupted tile cannot hide in a whole-tensor norm.
    -> per-point values (every point carries its tile's error) for locate()."""
    a, b = got.detach().double().cpu(), ref.detach().double().cpu()
    n = a.shape[0]
    a, b = a.reshape(n, -1), b.reshape(n, -1)
    nt = -(-n // tile)
    pad = nt * tile - n
    d2 = torch.nn.functional.pad(((a - b) ** 2).sum(1), (0, pad)).reshape(nt, tile).sum(1)
    r2 = torch.nn.functional.pad((b ** 2).sum(1), (0, pad)).reshape(nt, tile).sum(1)
    rel = (d2 / (r2 + 1e-12 * float(r2.mean()) + 1e-300)).sqrt()
    return rel.repeat_interleave(tile)[:n]


# ---------------------------------------------------------------------------------------------- buffers no kernel has written
# NaN bit patterns per dtype (int32 words: all ones; uint8 masks: a value that is neither 0 nor 1)
_POISON = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.bfloat16: (torch.int16, 0x7FC1), torch.int32: (torch.int32, -1),
           torch.uint8: (torch.uint8, 0xA5)}


def _poisoned(bufs):
    """Every buffer filled with a NaN bit pattern (int32 mask words: all ones), so that what no path wrote does not pass as equal."""
    for t in bufs.values():
        it, pattern = _POISON[t.dtype]
        t.view(it).fill_(pattern)
    return bufs


def _is_poison(t):
    """bool [rows]: every element of the row still holds the fill pattern."""
    it, pattern = _POISON[t.dtype]
    return (t.view(it).reshape(t.shape[0], -1) == pattern).all(dim=1).cpu()


def _has_poison(t):
    it, pattern = _POISON[t.dtype]
    return (t.view(it).reshape(t.shape[0], -1) == pattern).any(dim=1).cpu()


def _check_count(label, bufs, live):
    """Rows < live written (no element holds the fill pattern), rows >= live untouched (every element does)."""
    for k, t in bufs.items():
        assert not bool(_has_poison(t)[:live].any()), f"{label} {k}: a live row was not written"
        behind = ~_is_poison(t)[live:]
        assert not bool(behind.any()), f"{label} {k}: rows {(behind.nonzero().flatten() + live).tolist()[:8]} behind the count were written"


def _count(n, dev):
    return torch.tensor([n], dtype=torch.int32, device=dev)
