"""K29 (views of point clouds as shaded spheres), what needs no GPU: the two sample-image options, the refusals of
``draw_reconstruction``, ``meshes.render_points`` and the C entry, the workspace's closed form, the patch palette,
``render_clouds.py``'s parser and readers, and the numpy restatement (``_points_ref.py``) checked against cases whose
answer is known in closed form."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import _points_ref as pref
from fpsg_amd import meshes, visualization
from fpsg_amd._hip import FpsgHipError

TOP = meshes.camera_views(0.0, [0.0])
assert pref.MAX_RADIUS_PX == meshes.POINTS_MAX_RADIUS_PX          # the restatement and the package state one limit


# ---- options ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("evaluation", [False, True])
def test_sample_image_options_on_both_parsers(evaluation):
    from fpsg_amd import cli
    parser = cli.few_shot_parser(evaluation=evaluation)
    actions = {a.dest: a for a in parser._actions}
    assert actions["sample_renderer"].default == "matplotlib" and tuple(actions["sample_renderer"].choices) == ("matplotlib", "splat")
    assert actions["sample_up"].default == "z" and tuple(actions["sample_up"].choices) == ("z", "y")
    opt = parser.parse_args(["--sample_renderer", "splat", "--sample_up", "y"])
    assert (opt.sample_renderer, opt.sample_up) == ("splat", "y")
    with pytest.raises(SystemExit):
        parser.parse_args(["--sample_renderer", "blender"])


def test_default_options_carry_the_two_options():
    from fpsg_amd.engine import default_options
    opt = default_options()
    assert (opt.sample_renderer, opt.sample_up) == ("matplotlib", "z")


def test_draw_reconstruction_refuses_an_unknown_renderer_before_any_forward(tmp_path, monkeypatch):
    from fpsg_amd.engine import build_model, default_options
    model = build_model(default_options(device="cpu")).eval()
    monkeypatch.setattr(model, "reconstruct", lambda sample: pytest.fail("the forward ran"))
    with pytest.raises(ValueError, match="renderer must be 'matplotlib' or 'splat'"):
        model.draw_reconstruction({}, str(tmp_path / "a.png"), renderer="x")
    with pytest.raises(ValueError, match="up must be 'z' or 'y'"):
        model.draw_reconstruction({}, str(tmp_path / "a.png"), renderer="splat", up="x")
    assert os.listdir(tmp_path) == []


# ---- meshes.render_points ---------------------------------------------------------------------------------------------

def test_render_points_refusals_and_their_messages():
    pts = torch.zeros((2, 8, 3))
    for kw, text in [(dict(ssaa=3), "ssaa must be 1, 2 or 4"),
                     (dict(size=0), "size \\* ssaa must be from 1 to 8192"),
                     (dict(size=4097, ssaa=2), "size \\* ssaa must be from 1 to 8192"),
                     (dict(ortho_scale=0.0), "ortho_scale must be positive and finite"),
                     (dict(point_radius=float("nan")), "point_radius must be positive and finite"),
                     (dict(point_radius=-1.0), "point_radius must be positive and finite"),
                     (dict(point_radius=1e-7), "sample pixels, from 1/256 to 64 are supported"),
                     (dict(point_radius=0.5), "sample pixels, from 1/256 to 64 are supported"),
                     (dict(up="x"), "up must be 'z' or 'y'"),
                     (dict(views=np.zeros((0, 12), np.float32)), "no views"),
                     (dict(colors=torch.zeros((2, 8, 3))), "colors must be a uint8 tensor"),
                     (dict(colors=torch.zeros((2, 7, 3), dtype=torch.uint8)), "colors must be a uint8 tensor"),
                     (dict(background=np.zeros((5, 5, 3), np.uint8)), "a background image must be uint8"),
                     (dict(views=np.zeros((40000, 12), np.float32)), "clouds \\* views must be below 65536")]:
        with pytest.raises(ValueError, match=text):
            meshes.render_points(pts, **kw)
    for bad in (torch.zeros((8, 2)), torch.zeros((2, 2, 8, 3)), torch.zeros((0, 3)), np.zeros((8, 3), np.float32)):
        with pytest.raises(ValueError, match="expected \\[N,3\\] or \\[B,N,3\\] points"):
            meshes.render_points(bad)
    with pytest.raises(ValueError, match="more than 16384 points"):
        meshes.render_points(torch.zeros((16385, 3)))
    with pytest.raises(ValueError, match="shininess must be a power of two"):
        meshes.render_points(pts, material=meshes.PhongMaterial(shininess=3))
    with pytest.raises(FpsgHipError, match="no CPU fallback"):                # like render_views: never a CPU path
        meshes.render_points(pts)


def test_signature_of_render_points():
    import inspect
    sig = inspect.signature(meshes.render_points)
    assert list(sig.parameters) == ["points", "colors", "size", "elevations_deg", "azimuths_deg", "radius_cam",
                                    "ortho_scale", "up", "ssaa", "point_radius", "background", "material", "views",
                                    "return_buffers"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["size"], d["elevations_deg"], tuple(d["azimuths_deg"]), d["radius_cam"], d["ortho_scale"], d["up"], d["ssaa"],
            d["point_radius"], tuple(d["background"]), d["return_buffers"]) == \
        (256, 60.0, (0, 120, 240), 3.0, 2.0, "z", 2, 0.02, (1, 1, 1), False)
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for k, p in sig.parameters.items() if k != "points")


# ---- the C entry --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    assert "fpsg_points_render" in _hip.SIGNATURES and "fpsg_points_render_workspace_bytes" in _hip.SIGNATURES
    return _hip.load()


def _call(lib, points=64, colors=None, B=2, N=100, views=64, n_views=3, W=64, H=48, ssaa=2, ortho=2.0, radius=0.02,
          params=True, log2s=5, bg=None, image=64, radiance=None, point_id=None, depth=None, ws=64, ws_bytes=1 << 30):
    """Fake pointers (never dereferenced: every refusal comes before a launch or a copy)."""
    c_params = (ctypes.c_float * 17)(*([0.5] * 17)) if params else None
    return lib.fpsg_points_render(points, colors, B, N, views, n_views, W, H, ssaa, ctypes.c_float(ortho),
                                  ctypes.c_float(radius), c_params, log2s, bg, image, radiance, point_id, depth, ws,
                                  ws_bytes, None)


def test_entry_refuses_bad_arguments_with_the_documented_codes(lib):
    E_NULL, E_SHAPE, E_ALIGN, E_LIMIT = -1, -2, -3, -4
    for kw in (dict(B=0), dict(N=0), dict(n_views=0), dict(W=0), dict(H=-1), dict(ssaa=0), dict(ssaa=3), dict(ssaa=8),
               dict(W=66, ssaa=4), dict(ortho=0.0), dict(ortho=float("inf")), dict(radius=0.0), dict(radius=float("nan")),
               dict(radius=1e-7),                                    # R = 0
               dict(radius=2.01),                                    # R = 256 * 64.32
               dict(log2s=-1), dict(log2s=11), dict(ws_bytes=16 * 2 * 3 * 100 - 1)):
        assert _call(lib, **kw) == E_SHAPE, kw
    assert _call(lib, radius=1e-7) == E_SHAPE and b"sample pixels" in lib.fpsg_last_error()
    small = 0.001                                                    # keeps R in range on an image of 8194 samples
    for kw in (dict(N=16385), dict(W=8194, ssaa=2, radius=small), dict(H=8196, ssaa=2, radius=small), dict(n_views=1025),
               dict(B=65536 // 3 + 1)):
        assert _call(lib, **kw) == E_LIMIT, kw
    # B n_views = 65535 passes the limit (and stops at the workspace), 65538 does not
    assert _call(lib, B=21845, ws_bytes=0) == E_SHAPE and b"workspace" in lib.fpsg_last_error()
    assert _call(lib, B=21846, ws_bytes=0) == E_LIMIT
    for kw in (dict(points=None), dict(views=None), dict(ws=None), dict(params=False), dict(image=None)):
        assert _call(lib, **kw) == E_NULL, kw
    assert _call(lib, image=None) == E_NULL and b"no output" in lib.fpsg_last_error()
    for kw in (dict(points=66), dict(views=62), dict(radiance=65), dict(point_id=66), dict(depth=67), dict(ws=72)):
        assert _call(lib, **kw) == E_ALIGN, kw
    # shape before limit before pointers
    assert _call(lib, N=0, W=9000, points=None) == E_SHAPE and _call(lib, N=16385, points=None) == E_LIMIT
    # the largest and smallest R: 256 * 64 and 1 (radius / ortho_scale * 64 samples * 256)
    assert _call(lib, radius=2.0, ws_bytes=0) == E_SHAPE and b"workspace" in lib.fpsg_last_error()
    assert _call(lib, radius=2.0 / 16384, ws_bytes=0) == E_SHAPE and b"workspace" in lib.fpsg_last_error()


def test_workspace_is_the_closed_form_of_the_header(lib):
    f = lib.fpsg_points_render_workspace_bytes
    for B, N, NV, W, H in [(1, 1, 1, 1, 1), (2, 257, 3, 64, 48), (10, 2048, 3, 384, 384), (21845, 16384, 3, 8192, 8192)]:
        assert f(B, N, NV, W, H) == 16 * B * NV * N
    for shape in [(0, 8, 1, 8, 8), (1, 0, 1, 8, 8), (1, 8, 0, 8, 8), (1, 8, 1, 0, 8), (1, 8, 1, 8, 0), (1, 16385, 1, 8, 8),
                  (1, 8, 1, 8193, 8), (1, 8, 1025, 8, 8), (64, 8, 1024, 8, 8)]:
        assert f(*shape) == 0, shape


# ---- colours and the tool -------------------------------------------------------------------------------------------------

def test_patch_colors():
    pal = visualization.PATCH_PALETTE
    assert pal.shape == (16, 3) and pal.dtype == np.uint8 and len({tuple(c) for c in pal.tolist()}) == 16
    c = visualization.patch_colors(2048, 128)
    assert c.shape == (2048, 3) and c.dtype == np.uint8
    assert all((c[k * 128:(k + 1) * 128] == pal[k]).all() for k in range(16))
    c = visualization.patch_colors(100, 3)                           # 34 patches: the palette repeats, the last one is short
    assert (c[48:51] == pal[0]).all() and (c[51:54] == pal[1]).all() and (c[99] == pal[33 % 16]).all()
    for bad in [(0, 4), (8, 0), (8.5, 2), (8, True)]:
        with pytest.raises(ValueError):
            visualization.patch_colors(*bad)


def test_render_clouds_parser_and_readers(tmp_path):
    import render_clouds
    opt = render_clouds.build_parser().parse_args(["--input", "a.npy", "b.ply"])
    assert (opt.input, opt.output, opt.size, opt.ssaa, opt.point_radius, opt.elevation, opt.azimuths, opt.up,
            opt.background, opt.patch) == (["a.npy", "b.ply"], "clouds.png", 256, 2, 0.02, 60.0, [0.0, 120.0, 240.0], "z",
                                           "1,1,1", 0)
    with pytest.raises(SystemExit):
        render_clouds.build_parser().parse_args([])
    with pytest.raises(SystemExit):
        render_clouds.build_parser().parse_args(["--input", "a.npy", "--ssaa", "3"])
    assert render_clouds.background_colour("0.5,0,1") == (0.5, 0.0, 1.0)
    for bad in ("1,1", "a,b,c", "2,0,0"):
        with pytest.raises(ValueError, match="--background"):
            render_clouds.background_colour(bad)
    rng = np.random.default_rng(0)
    one, many = rng.normal(size=(50, 3)).astype(np.float32), rng.normal(size=(2, 30, 3))
    np.save(tmp_path / "one.npy", one)
    np.save(tmp_path / "many.npy", many)
    meshes.write_ply_points(str(tmp_path / "one.ply"), one)
    assert np.array_equal(render_clouds.read_clouds(str(tmp_path / "one.npy")), one[None])
    got = render_clouds.read_clouds(str(tmp_path / "many.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, many.astype(np.float32))
    assert np.array_equal(render_clouds.read_clouds(str(tmp_path / "one.ply")), one[None])       # %.9g keeps the bits
    np.save(tmp_path / "flat.npy", np.zeros(9, np.float32))
    np.save(tmp_path / "big.npy", np.zeros((16385, 3), np.float32))
    for name, text in [("flat.npy", "expected \\[N,3\\] or \\[B,N,3\\]"), ("big.npy", "more than 16384"),
                       ("one.txt", "expected a .npy or .ply")]:
        with pytest.raises(ValueError, match=text):
            render_clouds.read_clouds(str(tmp_path / name))


# ---- the restatement itself -------------------------------------------------------------------------------------------

def _point_at(i, j, W, z=0.0):
    """A point that the top view (x right, y up on the image, looking down -z) projects onto sample coordinate (i, j)
    exactly: W a power of two, i and j dyadic fractions."""
    return [(i / W - 0.5) * 2.0, (0.5 - j / W) * 2.0, z]


@pytest.mark.parametrize("k", [1, 3, 5])
def test_a_point_on_a_pixel_centre_covers_the_open_lattice_disc(k):
    W = 16
    radius = 2.0 * k / W                                             # R = 256 k exactly
    assert pref.snapped_radius(radius, 2.0, W, W) == 256 * k
    pts = np.array([[_point_at(8.5, 6.5, W)]], dtype=np.float32)     # the centre of sample (8, 6)
    pid, depth, snaps = pref.rasterize(pts, TOP, 2.0, radius, W, W)
    assert snaps[0, 0, 0].tolist() == [256 * 8 + 128, 256 * 6 + 128]
    jj, ii = np.mgrid[0:W, 0:W]
    want = (ii - 8) ** 2 + (jj - 6) ** 2 < k * k
    assert np.array_equal(pid[0, 0] == 0, want) and want.sum() > 0
    assert pid[0, 0, 6, 8 + k] == -1 and pid[0, 0, 6 - k, 8] == -1   # at distance exactly R: out
    assert pid[0, 0, 6, 8 + k - 1] == 0
    assert np.isinf(depth[0, 0][~want]).all()
    # the centre sample: t = 0, c = 1, depth = z - radius, z the camera's distance 3 to the plane of the point
    assert depth[0, 0, 6, 8] == np.float32(3.0) - np.float32(radius) * np.float32(1.0)
    # the sphere's profile: depth grows with the distance from the centre
    row = depth[0, 0, 6, 8:8 + k]
    assert (np.diff(row) > 0).all()


def test_the_lower_index_owns_every_sample_of_two_coincident_points():
    W = 16
    p = _point_at(5.25, 9.75, W, 0.125)
    pts = np.array([[[9, 9, 9], p, p, [9, 9, 9]]], dtype=np.float32)
    pid, depth, _ = pref.rasterize(pts, TOP, 2.0, 0.3, W, W)
    assert set(np.unique(pid)) == {-1, 1}
    # equal depth from different points: the nearer sphere still wins where the two differ
    pts[0, 2, 2] = 0.25
    pid2, _, _ = pref.rasterize(pts, TOP, 2.0, 0.3, W, W)
    assert set(np.unique(pid2)) == {-1, 2} and np.array_equal(pid2 >= 0, pid >= 0)


def test_the_two_shadings_of_the_restatement_agree_and_the_image_is_the_rounded_radiance():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.6, 0.6, (1, 40, 3)).astype(np.float32)
    views = meshes.camera_views(60.0, [0.0, 120.0])
    pid, _, snaps = pref.rasterize(pts, views, 2.0, 0.1, 32, 32)
    R = pref.snapped_radius(0.1, 2.0, 32, 32)
    mat = meshes.PhongMaterial()
    params = np.concatenate([mat.params((0.2, 0.4, 0.6)), [mat.ambient, mat.diffuse]]).astype(np.float32)
    colors = rng.integers(0, 256, (1, 40, 3), dtype=np.uint8)
    for col in (None, colors):
        r32 = pref.shade(pid, snaps, R, 2, params, mat.log2_shininess(), colors=col)
        r64 = pref.shade(pid, snaps, R, 2, params, mat.log2_shininess(), colors=col, dtype=np.float64)
        assert r32.dtype == np.float32 and r32.shape == (1, 2, 16, 16, 3) and (pid >= 0).sum() > 200
        assert np.abs(r32 - r64).max() < 1e-3 and np.abs(r32 - r64).max() > 0
        empty = (pid.reshape(1, 2, 16, 2, 16, 2) < 0).all(axis=(3, 5))
        assert np.array_equal(r32[empty], np.broadcast_to(params[12:15], r32[empty].shape))      # background alone
        img = pref.to_image(r32)
        assert img.dtype == np.uint8 and np.abs(img.astype(np.float64) - np.clip(r64, 0, 1) * 255).max() <= 0.5 + 1e-3 * 255
