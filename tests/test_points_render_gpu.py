"""K29 (views of point clouds as shaded spheres) on the GPU: ``point_id`` and ``depth`` equal the numpy restatement of the
definition (``_points_ref.py``, include/fpsg_hip.h) bit for bit, ``radiance`` equals its float32 shading bit for bit and
agrees with its float64 shading within a bound derived from the definition's operation count, ``image`` is the rounded
radiance; and the sample images of training and evaluation and ``render_clouds.py`` run end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, unit_ball_clouds

import _points_ref as pref
from fpsg_amd import meshes, visualization

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                 # fp32 unit roundoff
TOP = meshes.camera_views(0.0, [0.0])
THREE = np.concatenate([TOP, meshes.camera_views(60.0, [30.0, 200.0])])
MATERIAL = meshes.PhongMaterial()


def _params(material=MATERIAL, background=(1.0, 1.0, 1.0)):
    return np.concatenate([material.params(background), [material.ambient, material.diffuse]]).astype(np.float32)


def _at(i, j, W, z=0.0):
    """The point that the top view projects onto sample coordinate (i, j) exactly (W a power of two, i, j dyadic)."""
    return [(i / W - 0.5) * 2.0, (0.5 - j / W) * 2.0, z]


def _render(gpu, pts, views, W, H, ssaa, radius, colors=None, background=(1.0, 1.0, 1.0)):
    t = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(gpu)
    c = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors)).to(gpu)
    img, buf = meshes.render_points(t, colors=c, size=(H // ssaa, W // ssaa), ssaa=ssaa, views=views, point_radius=radius,
                                    background=background, return_buffers=True)
    return img.cpu().numpy(), {k: v.cpu().numpy() for k, v in buf.items()}


def _check(gpu, pts, views, W, H, ssaa, radius, colors=None, bg_image=None):
    """Renders and compares every output with the restatement; -> (want_id, want_depth, got buffers, snaps)."""
    pts = np.asarray(pts, np.float32)
    pts = pts[None] if pts.ndim == 2 else pts
    want_id, want_depth, snaps = pref.rasterize(pts, views, 2.0, radius, W, H)
    img, buf = _render(gpu, pts, views, W, H, ssaa, radius, colors, (1.0, 1.0, 1.0) if bg_image is None else bg_image)
    B, NV = len(pts), len(views)
    assert buf["point_id"].shape == (B, NV, H, W) and buf["point_id"].dtype == np.int32
    assert img.shape == (B, NV, H // ssaa, W // ssaa, 3) and img.dtype == np.uint8
    assert np.array_equal(buf["point_id"], want_id)
    assert np.array_equal(buf["depth"].view(np.uint32), want_depth.view(np.uint32))
    R = pref.snapped_radius(radius, 2.0, W, H)
    want = pref.shade(want_id, snaps, R, ssaa, _params(), MATERIAL.log2_shininess(), colors=colors, bg_image=bg_image)
    assert np.array_equal(buf["radiance"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(img, pref.to_image(buf["radiance"]))
    return want_id, want_depth, buf, snaps


# ---- single points ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where,covered", [("centre", 9), ("corner", 12)])
def test_one_point_on_a_pixel_centre_and_on_a_pixel_corner(gpu, where, covered):
    W, k = 8, 2
    radius = 2.0 * k / W                                             # R = 256 k
    assert pref.snapped_radius(radius, 2.0, W, W) == 256 * k
    ci, cj = (4.5, 3.5) if where == "centre" else (4.0, 4.0)
    want_id, want_depth, _, _ = _check(gpu, [_at(ci, cj, W)], TOP, W, W, 1, radius)
    jj, ii = np.mgrid[0:W, 0:W]
    disc = (ii + 0.5 - ci) ** 2 + (jj + 0.5 - cj) ** 2 < k * k       # strict: the sample at distance R is out
    assert np.array_equal(want_id[0, 0] == 0, disc) and disc.sum() == covered
    if where == "centre":
        assert want_depth[0, 0, 3, 4] == np.float32(3.0) - np.float32(radius) and want_id[0, 0, 3, 4 + k] == -1


def test_radius_of_one_snapped_unit_covers_only_exact_hits(gpu):
    W = 64
    radius = 2.0 / 16384                                              # R = 1: q < 1 means the sample centre itself
    assert pref.snapped_radius(radius, 2.0, W, W) == 1
    pts = [_at(10.5, 20.5, W), _at(10.5 + 1 / 256, 21.5, W), _at(40.5, 7.5, W, 0.5), _at(0.5, 63.5, W), _at(33.0, 33.0, W)]
    want_id, _, _, _ = _check(gpu, pts, TOP, W, W, 1, radius)
    assert (want_id >= 0).sum() == 3 and want_id[0, 0, 20, 10] == 0 and want_id[0, 0, 7, 40] == 2 and want_id[0, 0, 63, 0] == 3


# ---- clouds ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cloud(B, N, seed):
    return unit_ball_clouds(np.random.default_rng(seed), B, N) * np.float32(0.9)


def _colors(B, N, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, N, 3), dtype=np.uint8)


@pytest.mark.parametrize("with_colors", [False, True])
def test_two_clouds_one_point_past_a_chunk_three_views(gpu, with_colors):
    B, N, W, H = 2, 257, 64, 48
    want_id, _, _, _ = _check(gpu, _cloud(B, N, 1), THREE, W, H, 2, 0.05, _colors(B, N, 2) if with_colors else None)
    assert (want_id >= 0).mean() > 0.2 and want_id.max() == N - 1     # the 257th point is drawn


def test_a_sphere_over_several_tiles_and_the_border(gpu):
    W = 96
    radius = 2.0 * 40 / W                                            # 40 sample pixels
    assert pref.snapped_radius(radius, 2.0, W, W) == 256 * 40
    pts = [_at(50.3, 44.1, W, 0.2), _at(5.0, 90.0, W, 0.5), _at(95.5, 0.5, W, -0.3), _at(48.0, 48.0, W, -2.0)]
    want_id, _, _, _ = _check(gpu, pts, TOP, W, W, 2, radius, _colors(1, 4, 5))
    assert set(np.unique(want_id)) == {-1, 0, 1, 2, 3}                # the last one lies behind the first: a rim shows
    tiles = {(j // 32, i // 32) for j, i in zip(*np.nonzero(want_id[0, 0] == 0))}
    assert len(tiles) >= 6
    _check(gpu, pts, THREE, W, W, 1, radius)


def test_off_screen_far_and_non_finite_points(gpu):
    W = 32
    pts = np.array([[0.97, 0.0, 0.0], [-1.02, -0.99, 0.1],            # partly off screen
                    [3.0, 3.0, 0.0], [0.0, -1.2, 0.0],                # wholly off screen (radius 0.1)
                    [1e6, 0.1, 0.0], [-1e6, -1e6, 1e6],               # 10^6 away: the snap clamps
                    [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.1, 0.1, -np.inf], [3e38, 0.0, 0.0],
                    [0.0, 0.0, 3.3e38],                               # a finite depth of -3.3e38: drawn, in front of all
                    [0.2, -0.3, 0.4], [-0.5, 0.5, 0.0]], dtype=np.float32)
    for views in (TOP, THREE):
        want_id, _, _, _ = _check(gpu, pts, views, W, W, 1, 0.1)
        assert {0, 1, 10, 11, 12} <= set(np.unique(want_id)) <= {-1, 0, 1, 3, 5, 10, 11, 12}
    want_id, _, _, _ = _check(gpu, pts[2:10], TOP, W, W, 2, 0.1)
    assert (want_id == -1).all()                                      # nothing to draw: the background alone


def test_coincident_points_and_pairs_of_equal_depth(gpu):
    W = 16
    radius = 2.0 * 2 / W                                             # 2 sample pixels
    p = _at(5.25, 9.75, W, 0.125)
    pair = [_at(9.5, 4.5, W, 0.25), _at(11.5, 4.5, W, 0.25)]          # mirror images about the column of sample 10
    pts = [[9, 9, 9], p, p, pair[1], pair[0]]
    want_id, want_depth, _, _ = _check(gpu, pts, TOP, W, W, 1, radius)
    assert set(np.unique(want_id)) == {-1, 1, 3, 4}                   # 2 coincides with 1 and never wins
    assert want_id[0, 0, 4, 10] == 3                                 # equal depth at the mirror column: the lower index
    assert want_id[0, 0, 4, 9] == 4 and want_id[0, 0, 4, 11] == 3
    _check(gpu, pts, THREE, W, W, 1, radius)


def test_2048_points_in_16_patch_colours(gpu):
    N = 2048
    colors = visualization.patch_colors(N, 128)[None]
    want_id, _, buf, _ = _check(gpu, _cloud(1, N, 7), THREE, 128, 128, 2, 0.02, colors)
    assert len(np.unique(want_id)) > 1000
    seen = {tuple(c) for c in np.round(buf["radiance"].reshape(-1, 3) * 255).astype(int).tolist()}
    assert len(seen) > 16


def test_ssaa_4_over_a_background_image(gpu):
    B, N, W, H = 1, 300, 64, 96
    bg = np.random.default_rng(11).integers(0, 256, (H // 4, W // 4, 3), dtype=np.uint8)
    want_id, _, buf, _ = _check(gpu, _cloud(B, N, 12), THREE, W, H, 4, 0.06, bg_image=bg)
    cover = (want_id >= 0).reshape(B, 3, H // 4, 4, W // 4, 4).sum(axis=(3, 5))
    assert (cover == 0).any() and (cover == 16).any() and ((cover > 0) & (cover < 16)).any()
    want_bg = np.broadcast_to(bg.astype(np.float32) / np.float32(255), buf["radiance"].shape)
    assert np.array_equal(buf["radiance"][cover == 0], want_bg[cover == 0])


def test_a_batch_equals_each_cloud_alone_and_two_runs_are_identical(gpu):
    B, N, W = 3, 500, 64
    pts, colors = _cloud(B, N, 21), _colors(B, N, 22)
    img, buf = _render(gpu, pts, THREE, W, W, 2, 0.04, colors)
    again_img, again = _render(gpu, pts, THREE, W, W, 2, 0.04, colors)
    assert np.array_equal(img, again_img)
    for k in buf:
        assert np.array_equal(buf[k].view(np.uint32), again[k].view(np.uint32)), k
    for b in range(B):
        one_img, one = _render(gpu, pts[b], THREE, W, W, 2, 0.04, colors[b])
        assert np.array_equal(one_img[0], img[b])
        for k in buf:
            assert np.array_equal(one[k][0].view(np.uint32), buf[k][b].view(np.uint32)), (b, k)
    assert not np.array_equal(img[0], img[1])


def test_outputs_may_be_left_out(gpu):
    """The Python entry asks for the image alone unless ``return_buffers``: the same image either way."""
    t = torch.from_numpy(_cloud(2, 257, 1)).to(gpu)
    alone = meshes.render_points(t, size=32, views=THREE)
    both, buf = meshes.render_points(t, size=32, views=THREE, return_buffers=True)
    assert alone.shape == (2, 3, 32, 32, 3) and alone.device == t.device and torch.equal(alone, both)
    assert buf["point_id"].shape == (2, 3, 64, 64) and buf["radiance"].shape == (2, 3, 32, 32, 3)
    single = meshes.render_points(t[0], size=32, views=THREE)          # [N,3]: one cloud
    assert torch.equal(single[0], alone[0])


# ---- float64 ------------------------------------------------------------------------------------------------------------

def _radiance_bound(c64, hit, ssaa, params, shininess):
    """First-order bound, with the second-order terms carried as factors, on |fp32 radiance - float64 radiance| per
    output pixel for the operations the header lists; eps = 2^-24, c64 the float64 c per sample.
      t = (float) q / (float) (R R): two conversions and a division, t <= 1: 3 eps;  u = 1 - t: 4 eps;
      c = sqrt(u): |sqrt(u') - sqrt(u)| = |u' - u| / (sqrt(u') + sqrt(u)) <= min(4 eps / c, sqrt(4 eps)), + eps for its own
        rounding: dc.  (The rim of a sphere, c -> 0, is where the bound is widest: the square root's slope.)
      nx = (float) dx / (float) R: both conversions exact below 2^24, |nx| < 1: eps; ny likewise; nz = -c: dc;
      ndl = (nx lx + ny ly) + nz lz: carried eps (|lx| + |ly|) + dc |lz|; three products of at most 1 and two sums of at
        most 2: 7 eps;
      s = lz - (2 ndl) nz: carried 2 (d_ndl |nz| + |ndl| dc) <= 2.02 (d_ndl + dc); a product of at most 2 and a
        difference of at most 3: 5.02 eps.  spec is 0 on both sides of ndl = 0 because lz < 0 (asserted);
      s^S by log2 S squarings: |a^S - b^S| <= S max(a, b)^(S-1) |a - b| with a, b <= 1 + 8 eps + ds (n is a unit vector
        up to the roundings of t and c), and (S - 1) eps for the squarings' own roundings, times the same factor;
      colour: kd d_ndl + ks d_spec carried (ambient, diffuse, ka, kd, ks <= 1, asserted), 10 eps for the base colour's
        division and the products and sums (each at most 1.25, asserted);
      resolve: k <= n = ssaa^2 sums of at most n 1.25: n^2 1.25 eps, scaled by inv = 1 / n exactly; the background's
        division, product and the last sum: 4 eps."""
    p = np.asarray(params, np.float64)
    l, S = p[9:12], float(shininess)
    assert l[2] < 0 and max(p[0:9].max(), p[15], p[16]) <= 1.0
    assert max((p[0:3] + p[3:6] + p[6:9]).max(), p[15] + p[16] + p[6:9].max()) <= 1.25
    dc = np.minimum(4 * EPS / np.maximum(c64, 1e-300), np.sqrt(4 * EPS)) + EPS
    d_ndl = EPS * (abs(l[0]) + abs(l[1])) + dc * abs(l[2]) + 7 * EPS
    assert l[2] + 2.02 * d_ndl.max() < 0
    d_s = 2.02 * (d_ndl + dc) + 5.02 * EPS
    grow = (1 + 8 * EPS + d_s) ** (S - 1)
    d_spec = (S * d_s + (S - 1) * EPS) * grow
    d_col = np.where(hit, max(p[3:6].max(), p[16]) * d_ndl + p[6:9].max() * d_spec + 10 * EPS, 0.0)
    B, NV, H, W = hit.shape
    n = ssaa * ssaa
    per_pixel = d_col.reshape(B, NV, H // ssaa, ssaa, W // ssaa, ssaa).sum(axis=(3, 5)) / n
    return per_pixel + (n * 1.25 + 4) * EPS


@pytest.mark.parametrize("ssaa,with_colors", [(1, False), (2, True), (4, False)])
def test_radiance_against_float64_within_the_derived_bound(gpu, ssaa, with_colors):
    B, N, W = 2, 1024, 128
    pts = _cloud(B, N, 31)
    colors = _colors(B, N, 32) if with_colors else None
    radius = 0.03
    _, buf = _render(gpu, pts, THREE, W, W, ssaa, radius, colors, (0.2, 0.4, 0.6))
    pid = buf["point_id"]
    snaps = pref.snap_all(pts, THREE, 2.0, W, W)                    # on the kernel's own point_id: the shading alone
    R = pref.snapped_radius(radius, 2.0, W, W)
    params = _params(background=(0.2, 0.4, 0.6))
    r64, c64 = pref.shade(pid, snaps, R, ssaa, params, MATERIAL.log2_shininess(), colors=colors, dtype=np.float64,
                          parts=True)
    bound = _radiance_bound(c64, pid >= 0, ssaa, params, MATERIAL.shininess)[..., None]
    err = np.abs(buf["radiance"].astype(np.float64) - r64)
    print(f"K29 radiance vs float64 (ssaa {ssaa}, colours {with_colors}): worst error {err.max():.3e}, worst error / bound "
          f"{(err / bound).max():.3f}, bound median {np.median(bound):.3e} max {bound.max():.3e}, covered "
          f"{(pid >= 0).mean():.2f}")
    assert (pid >= 0).mean() > 0.2
    assert (err <= bound).all()


# ---- the sample images and the tool ---------------------------------------------------------------------------------------

def test_draw_reconstruction_with_the_splat_renderer(gpu, tmp_path):
    from PIL import Image

    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    torch.manual_seed(0)
    model = build_model(default_options(device="cuda", n_shot=2, n_query=2)).to(gpu).eval()
    sample = synthetic_episode(2, 2, n_pts=2048, img_size=224, seed=3, device=gpu)
    for name in ("splat", "matplotlib"):
        os.makedirs(tmp_path / name)
        torch.manual_seed(5)
        model.draw_reconstruction(sample, [7, str(tmp_path / name)], renderer=name)
    assert sorted(os.listdir(tmp_path / "splat")) == ["7.png", "7_0.npy", "7_0_gt.npy"]
    for f in ("7_0.npy", "7_0_gt.npy"):
        a, b = np.load(tmp_path / "splat" / f), np.load(tmp_path / "matplotlib" / f)
        assert a.shape == (2, 2048, 3) and np.array_equal(a, b)
    sheet = np.asarray(Image.open(tmp_path / "splat" / "7.png"))
    assert sheet.shape == (2 * 192, 2 * 3 * 192, 3)                  # Q rows; generated and ground truth, three views each
    syn, gt = torch.from_numpy(np.load(tmp_path / "splat" / "7_0.npy")).to(gpu), sample["pcq"].squeeze(0)
    want = visualization.render_reconstruction(syn, gt, model.pc_decoder.pts_per_patch)
    assert np.array_equal(sheet, want)
    left, right = sheet[:, :576].reshape(-1, 3), sheet[:, 576:].reshape(-1, 3)
    assert (right.max(axis=1) - right.min(axis=1)).max() <= 2          # ground truth: grey
    assert (left.max(axis=1).astype(int) - left.min(axis=1)).max() > 60                # generated: patch colours
    assert not np.array_equal(sheet[:192], sheet[192:])
    with pytest.raises(ValueError, match="expected \\[Q,N,3\\]"):
        visualization.render_reconstruction(syn[0], gt)


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_training_writes_splat_sample_images(gpu, tmp_path):
    from PIL import Image
    _run(["trainNetwork.py", "--synthetic", "--n_shot", "1", "--n_query", "1", "--epoch", "1", "--n_episode", "2",
          "--sample_interval", "1", "--sample_renderer", "splat", "--model_path", str(tmp_path), "--name", "s"])
    imgs = os.listdir(tmp_path / "s" / "images")
    assert "sample_img_1.png" in imgs and any(f.endswith("_gt.npy") for f in imgs)
    assert Image.open(tmp_path / "s" / "images" / "sample_img_1.png").size == (2 * 3 * 192, 192)


def test_render_clouds_end_to_end(gpu, tmp_path):
    from PIL import Image
    clouds = _cloud(3, 500, 41)
    np.save(tmp_path / "two.npy", clouds[:2])
    meshes.write_ply_points(str(tmp_path / "one.ply"), clouds[2])
    out = _run(["render_clouds.py", "--input", str(tmp_path / "two.npy"), str(tmp_path / "one.ply"), "--output",
                str(tmp_path / "sheet.png"), "--size", "64", "--patch", "125", "--azimuths", "0", "90"])
    assert "3 clouds x 2 views of 64 pixels" in out
    sheet = np.asarray(Image.open(tmp_path / "sheet.png"))
    assert sheet.shape == (3 * 64, 2 * 64, 3)
    t = torch.from_numpy(clouds).to(gpu)
    colors = torch.from_numpy(visualization.patch_colors(500, 125)).to(gpu).expand(3, 500, 3).contiguous()
    want = meshes.render_points(t, colors=colors, size=64, azimuths_deg=[0.0, 90.0])
    assert np.array_equal(sheet, want.permute(0, 2, 1, 3, 4).reshape(3 * 64, 2 * 64, 3).cpu().numpy())
