"""K26 (surface sampling) and K27 (orthographic Phong views) on the GPU: both equal the numpy restatement of their
definitions (``_mesh_ref.py``, include/fpsg_hip.h) bit for bit where the definition is integer or fixed-order fp32, the
shading agrees with a float64 evaluation within a bound derived from its operation count, and ``prepare_dataset.py``
turns a tree of ``.off`` files into one that ``FewShotModelNet`` reads."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import _mesh_ref as ref
from fpsg_amd import datasets, meshes, sampling
from fpsg_amd._hip import FpsgHipError

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                 # fp32 unit roundoff


# ---- K26 ------------------------------------------------------------------------------------------------------------

def _soup(F, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (F + 2, 3)).astype(np.float32)
    f = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], axis=1).astype(np.int32)
    return v, f


def _hard65():
    """65 faces: areas spanning 10^6 : 1, zero-area faces, duplicated faces, faces on NaN / inf vertices."""
    sides = np.concatenate([[1.0, 1e-3], np.geomspace(1e-3, 1.0, 55)]).astype(np.float32)
    v, f = [], []
    for k, s in enumerate(sides):
        o = np.float32(2.0 * k)
        v += [[o, 0, 0], [o + s, 0, 0], [o, s, 0]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    n = len(v)
    v += [[np.nan, 0, 0], [np.inf, 1, 0], [1e30, 0, 0], [0, 1e30, 0]]
    f += [[0, 0, 1], [5, 5, 5], [0, 1, 2], [0, 1, 2], [0, 1, n], [0, n + 1, 2], [0, n + 2, n + 3], [3, 4, 3]]
    f = np.asarray(f, dtype=np.int32)
    assert len(f) == 65
    return np.asarray(v, dtype=np.float32), f


@functools.lru_cache(maxsize=None)
def _k26_mesh(F):
    if F == 1:
        return np.array([[0, 0, 0], [1, 0, 0.5], [0, 2, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)
    if F == 2:
        return (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float32),
                np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
    if F == 12:
        return ref.cube()
    if F == 65:
        return _hard65()
    if F == 777:
        return _soup(777, 3)
    v, f = ref.icosphere(5)
    assert len(f) == F == 20480
    return v, f


def _k26_u(C, n, seed):
    """Random rows, with u0 also 0, the largest float below 1 and values on and beside CDF boundaries."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 3), dtype=np.float32)
    T = np.float64(C[-1])
    edges = (C[:-1][:: max(1, len(C) // 16)].astype(np.float64) / T).astype(np.float32)
    special = np.concatenate([[0.0, np.nextafter(np.float32(1), np.float32(0)), 0.5], edges,
                              np.nextafter(edges, np.float32(0)), np.nextafter(edges, np.float32(1))]).astype(np.float32)
    k = min(len(special), n)
    u[:k, 0] = special[:k]
    if n > 8:
        u[-4:, 1:] = [[0, 0], [np.nextafter(np.float32(1), np.float32(0)), 0], [0.25, np.nextafter(np.float32(1), np.float32(0))],
                      [1.0, 1.0]]                      # the last row is clamped below 1 by the definition
    return u


@pytest.mark.parametrize("F,n", [(1, 1), (2, 64), (12, 2048), (777, 333), (65, 4096), (20480, 2048)])
def test_sampling_equals_the_restatement_bit_for_bit(gpu, F, n):
    v, f = _k26_mesh(F)
    q, C = ref.weights(v, f)
    if F == 65:
        a = ref.areas(v, f)
        assert a[a > 0].max() / a[a > 0].min() >= 1e6 - 1 and (q[57:] == 0)[[0, 1, 4, 5, 6, 7]].all()
    u = _k26_u(C, n, seed=F + n)
    want_p, want_f = ref.sample(v, f, u)
    tv, tf, tu = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), torch.from_numpy(u).to(gpu)
    assert np.array_equal(meshes.surface_cdf(tv, tf).cpu().numpy().astype(np.uint64), C)
    pts, fidx = meshes.sample_surface(tv, tf, n, u=tu)
    assert pts.shape == (n, 3) and pts.dtype == torch.float32 and fidx.dtype == torch.int64
    assert np.array_equal(fidx.cpu().numpy(), want_f)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
    assert (q[want_f] > 0).all()
    again_p, again_f = meshes.sample_surface(tv, tf, n, u=tu)                # the same u: the same bits
    assert torch.equal(again_p, pts) and torch.equal(again_f, fidx)


def test_two_triangle_square_splits_exactly_at_one_half(gpu):
    v, f = _k26_mesh(2)
    below = np.nextafter(np.float32(0.5), np.float32(0))
    u = np.array([[0.5, 0.3, 0.3], [below, 0.3, 0.3]], dtype=np.float32)
    _, fidx = meshes.sample_surface(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), 2, u=torch.from_numpy(u).to(gpu))
    assert fidx.tolist() == [1, 0]


def test_mesh_without_area_is_an_error_not_a_fault(gpu):
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 0, 1], [1, 1, 1], [0, 1, 3]], dtype=np.int32)
    tv, tf = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    assert int(meshes.surface_cdf(tv, tf)[-1]) == 0
    with pytest.raises(FpsgHipError, match="no area"):
        meshes.sample_surface(tv, tf, 16)
    with pytest.raises(ValueError, match="face indices"):
        meshes.sample_surface(tv, torch.tensor([[0, 1, 4]], dtype=torch.int32, device=gpu), 16)
    pts, _ = meshes.sample_surface(*(torch.from_numpy(a).to(gpu) for a in ref.cube()), 16)   # the device is fine
    assert torch.isfinite(pts).all()


def test_oversampled_set_is_thinned_by_farthest_point_sampling(gpu):
    v, f = ref.icosphere(2)
    tv, tf = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    n, over = 512, 4
    u = torch.rand((n * over, 3), generator=torch.Generator().manual_seed(5))
    all_p, all_f = meshes.sample_surface(tv, tf, n * over, u=u)
    pts, fidx = meshes.sample_surface(tv, tf, n, u=u, oversample=over)
    keep = sampling.farthest_point_sample(all_p.unsqueeze(0), n)[0]
    assert keep[0] == 0 and len(torch.unique(keep)) == n                      # n distinct rows of the oversampled set
    assert torch.equal(pts, all_p[keep]) and torch.equal(fidx, all_f[keep])
    assert len(np.unique(pts.cpu().numpy(), axis=0)) == n
    g1, _ = meshes.sample_surface(tv, tf, n, generator=torch.Generator().manual_seed(5), oversample=over)
    assert torch.equal(g1, pts)                                             # u is torch.rand from the generator


# ---- K27: face-id and depth buffers ----------------------------------------------------------------------------------

TOP = meshes.camera_views(0.0, [0.0])
THREE = np.concatenate([TOP, meshes.camera_views(60.0, [30.0, 200.0])])


def _pix(i, j, R):
    return (i / R - 0.5) * 2.0, (0.5 - j / R) * 2.0


def _buffers(gpu, v, f, views, W, H, ssaa=1, **kw):
    img, buf = meshes.render_views(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), size=(H // ssaa, W // ssaa),
                                   ssaa=ssaa, views=views, return_buffers=True, **kw)
    return img, buf


def _check_raster(gpu, v, f, views, W, H, ssaa=1):
    want_id, want_depth, hits = ref.rasterize(v, f, views, 2.0, W, H)
    _, buf = _buffers(gpu, v, f, views, W, H, ssaa)
    got_id, got_depth = buf["face_id"].cpu().numpy(), buf["depth"].cpu().numpy()
    assert got_id.shape == (len(views), H, W)
    assert np.array_equal(got_id, want_id)
    assert np.array_equal(got_depth.view(np.uint32), want_depth.view(np.uint32))
    return want_id, hits


@pytest.mark.parametrize("W,H,ssaa", [(64, 64, 1), (67, 45, 1), (32, 32, 2)])
def test_buffers_equal_the_restatement_over_three_views(gpu, W, H, ssaa):
    v, f = ref.icosphere(2)
    cv, cf = ref.cube(-0.3, 0.45)
    v, f = np.concatenate([v * np.float32(1.3), cv]), np.concatenate([f, cf + len(v)])      # the cube's corners stick out
    want_id, _ = _check_raster(gpu, v, f, THREE, W, H, ssaa)
    for k in range(3):
        assert (want_id[k] >= 0).sum() > W * H // 5 and len(np.unique(want_id[k])) > 40


def _scene(name):
    R = 32
    if name == "shared_diagonal":
        (x0, y0), (x1, y1) = _pix(3, 5, R), _pix(19, 21, R)
        v = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], dtype=np.float32)
        return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), R
    if name == "fan":
        cx, cy = _pix(16.5, 15.5, R)
        ang = np.linspace(0, 2 * np.pi, 64, endpoint=False) + 0.01
        rim = np.stack([cx + 0.7 * np.cos(ang), cy + 0.7 * np.sin(ang), 0.1 * np.cos(3 * ang)], axis=1)
        v = np.concatenate([[[cx, cy, 0.2]], rim]).astype(np.float32)
        f = np.array([[0, 1 + k, 1 + (k + 1) % 64] for k in range(64)], dtype=np.int32)
        f[::3] = f[::3][:, [0, 2, 1]]
        return v, f, R
    if name == "coincident":
        v = np.array([[-0.7, -0.6, 0.1], [0.8, -0.5, 0.3], [0.1, 0.9, -0.2], [4, 4, 4], [5, 4, 4], [4, 5, 4]],
                     dtype=np.float32)
        return v, np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2], [0, 2, 1]], dtype=np.int32), R
    if name == "full_plus_subpixel":
        rng = np.random.default_rng(8)
        big = np.array([[-3, -1.5, -0.5], [3, -1.5, -0.5], [0, 4, -0.5]], dtype=np.float32)     # covers the whole image
        c = rng.uniform(-1, 1, (5000, 1, 3)) * np.array([1, 1, 0.4])
        small = (c + rng.uniform(-0.02, 0.02, (5000, 3, 3))).reshape(-1, 3).astype(np.float32)   # about half a pixel
        f = np.concatenate([[[0, 1, 2]], 3 + np.arange(15000).reshape(5000, 3)]).astype(np.int32)
        return np.concatenate([big, small]), f, R
    if name == "clipped":
        v = np.array([[-1.5, -0.2, 0], [0.3, -0.4, 0], [-0.2, 1.7, 0],        # partly off screen
                      [2, 2, 0], [3, 2, 0], [2, 3, 0],                         # wholly off screen
                      [1e6, 0.1, -0.3], [-1e6, -1e6, -0.3], [-0.5, 1e6, -0.3], # 10^6 away, clamped by the snap; behind face 0
                      [0.2, 0.2, 0.5], [3e38, 0.2, 0.5], [0.2, -0.9, 0.5],     # px overflows to inf: the face is skipped
                      [-3, 0, 0], [0, -3, 0], [-3, -3, 0]], dtype=np.float32)  # bounding box over the image, no coverage
        return v, np.arange(15, dtype=np.int32).reshape(5, 3), R
    assert name == "degenerate_and_reversed"
    v = np.array([[-0.8, -0.8, 0], [0.8, -0.8, 0], [0.8, 0.8, 0], [-0.8, 0.8, 0.4], [0, 0, 0.1], [np.nan, 0, 0]],
                 dtype=np.float32)
    f = np.array([[0, 1, 1], [0, 4, 2], [2, 1, 0], [0, 2, 3], [3, 2, 0], [4, 4, 4], [0, 1, 5]], dtype=np.int32)
    return v, f, R


@pytest.mark.parametrize("name", ["shared_diagonal", "fan", "coincident", "full_plus_subpixel", "clipped",
                                  "degenerate_and_reversed"])
def test_raster_edge_cases_equal_the_restatement(gpu, name):
    v, f, R = _scene(name)
    views = TOP if name != "coincident" else THREE
    want_id, hits = _check_raster(gpu, v, f, views, R, R)
    if name == "shared_diagonal":
        assert hits[0].sum() == 16 * 16 and hits.max() == 1 and (want_id[0, 5:21, 3:19] >= 0).all()
    if name == "fan":
        assert hits.max() == 1 and want_id[0, 15, 16] >= 0
    if name == "coincident":
        assert set(np.unique(want_id)) == {-1, 1}                            # the lowest face index wins equal depths
    if name == "full_plus_subpixel":
        assert (want_id[0] >= 0).all() and (want_id[0] > 0).sum() > 100 and (want_id[0] == 0).sum() > 100
    if name == "clipped":
        assert set(np.unique(want_id)) == {0, 2}
    if name == "degenerate_and_reversed":
        ids = set(np.unique(want_id))                                        # 3 and 4 coincide up to rounding of the depth
        assert {-1, 2, 3} <= ids <= {-1, 2, 3, 4}                            # the others are skipped


# ---- K27: shading ------------------------------------------------------------------------------------------------------

def _shading_bound(v, f, material, ssaa):
    """First-order bound on |fp32 radiance - float64 radiance| for the operations the header lists, eps = 2^-24:
      edges b - a: eps |e|; each turned by a 3-term dot product with a unit row: + 3 eps |e| per component, so a
        vector error of 4 sqrt(3) eps |e| = 6.93 eps |e|;
      cross product: 2 * 6.93 eps |e1| |e2| carried over + 2 sqrt(3) eps |e1| |e2| of its own = 17.3 eps |n| / sin(phi),
        phi the angle at the face's first vertex; normalisation (3 squares, 2 adds, sqrt, divide): 3.5 eps;
        rho = 17.3 eps / sin(phi) + 3.5 eps is the unit normal's error;
      n.l: rho + 3 eps;   s = l_z - (2 n.l) n_z: 2 (rho + 3 eps + rho) + 3 eps;
      s^S by log2 S squarings (s <= 1): S ds + (S - 1) eps;
      colour: kd (d(n.l) + eps) + ks (d(spec) + eps) + 2 eps;  the sum of ssaa^2 samples, the scaling and the
        background's share: 14 eps more."""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    e1, e2 = b - a, c - a
    sin_phi = np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    p = material.params().astype(np.float64)
    S = material.shininess
    rho = 17.3 * EPS / sin_phi.min() + 3.5 * EPS
    d_ndl = rho + 3 * EPS
    d_s = 2 * (d_ndl + rho) + 3 * EPS
    d_spec = S * d_s + (S - 1) * EPS
    return p[3:6].max() * (d_ndl + EPS) + p[6:9].max() * (d_spec + EPS) + 2 * EPS + 14 * EPS


@functools.lru_cache(maxsize=None)
def _shaded(ssaa, bg_kind):
    gpu = torch.device("cuda:0")
    v, f = ref.cube()
    tv, tf = ref.tetrahedron()
    v, f = np.concatenate([v, tv * np.float32(1.2)]), np.concatenate([f, tf[:, [0, 2, 1]] + len(v)])
    size = 48
    if bg_kind == "image":
        bg = np.random.default_rng(4).integers(0, 256, (size, size, 3), dtype=np.uint8)
    else:
        bg = (0.1, 0.55, 0.9)
    mat = meshes.PhongMaterial()
    img, buf = _buffers(gpu, v, f, THREE, size * ssaa, size * ssaa, ssaa, background=bg, material=mat)
    return v, f, mat, bg, img.cpu(), {k: t.cpu() for k, t in buf.items()}


@pytest.mark.parametrize("ssaa,bg_kind", [(1, "colour"), (2, "image"), (2, "colour")])
def test_radiance_agrees_with_float64_on_the_same_face_ids(gpu, ssaa, bg_kind):
    v, f, mat, bg, img, buf = _shaded(ssaa, bg_kind)
    bound = _shading_bound(v, f, mat, ssaa)
    print(f"shading bound {bound:.3e} ({bound / EPS:.0f} eps); 1/5100 = {1 / 5100:.3e}")
    assert bound < 1 / 5100                     # a tenth of half a grey level, at the default shininess of 32
    is_img = bg_kind == "image"
    want = ref.shade64(v, f, THREE, buf["face_id"].numpy(), ssaa, mat.params((0, 0, 0) if is_img else bg),
                       mat.log2_shininess(), bg_image=bg if is_img else None)
    err = np.abs(buf["radiance"].numpy().astype(np.float64) - want).max()
    print(f"largest |radiance - float64| = {err:.3e} ({err / EPS:.1f} eps)")
    assert err <= bound
    covered = (buf["face_id"].numpy() >= 0).mean()
    assert 0.15 < covered < 0.9 and want.max() - want.min() > 0.3


@pytest.mark.parametrize("ssaa,bg_kind", [(1, "colour"), (2, "image")])
def test_image_is_the_quantised_radiance_and_the_background_shows_through(gpu, ssaa, bg_kind):
    v, f, mat, bg, img, buf = _shaded(ssaa, bg_kind)
    rad = buf["radiance"]
    assert img.dtype == torch.uint8 and img.shape == (3, 48, 48, 3)
    assert torch.equal(img, torch.round(rad.clamp(0, 1) * 255).to(torch.uint8))
    fid = buf["face_id"].reshape(3, 48, ssaa, 48, ssaa)
    empty = (fid < 0).all(dim=4).all(dim=2)
    assert empty.sum() > 500
    if bg_kind == "image":
        assert torch.equal(img[empty], torch.from_numpy(bg).expand(3, -1, -1, -1)[empty])
    else:
        want = torch.round(torch.tensor(bg, dtype=torch.float32) * 255).to(torch.uint8)
        assert (img[empty] == want).all()
    assert len(torch.unique(img[~empty])) >= 6                              # flat shading: a grey per lit face and view


def test_half_covered_pixel_is_the_stated_mix(gpu):
    size, ssaa = 16, 2
    R = size * ssaa
    (x0, y0), (x1, y1) = _pix(-4, -4, R), _pix(17, R + 4, R)                # the right edge between samples 16 and 17
    v = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    bg = (0.25, 0.5, 0.75)
    _, buf = _buffers(gpu, v, f, TOP, R, R, ssaa, background=bg)
    fid, rad = buf["face_id"][0].cpu().numpy(), buf["radiance"][0].cpu().numpy().astype(np.float64)
    assert (fid[:, :17] >= 0).all() and (fid[:, 17:] < 0).all()             # output column 8: samples 16 (in), 17 (out)
    colour = rad[3, 2]                                                       # a fully covered pixel: the face's colour
    assert np.abs(rad[:, :8] - colour).max() <= 4 * EPS and np.abs(rad[:, 9:] - np.array(bg)).max() <= EPS
    assert np.abs(rad[:, 8] - (0.5 * colour + 0.5 * np.array(bg))).max() <= 4 * EPS


# ---- end to end ------------------------------------------------------------------------------------------------------

def _run_prepare(root, mesh_root, tag, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "prepare_dataset.py"), "--mesh_root", mesh_root,
           "--img_root", os.path.join(root, tag, "img"), "--pc_root", os.path.join(root, tag, "pc"),
           "--output", os.path.join(root, tag), "--views", "2", "--n_points", "2048", "--oversample", "2",
           "--train_classes", "chair", "sofa", "--test_classes", "cup", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def _mtimes(top):
    return {os.path.join(d, n): os.stat(os.path.join(d, n)).st_mtime_ns for d, _, names in os.walk(top) for n in names}


def test_prepare_dataset_makes_a_tree_the_few_shot_dataset_reads(gpu, tmp_path):
    root = str(tmp_path)
    shapes = [ref.cube(), ref.icosphere(1), ref.tetrahedron(), ref.icosphere(2)]

    def tree(name, labels):
        for li, label in enumerate(labels):
            for si, split in enumerate(("train", "test")):
                d = os.path.join(root, name, label, split)
                os.makedirs(d)
                for k in range(2):
                    v, f = shapes[(li + si + k) % 4]
                    v = v * np.float32(1 + li) + np.float32(k)              # off centre and of different sizes
                    with open(os.path.join(d, f"{label}_{2 * si + k:04d}.off"), "w") as fh:
                        fh.write(ref.off_text(v, f, fused=bool(k)))

    tree("meshes", ["chair", "sofa", "cup"])
    with open(os.path.join(root, "meshes", "sofa", "train", "broken.off"), "w") as fh:
        fh.write("OFF\n3 1 0\n0 0 0\n1 0 0\n2 0 0\n3 0 1 2\n")               # no area: reported and skipped
    out = _run_prepare(root, os.path.join(root, "meshes"), "a")
    assert "prepared 12 items, 24 views" in out.stdout and out.stdout.strip().endswith("skipped 1")
    assert "broken.off" in out.stderr
    before = _mtimes(os.path.join(root, "a", "img")) | _mtimes(os.path.join(root, "a", "pc"))
    assert len(before) == 12 * 2 + 12

    ds = datasets.FewShotModelNet(os.path.join(root, "a", "modelnet_train.txt"), os.path.join(root, "a", "modelnet_files"),
                                  1, 2, 2, transform=datasets.modelnet_transform())
    assert len(ds) == 8 and sorted(ds.reference) == ["chair", "cup", "sofa"]
    ep = ds[0]
    for key in ("xs", "xq", "xad"):
        assert ep[key].shape[1:] == (3, 224, 224) and ep[key].std() > 0.05   # images that are not constant
    for key in ("pcs", "pcq", "pcad"):
        assert ep[key].shape[1:] == (2048, 3)
        assert float(ep[key].norm(dim=-1).max()) <= 1 + 1e-5                 # in the unit ball
    assert len(open(os.path.join(root, "a", "modelnet_test.txt")).read().split("\n")) == 4

    out = _run_prepare(root, os.path.join(root, "meshes"), "a")             # nothing is rewritten
    assert "prepared 0 items, 0 views" in out.stdout
    after = _mtimes(os.path.join(root, "a", "img")) | _mtimes(os.path.join(root, "a", "pc"))
    assert after == before

    # another traversal: chair, which came first above, is not prepared at all -- the same clouds for the others
    _run_prepare(root, os.path.join(root, "meshes"), "b", extra=("--classes", "sofa", "cup"))
    compared = 0
    for path in _mtimes(os.path.join(root, "a", "pc")):
        other = path.replace(os.path.join(root, "a"), os.path.join(root, "b"))
        if os.sep + "chair" + os.sep not in path:
            assert open(path, "rb").read() == open(other, "rb").read(), path
            compared += 1
    assert compared == 8
