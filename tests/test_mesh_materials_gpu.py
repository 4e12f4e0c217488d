"""K28 on the device (materials and textures in the rendered views) and ``prepare_dataset.py --dataset shapenet`` end to
end.  Face ids and depths are K27's and are compared bit for bit; the radiance is compared bit for bit with the float32
restatement of the header (``_mesh_material_ref.py``) and, against its float64 evaluation, with a derived bound."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT

import _mesh_material_ref as mref
import _mesh_ref as ref
import test_meshes_gpu as k27                     # its scenes, its views and its shading bound
from fpsg_amd import _hip, datasets, meshes
from fpsg_amd._hip import FpsgHipError

pytestmark = pytest.mark.gpu

EPS = k27.EPS
TOP, THREE = k27.TOP, k27.THREE


def _textures(rng, sizes):
    """uint8 [h,w,3] textures with every texel different from every other, also across the textures."""
    n = sum(w * h for w, h in sizes)
    values = rng.permutation(256)[:n] if n <= 256 else rng.integers(0, 256, n)
    out, k = [], 0
    for w, h in sizes:
        r = values[k:k + w * h].astype(np.int64)
        out.append(np.stack([r, 255 - r, (r * 7 + 13) % 256], axis=1).astype(np.uint8).reshape(h, w, 3))
        k += w * h
    return out


def _pack(textures):
    table, offset = [], 0
    for t in textures:
        table.append((offset, t.shape[1], t.shape[0]))
        offset += t.shape[0] * t.shape[1]
    texels = np.concatenate([t.reshape(-1, 3) for t in textures]) if textures else np.zeros((0, 3), np.uint8)
    return np.asarray(table, np.int32).reshape(-1, 3), texels


def _scene(gpu, face_material, materials, face_uv, textures):
    table, texels = _pack(textures)
    return meshes.RenderScene(None if face_material is None else torch.from_numpy(np.asarray(face_material, np.int32)).to(gpu),
                              None if face_uv is None else torch.from_numpy(np.asarray(face_uv, np.float32)).to(gpu),
                              np.asarray(materials, np.float32).reshape(-1, 4), table,
                              torch.from_numpy(texels).to(gpu) if len(texels) else None)


def _render(gpu, v, f, views, R, ssaa, scene, **kw):
    img, buf = meshes.render_views(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), size=R // ssaa, ssaa=ssaa,
                                   views=views, return_buffers=True, scene=scene, **kw)
    return img.cpu().numpy(), {k: t.cpu().numpy() for k, t in buf.items()}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. faces without a material are K27's ---------------------------------------------------------------------------

@pytest.mark.parametrize("ssaa", [1, 2])
@pytest.mark.parametrize("name", ["shared_diagonal", "fan", "coincident"])
def test_bare_faces_equal_k27_bit_for_bit(gpu, name, ssaa):
    v, f, R = k27._scene(name)
    assert R == 32
    bg = (0.1, 0.55, 0.9)
    img0, buf0 = _render(gpu, v, f, THREE, R, ssaa, None, background=bg)
    assert (buf0["face_id"] >= 0).sum() > 100
    tex = _textures(np.random.default_rng(0), [(2, 2)])
    uv = np.random.default_rng(1).uniform(-1, 2, (len(f), 3, 2))
    scenes = {"M = 0": _scene(gpu, None, np.zeros((0, 4)), None, []),
              "materials that no face uses": _scene(gpu, np.full(len(f), -1), [[1, 0, 0, 0], [0, 1, 0, -1]], uv, tex),
              "indices outside [0, M)": _scene(gpu, np.where(np.arange(len(f)) % 2, 2, -7), [[1, 0, 0, 0], [0, 1, 0, -1]], uv, tex)}
    for what, scene in scenes.items():
        img, buf = _render(gpu, v, f, THREE, R, ssaa, scene, background=bg)
        assert _same_bits(img, img0), what
        for key in ("radiance", "face_id", "depth"):
            assert _same_bits(buf[key], buf0[key]), (what, key)


# ---- 2. the texel lookup -----------------------------------------------------------------------------------------------

R2 = 32


def _quad(u_range, v_range, lo=4.5, hi=28.5):
    """Two triangles facing the camera; the quad's corners are the centres of samples 4 and 28 of 32, so that a uv range
    of k (w / 2) over its 24 samples puts sample centres on texel centres and on texel edges."""
    (x0, y0), (x1, y1) = k27._pix(lo, hi, R2), k27._pix(hi, lo, R2)           # y0: bottom
    v = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0.25], [x0, y1, 0.25]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    (ua, ub), (va, vb) = u_range, v_range
    corner = np.array([[ua, va], [ub, va], [ub, vb], [ua, vb]], dtype=np.float32)
    return v, f, corner[f]


CASES = {
    # name: (texture sizes, materials [Kd, texture], face_material, u range, v range)
    "unit_1x1": ([(1, 1)], [[0.2, 0.4, 0.6, 0]], [0, 0], (0, 1), (0, 1)),
    "unit_2x2": ([(2, 2)], [[0, 0, 0, 0]], [0, 0], (0, 1), (0, 1)),
    "unit_3x5": ([(3, 5)], [[0, 0, 0, 0]], [0, 0], (0, 1), (0, 1)),
    "repeat_negative": ([(3, 5)], [[0, 0, 0, 0]], [0, 0], (-1.5, 2.5), (2.5, -1.5)),
    "texel_centres_and_integers": ([(3, 5)], [[0, 0, 0, 0]], [0, 0], (-2, 2), (0, 2.4)),   # tu w and tv h in steps of 1/2
    "two_textures": ([(2, 2), (3, 5)], [[0, 0, 0, 1], [1, 1, 1, 0]], [0, 1], (-0.3, 1.7), (0.2, 1.1)),
    "non_finite_uv": ([(2, 2)], [[0.9, 0.1, 0.3, 0]], [0, 0], (0, 1), (0, 1)),
    "kd_only": ([(2, 2)], [[0.3, 0.6, 0.9, -1], [0, 0, 0, 0]], [0, 1], (0, 1), (0, 1)),
}


def _lookup_bound(v, f, material, ssaa, textures, face_uv):
    """First-order bound on |fp32 radiance - float64 radiance| of a textured face, eps = 2^-24, for the operations the
    header lists (K28), on top of K27's bound (test_meshes_gpu._shading_bound):
      l_k = (float) E_k / (float) A2: three roundings, 3 eps l_k;  u = (l0 u0 + l1 u1) + l2 u2 with l_k >= 0 and
        l0 + l1 + l2 = 1 at a covered sample: 4 eps sum l_k |u_k| + 2 eps U <= 6 eps U, U the largest |u| or |v| of a corner;
      tu = u - floor(u): exact for u >= 0, one rounding of a number below 1 otherwise: + eps, as a point of the circle
        (a tu that wraps moves x by w, and the wrapped neighbours make that no step at all);
      x = tu w - 0.5: w (6 U + 1) eps carried, 2 eps w of its own;  y = (1 - tv) h - 0.5: one subtraction more; both
        are off by at most s (6 U + 4) eps, s the texture's larger side;
      b is linear between neighbouring texels, so a shift of (dx, dy) moves it by at most D (dx + dy), D the largest
        difference between horizontally or vertically neighbouring texels (the wrapped ones included), in [0, 1] units;
      its own arithmetic: byte / 255 eps, fx, gx and each weight 3 eps, four products, three additions: below 20 eps;
      colour: (ambient + diffuse) db, 2 eps for ambient b and diffuse b, then K27's bound for kd <= diffuse and
        ks (its material's colour set to white), which also holds the resolve's 14 eps."""
    U = np.abs(face_uv[np.isfinite(face_uv)]).max()
    db = 20 * EPS
    for t in textures:
        c = t.astype(np.float64) / 255
        D = max(np.abs(c - np.roll(c, 1, axis=0)).max(), np.abs(c - np.roll(c, 1, axis=1)).max())
        db = max(db, 2 * D * max(t.shape[:2]) * (6 * U + 4) * EPS + 20 * EPS)
    white = meshes.PhongMaterial(color=(1.0, 1.0, 1.0), ambient=material.ambient, diffuse=material.diffuse,
                                 specular=material.specular, shininess=material.shininess, light=material.light)
    return (material.ambient + material.diffuse) * db + 2 * EPS + k27._shading_bound(v, f, white, ssaa)


@functools.lru_cache(maxsize=None)
def _lookup_case(name, reverse=False):
    gpu = torch.device("cuda:0")
    sizes, materials, face_material, u_range, v_range = CASES[name]
    textures = _textures(np.random.default_rng(5), sizes)
    v, f, face_uv = _quad(u_range, v_range)
    if name == "non_finite_uv":
        face_uv[1, 2, 0] = np.inf
    if reverse:                                   # the second triangle the other way round, its uv with its corners
        f, face_uv = f.copy(), face_uv.copy()
        f[1], face_uv[1] = f[1, [0, 2, 1]], face_uv[1, [0, 2, 1]]
    mat = meshes.PhongMaterial()
    bg = (0.1, 0.55, 0.9)
    img, buf = _render(gpu, v, f, TOP, R2, 1, _scene(gpu, face_material, materials, face_uv, textures), background=bg,
                       material=mat)
    params = np.concatenate([mat.params(bg), [mat.ambient, mat.diffuse]]).astype(np.float32)
    args = (v, f, TOP, 2.0, buf["face_id"], 1, params, mat.log2_shininess(), face_material, materials, face_uv, textures)
    return v, f, mat, textures, face_uv, img, buf, args


@pytest.mark.parametrize("name", sorted(CASES))
def test_texel_lookup_equals_the_restatement(gpu, name):
    v, f, mat, textures, face_uv, img, buf, args = _lookup_case(name)
    want_id, want_depth, _ = ref.rasterize(v, f, TOP, 2.0, R2, R2)
    assert np.array_equal(buf["face_id"], want_id) and _same_bits(buf["depth"], want_depth)
    assert set(np.unique(want_id)) == {-1, 0, 1} and (want_id >= 0).sum() == 24 * 24
    want32 = mref.shade(*args, np.float32)
    want64 = mref.shade(*args, np.float64)
    rad = buf["radiance"]
    bound = _lookup_bound(v, f, mat, 1, textures, face_uv)
    err = np.abs(rad.astype(np.float64) - want64).max()
    differ = int((rad.view(np.uint32) != want32.view(np.uint32)).sum())
    print(f"{name}: |radiance - float64| = {err:.3e} ({err / EPS:.1f} eps), bound {bound:.3e} ({bound / EPS:.0f} eps); "
          f"{differ} of {rad.size} numbers differ from the float32 restatement")
    assert bound < 1 / 510                        # a bound above a grey level's half would test nothing
    assert err <= bound
    assert differ == 0
    assert np.array_equal(img, np.rint(np.clip(rad, 0, 1) * 255).astype(np.uint8))
    # what each case is there for
    covered = want_id[0] >= 0
    colours = len(np.unique(rad[0][covered].reshape(-1, 3), axis=0))
    if name == "unit_1x1":
        assert colours < 50 and np.ptp(rad[0][covered], axis=0).max() <= 8 * EPS     # one colour: the weights sum to 1 +- eps
    elif name in ("unit_2x2", "unit_3x5", "repeat_negative", "two_textures"):
        assert colours > 100                      # bilinear: a gradient, not texel-sized blocks
    elif name == "texel_centres_and_integers":
        # the premise: sample i of the quad's 24 has u = -2 + (i - 4) / 6, so x = tu w - 0.5 is an integer (a texel's
        # centre) or an integer and a half (a texel's edge) in turn, and u itself an integer every sixth sample; v likewise
        snapped = ref.project(v, TOP, 2.0, R2, R2)[1][0]
        u, vv, _ = mref.sample_uv(snapped, f.astype(np.int64), face_uv, want_id[0], np.float64)
        # (2.4 is not a float32: the corner's v is off by 1e-7, ten times that in tv h)
        assert np.abs(u * 6 - np.rint(u * 6))[covered].max() < 1e-9 and np.abs(vv * 10 - np.rint(vv * 10))[covered].max() < 2e-6
        assert (np.abs(u - np.rint(u)) < 1e-9)[covered].sum() == 4 * 24 and (np.abs(vv - np.rint(vv)) < 2e-6)[covered].sum() == 2 * 24
    elif name == "non_finite_uv":
        lit = mref.shade(*args[:9], [[0.9, 0.1, 0.3, -1]], *args[10:], np.float32)     # the same material without texture
        assert _same_bits(rad[0][want_id[0] == 1], lit[0][want_id[0] == 1])
        assert len(np.unique(rad[0][want_id[0] == 1].reshape(-1, 3), axis=0)) == 1
        assert len(np.unique(rad[0][want_id[0] == 0].reshape(-1, 3), axis=0)) > 50
    elif name == "kd_only":
        assert len(np.unique(rad[0][want_id[0] == 0].reshape(-1, 3), axis=0)) == 1


@pytest.mark.parametrize("name", ["repeat_negative", "two_textures"])
def test_reversed_winding_gives_the_same_colours(gpu, name):
    _, _, _, _, _, img, buf, _ = _lookup_case(name)
    v, f, _, _, _, img_r, buf_r, args = _lookup_case(name, reverse=True)
    assert f.tolist() == [[0, 1, 2], [0, 3, 2]]
    assert np.array_equal(buf_r["face_id"], buf["face_id"]) and _same_bits(buf_r["depth"], buf["depth"])
    assert _same_bits(buf_r["radiance"], buf["radiance"]) and np.array_equal(img_r, img)
    assert _same_bits(mref.shade(*args, np.float32), buf_r["radiance"])


# ---- 3. the resolve --------------------------------------------------------------------------------------------------

def test_half_covered_pixel_is_the_stated_mix_of_texture_and_background(gpu):
    size, ssaa = 16, 2
    R = size * ssaa
    (x0, y0), (x1, y1) = k27._pix(-4, -4, R), k27._pix(17, R + 4, R)        # the right edge between samples 16 and 17
    v = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    bg = (0.25, 0.5, 0.75)
    texel = np.array([[[255, 102, 0]]], dtype=np.uint8)
    uv = np.random.default_rng(2).uniform(-3, 3, (2, 3, 2))
    mat = meshes.PhongMaterial()
    _, buf = _render(gpu, v, f, TOP, R, ssaa, _scene(gpu, [0, 0], [[0, 0, 0, 0]], uv, [texel]), background=bg, material=mat)
    fid, rad = buf["face_id"][0], buf["radiance"][0].astype(np.float64)
    assert (fid[:, :17] >= 0).all() and (fid[:, 17:] < 0).all()             # output column 8: samples 16 (in), 17 (out)
    colour = rad[3, 2]                                                       # a fully covered pixel: the face's colour
    p = mat.params(bg).astype(np.float64)
    ndl = -p[11]                                                             # the face's normal is (0, 0, -1)
    spec = max(p[11] + 2 * ndl, 0.0) ** mat.shininess
    b = texel[0, 0] / 255.0
    want = mat.ambient * b + mat.diffuse * b * ndl + p[6:9] * spec
    # a 1 x 1 texture: its colour at every uv; 4 eps more for ambient, diffuse and the byte, which `want` does not round
    assert np.abs(colour - want).max() <= _lookup_bound(v, f, mat, ssaa, [texel], uv) + 4 * EPS
    assert colour[0] > 0.5 > colour[1] > colour[2]
    assert np.abs(rad[:, :8] - colour).max() <= 4 * EPS and np.abs(rad[:, 9:] - np.array(bg)).max() <= EPS
    assert np.abs(rad[:, 8] - (0.5 * colour + 0.5 * np.array(bg))).max() <= 4 * EPS


# ---- 4. refusals -----------------------------------------------------------------------------------------------------

def test_bad_tables_are_refused_before_any_launch(gpu):
    lib = _hip.load()
    v, f, face_uv = _quad((0, 1), (0, 1))
    tv, tf = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    views = torch.from_numpy(TOP).to(gpu)
    fm = torch.zeros(2, dtype=torch.int32, device=gpu)
    uv = torch.from_numpy(face_uv).to(gpu)
    texels = torch.zeros((10, 3), dtype=torch.uint8, device=gpu)
    image = torch.full((1, 32, 32, 3), 7, dtype=torch.uint8, device=gpu)
    face_id = torch.full((1, 32, 32), 12345, dtype=torch.int32, device=gpu)
    ws_bytes = lib.fpsg_mesh_render_materials_workspace_bytes(4, 2, 1, 32, 32, 2, 2)
    ws = torch.full((ws_bytes // 16 + 1, 2), 99, dtype=torch.int64, device=gpu)
    import ctypes
    params = (ctypes.c_float * 17)(*([0.5] * 17))

    def call(materials, table, n_texels=10, M=None, T=None):
        m = np.asarray(materials, np.float32).reshape(-1, 4)
        t = np.asarray(table, np.int32).reshape(-1, 3)
        return lib.fpsg_mesh_render_materials(
            _hip.ptr(tv), 4, _hip.ptr(tf), 2, _hip.ptr(fm), _hip.ptr(uv), m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            len(m) if M is None else M, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(t) if T is None else T,
            _hip.ptr(texels), n_texels, _hip.ptr(views), 1, 32, 32, 1, ctypes.c_float(2.0), params, 5, None,
            _hip.ptr(image), None, _hip.ptr(face_id), None, _hip.ptr(ws), ws.numel() * 8, _hip.stream_of(tv))

    good_m, good_t = [[1, 0, 0, 1], [0, 1, 0, -1]], [[0, 2, 2], [4, 3, 2]]
    bad = [(([[1, 0, 0, 2], [0, 1, 0, -1]], good_t), -2, b"texture index"),        # T = 2: 2 is outside
           (([[1, 0, 0, -2], [0, 1, 0, -1]], good_t), -2, b"texture index"),
           (([[1, 0, 0, 0.5], [0, 1, 0, -1]], good_t), -2, b"texture index"),
           (([[1, 0, 0, np.nan], [0, 1, 0, -1]], good_t), -2, b"texture index"),
           ((good_m, [[0, 2, 2], [5, 3, 2]]), -2, b"reaches outside"),               # 5 + 6 > 10
           ((good_m, [[-1, 2, 2], [4, 3, 2]]), -2, b"reaches outside"),
           ((good_m, [[0, 0, 2], [4, 3, 2]]), -2, b"reaches outside"),
           ((good_m, [[0, 65536, 65536], [4, 3, 2]]), -2, b"reaches outside")]      # w h beyond int32
    for (m, t), code, text in bad:
        assert call(m, t) == code and text in lib.fpsg_last_error(), (m, t)
    for kw in (dict(M=meshes.RENDER_MAX_MATERIALS + 1), dict(T=meshes.RENDER_MAX_TEXTURES + 1),
               dict(n_texels=meshes.RENDER_MAX_TEXELS + 1)):
        assert call(good_m, good_t, **kw) == -4, kw
    torch.cuda.synchronize()
    assert (image == 7).all() and (face_id == 12345).all() and (ws == 99).all()      # nothing ran, nothing was copied
    assert call(good_m, good_t) == 0                                                  # and the same call with good tables
    torch.cuda.synchronize()
    assert (face_id >= 0).sum() == 24 * 24 and not (image == 7).all()
    # through the wrapper the code arrives as FpsgHipError
    with pytest.raises(FpsgHipError, match="texture index"):
        meshes.render_views(tv, tf, size=32, ssaa=1, views=TOP, scene=meshes.RenderScene(fm, uv, np.float32([[1, 0, 0, 3]]),
                                                                                          np.int32([[0, 2, 2]]), texels))


# ---- 5. the tool, end to end -------------------------------------------------------------------------------------------

def _obj_text(v, f, uv_of_vertex, groups, mtllib):
    """groups: [(material name or None, first face, one past the last)]"""
    text = f"mtllib {mtllib}\n" + "".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist())
    text += "".join("vt %.9g %.9g\n" % tuple(t) for t in uv_of_vertex.tolist())
    for name, lo, hi in groups:
        if name:
            text += f"usemtl {name}\n"
        text += "".join("f %d/%d %d/%d %d/%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in f[lo:hi].tolist())
    return text


def _run_tool(root, tag, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "prepare_dataset.py"), "--dataset", "shapenet", "--mesh_root",
           os.path.join(root, "meshes"), "--pc_root", os.path.join(root, tag, "pc"), "--output", os.path.join(root, tag),
           "--size", "32", "--n_points", "64", "--views", "2", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def _files(top):
    return {os.path.relpath(os.path.join(d, n), top): open(os.path.join(d, n), "rb").read()
            for d, _, names in os.walk(top) for n in names}


def _covered(img):
    return (img != 255).any(axis=-1)                                        # the background is white


def test_prepare_dataset_shapenet_makes_a_tree_the_few_shot_dataset_reads(gpu, tmp_path):
    root = str(tmp_path)
    synsets = ("03001627", "03797390")                                       # chair (base), mug (novel)
    shapes = [ref.cube(), ref.icosphere(1), ref.tetrahedron()]
    rng = np.random.default_rng(0)
    for si, syn in enumerate(synsets):
        for k in range(3):
            d = os.path.join(root, "meshes", syn, f"item{si}{k}", "models")
            os.makedirs(os.path.join(d, "images"))                          # ShapeNet keeps textures in ../images or here
            v, f = shapes[k]
            uv = rng.uniform(0, 1, (len(v), 2))
            mtl = "newmtl skin\nKd 0 0 0\nmap_Kd images/tex.png\nnewmtl blue\nKd 0 0 1\nNs 5\nd 1\nillum 2\n"
            groups = [("skin", 0, len(f) // 2), ("blue", len(f) // 2, len(f))]
            if (si, k) == (0, 0):                                            # one plain red texture, nothing else
                Image.fromarray(np.tile(np.uint8([255, 0, 0]), (4, 4, 1))).save(os.path.join(d, "images", "tex.png"))
                groups = [("skin", 0, len(f))]
            elif (si, k) == (0, 1):                                          # the texture is missing: Kd, which is green
                mtl = mtl.replace("Kd 0 0 0", "Kd 0 1 0")
            else:
                Image.fromarray(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)).save(os.path.join(d, "images", "tex.png"))
            with open(os.path.join(d, "model_normalized.obj"), "w") as fh:
                fh.write(_obj_text(v, f, uv, groups, "model_normalized.mtl"))
            with open(os.path.join(d, "model_normalized.mtl"), "w") as fh:
                fh.write(mtl)
    broken = os.path.join(root, "meshes", synsets[1], "item12", "models", "model_normalized.obj")
    with open(broken, "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nf 1 2 nine\n")

    out = _run_tool(root, "a", ("--train_classes", synsets[0], "--test_classes", synsets[1]))
    assert "prepared 5 items, 10 views" in out.stdout and out.stdout.strip().endswith("skipped 1")
    assert "K28" in out.stdout and "textures" in out.stdout
    assert "skipped " + os.path.join(synsets[1], "item12") in out.stderr
    assert "warning:" in out.stderr and "tex.png" in out.stderr            # the missing texture is named
    pc = os.path.join(root, "a", "pc")
    first = _files(os.path.join(root, "a"))
    assert sum(n.endswith(".png") for n in first) == 10 and sum(n.endswith(".npy") for n in first) == 5
    cloud = np.load(os.path.join(pc, synsets[0], "item00", "models", "npy_file.npy"))
    assert cloud.shape == (64, 3) and cloud.dtype == np.float32 and np.abs(cloud).max() <= 0.5 + 1e-6     # on the cube, not normalised
    # the split files hold every item of the walk, the lists those that were made
    names = sorted(open(os.path.join(pc, f"{synsets[1]}_train.txt")).read().split() +
                   open(os.path.join(pc, f"{synsets[1]}_test.txt")).read().split())
    assert names == ["item10", "item11", "item12"]
    assert len(open(os.path.join(root, "a", "shapenet_train.txt")).read().split("\n")) == 3
    assert len(open(os.path.join(root, "a", "shapenet_test.txt")).read().split("\n")) == 2

    ds = datasets.FewShotShapeNet(os.path.join(root, "a", "shapenet_train.txt"), os.path.join(root, "a", "shapenet_files"),
                                  1, 1, 1, transform=datasets.ImageTransform(32))
    assert len(ds) == 3 and sorted(ds.reference) == list(synsets)
    ep = ds[0]
    assert ep["class"] == "chair" and ep["xs"].shape == (1, 3, 224, 224) and ep["pcs"].shape == (1, 2048, 3)

    def view(tag, item, k=0):
        return np.asarray(Image.open(os.path.join(root, tag, "pc", synsets[0], item, "models", "images", f"{item}.{k}.png")))

    for k in range(2):
        red = view("a", "item00", k)
        cov = _covered(red)
        assert cov.sum() > 100
        r, g, b = (red[cov][:, c].astype(int) for c in range(3))
        # red where covered: green and blue hold the highlight's share alone, the same in both; red holds the base colour
        # too.  Edge pixels mix with the white background, which raises all three: r >= g = b holds there as well
        assert (g == b).all() and (r >= g).all() and (r - g).max() > 100 and np.median(r - g) > 30
    green = view("a", "item01")                                              # the missing texture's Kd and the blue part
    assert ((green[..., 1].astype(int) - green[..., 0]) > 30).sum() > 20 and ((green[..., 2].astype(int) - green[..., 0]) > 30).sum() > 20

    out = _run_tool(root, "a", ("--train_classes", synsets[0], "--test_classes", synsets[1]))      # nothing is rewritten
    assert "prepared 0 items, 0 views" in out.stdout
    out = _run_tool(root, "a", ("--train_classes", synsets[0], "--test_classes", synsets[1], "--overwrite"))
    assert "prepared 5 items, 10 views" in out.stdout
    assert _files(os.path.join(root, "a")) == first                          # byte for byte

    _run_tool(root, "grey", ("--no_materials", "--classes", synsets[0]))
    for item in ("item00", "item01", "item02"):
        img = view("grey", item)
        assert (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all() and _covered(img).sum() > 60
    assert np.array_equal(np.load(os.path.join(root, "grey", "pc", synsets[0], "item00", "models", "npy_file.npy")), cloud)
