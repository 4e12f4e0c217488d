"""K31 on the device: vertex normals (K31a), the smooth shade pass (K31b), the decoder on a regular grid, and
``generate_meshes.py`` end to end.  Normals and radiance are compared bit for bit with the float32 restatement of the
header (``_mesh_smooth_ref.py``) and, against its float64 evaluation, with bounds derived from the header's operations;
face ids and depths are K27's."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import _mesh_ref as ref
import _mesh_smooth_ref as sref
import test_meshes_gpu as k27                     # its scenes and its views
import test_mesh_materials_gpu as k28            # its scene and texture helpers
import test_surface_cpu as host                   # the meshes whose bound the CPU suite checks
from fpsg_amd import _hip, meshes, surface
from fpsg_amd._hip import FpsgHipError

pytestmark = pytest.mark.gpu

EPS = sref.EPS
TOP, THREE = k27.TOP, k27.THREE
VIEWS = {"TOP": TOP, "THREE": THREE}
_same_bits = k28._same_bits


# ---- K31a: vertex normals ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(host.normal_shapes()))
def test_normals_equal_the_restatement_and_agree_with_float64(gpu, name):
    """Bit for bit the float32 restatement, and within ``_mesh_smooth_ref.normals_bound`` of the float64 one.  The bound is
    first order in eps = 2^-24 and follows the header's operations: an edge component is one rounding (eps |e|); a
    component p - q of a face's product carries 2 eps per product from the edges, eps from the product and eps (|p| + |q|)
    from the subtraction, 4 eps (|p| + |q|) together; the k sequential additions of a vertex add (k - 1) eps times the
    sum of the absolute components; the normalisation turns the sum's error ds into ds / |s| and adds 3.5 eps of its
    own.  Condition on the inputs, checked with the float64 reference in test_surface_cpu: the bound stays below 1e-4,
    so n.l moves by less than 1e-4, far under half a grey level (1/510)."""
    v, f = host.normal_shapes()[name]
    got = meshes.vertex_normals(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu))
    assert got.shape == v.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert _same_bits(got, sref.vertex_normals(v, f, np.float32))
    bound = sref.normals_bound(v, f)
    err = np.linalg.norm(got.astype(np.float64) - sref.vertex_normals(v, f, np.float64), axis=-1)
    print(f"{name}: largest |normal - float64| = {err.max():.3e} ({err.max() / EPS:.1f} eps), "
          f"bound {bound.max():.3e} ({bound.max() / EPS:.0f} eps)")
    assert bound.max() < 1e-4 and (err <= bound).all()
    # the table kept by the caller, int64 faces, the same bits on another run
    table = meshes.corner_table(f, v.shape[-2])
    again = meshes.vertex_normals(torch.from_numpy(v).to(gpu), torch.from_numpy(f).long().to(gpu), table)
    assert _same_bits(again.cpu().numpy(), got)


def test_a_mesh_whose_every_vertex_cancels_gives_zeros(gpu):
    v, f = ref.icosphere(1)
    both = np.stack([f, f[:, [0, 2, 1]]], axis=1).reshape(-1, 3)          # every face followed by its reverse
    extra = np.concatenate([both, [[0, 1, len(v)], [2, 2, 2]]]).astype(np.int32)   # out of range; no area
    got = meshes.vertex_normals(torch.from_numpy(v).to(gpu), torch.from_numpy(extra).to(gpu)).cpu().numpy()
    assert _same_bits(got, np.zeros_like(v))
    with pytest.raises(ValueError, match="table"):
        meshes.vertex_normals(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), (np.zeros(3, np.int32), np.zeros(1, np.int32)))


def test_a_lying_table_gives_no_access_outside_the_arrays(gpu):
    """The wrapper never builds such a table; this gives it to the C entry, once.  Offsets below 0, past the end and
    decreasing, face ids of F, -1 and the int32 extremes: the documented code (0: launched), normals that are unit
    vectors or zero, and the canaries around the output untouched."""
    lib = _hip.load()
    v, f = ref.icosphere(1)
    B, V, F = 2, len(v), len(f)
    n = 3 * F
    rng = np.random.default_rng(7)
    offsets = rng.integers(-50, n + 50, V + 1).astype(np.int32)
    offsets[:6] = [n + 100, -7, 2 ** 31 - 1, -2 ** 31, n, 0]
    offsets[-1] = 2 ** 31 - 1
    corner = rng.integers(0, F, n).astype(np.int32)
    corner[::5] = F
    corner[1::7] = -1
    corner[[3, 4]] = [2 ** 31 - 1, -2 ** 31]
    faces = f.copy()
    faces[5] = [0, 1, V]                                                  # and a face that is itself out of range
    tv = torch.from_numpy(np.stack([v, v * np.float32(2)])).to(gpu)
    tf, to, tc = (torch.from_numpy(a).to(gpu) for a in (faces, offsets, corner))
    pad = 64
    out = torch.full((pad + B * V * 3 + pad,), 777.0, dtype=torch.float32, device=gpu)
    rc = lib.fpsg_mesh_vertex_normals(_hip.ptr(tv), B, V, _hip.ptr(tf), F, _hip.ptr(to), _hip.ptr(tc), n,
                                      out.data_ptr() + 4 * pad, _hip.stream_of(tv))
    torch.cuda.synchronize()
    assert rc == 0
    assert (out[:pad] == 777.0).all() and (out[-pad:] == 777.0).all()
    length = out[pad:-pad].reshape(B, V, 3).double().norm(dim=-1)
    assert (((length - 1).abs() < 1e-6) | (length == 0)).all()


# ---- K31b: the smooth shade pass -----------------------------------------------------------------------------------------

def _params17(mat, bg):
    return np.concatenate([mat.params(bg), [mat.ambient, mat.diffuse]]).astype(np.float32)


def _cone_normals(v, f, seed, half_angle_deg=30.0, inward_every=3):
    """Corner normals [F,3,3] float32 within ``half_angle_deg`` of an axis per face: the face's own normal, or for every
    ``inward_every``-th face its negative (a normal that points away from the viewer of the face's front)."""
    rng = np.random.default_rng(seed)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    axis = np.cross(b - a, c - a)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    if inward_every:
        axis[::inward_every] *= -1
    r = rng.standard_normal((len(f), 3, 3))
    perp = r - (r * axis[:, None]).sum(-1, keepdims=True) * axis[:, None]
    perp /= np.linalg.norm(perp, axis=-1, keepdims=True)
    t = np.deg2rad(rng.uniform(0, half_angle_deg - 0.5, (len(f), 3, 1)))   # half a degree inside the cone: float32 rounding
    return (np.cos(t) * axis[:, None] + np.sin(t) * perp).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ball():
    v, f = ref.icosphere(2, radius=0.8)
    return v, f, _cone_normals(v, f, seed=11)


def _render(gpu, v, f, views, R, ssaa, scene=None, face_normals=None, **kw):
    fn = None if face_normals is None else torch.from_numpy(np.ascontiguousarray(face_normals, np.float32)).to(gpu)
    img, buf = meshes.render_views(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), size=R // ssaa, ssaa=ssaa,
                                   views=views, return_buffers=True, scene=scene, face_normals=fn, **kw)
    return img.cpu().numpy(), {k: t.cpu().numpy() for k, t in buf.items()}


def _pixel_bound(length, ssaa, params, shininess, normal_size):
    """The largest per-sample bound among an output pixel's covered samples (the resolve averages their errors); a pixel
    without one is the background's 14 eps."""
    per_sample = sref.smooth_bound(length, params, shininess, normal_size)
    NV, H, W = length.shape
    blocks = np.where(np.isnan(per_sample), 14 * EPS, per_sample).reshape(NV, H // ssaa, ssaa, W // ssaa, ssaa)
    return blocks.max(axis=(2, 4))


@pytest.mark.parametrize("R,ssaa,views", [(32, 1, "TOP"), (32, 2, "THREE"), (48, 1, "THREE"), (48, 2, "TOP")])
def test_smooth_radiance_equals_the_restatement_and_agrees_with_float64(gpu, R, ssaa, views):
    """face_id and depth are K27's; the radiance is the float32 restatement's bit for bit and within
    ``_mesh_smooth_ref.smooth_bound`` of the float64 one, per sample: K27's chain from the unit normal on, the unit
    normal's error coming from the interpolation (10.4 eps N), the turn into the camera frame (5.2 eps N) and the second
    normalisation, (15.6 eps N) / |m| + 3.5 eps.  Condition on the inputs: corner normals within a 30 degree cone per
    face, so |m| >= 0.866 N and |c.g| >= 0.866, and the largest bound stays below half a grey level."""
    v, f, fn = _ball()
    mat, bg = meshes.PhongMaterial(), (0.1, 0.55, 0.9)
    img0, buf0 = _render(gpu, v, f, VIEWS[views], R, ssaa, background=bg, material=mat)
    img, buf = _render(gpu, v, f, VIEWS[views], R, ssaa, face_normals=fn, background=bg, material=mat)
    assert _same_bits(buf["face_id"], buf0["face_id"]) and _same_bits(buf["depth"], buf0["depth"])
    assert not _same_bits(buf["radiance"], buf0["radiance"])
    fid = buf["face_id"]
    assert 0.2 < (fid >= 0).mean() < 0.9 and ((fid >= 0) & (fid % 3 == 0)).sum() > 20       # inward normals are seen too
    args = (v, f, VIEWS[views], 2.0, fid, ssaa, _params17(mat, bg), mat.log2_shininess(), fn, None, np.zeros((0, 4)), None, [])
    assert _same_bits(buf["radiance"], sref.shade_smooth(*args, np.float32))
    want, length = sref.shade_smooth(*args, np.float64, return_length=True)
    N = float(np.linalg.norm(fn.astype(np.float64), axis=-1).max())
    assert np.nanmin(length) >= 0.866 and N < 1 + 4 * EPS
    bound = _pixel_bound(length, ssaa, _params17(mat, bg), mat.shininess, N)
    err = np.abs(buf["radiance"].astype(np.float64) - want).max(axis=-1)
    print(f"{R}x{R} ssaa {ssaa} {views}: largest |radiance - float64| = {err.max():.3e} ({err.max() / EPS:.1f} eps), "
          f"largest bound {bound.max():.3e} ({bound.max() / EPS:.0f} eps), smallest |m| {np.nanmin(length):.4f}")
    assert bound.max() < 1 / 510
    assert (err <= bound).all()
    assert np.array_equal(img, np.rint(np.clip(buf["radiance"], 0, 1) * np.float32(255)).astype(np.uint8))
    assert want.max() - want.min() > 0.3


def _bent_grid(n=6, bend=0.8):
    v, f = ref.grid(n, n, -0.6, 0.6)
    v = v.copy()
    v[:, 2] = np.float32(bend) * v[:, 0] * v[:, 0]                       # a gutter along y: every cell stays planar
    return v, f


def _largest_step(radiance, fid):
    both = (fid[:, :, 1:] >= 0) & (fid[:, :, :-1] >= 0)
    step = np.abs(radiance[:, :, 1:].astype(np.float64) - radiance[:, :, :-1]).max(axis=-1)
    return float(step[both].max())


def test_k31a_normals_smooth_the_steps_between_the_facets_of_a_bent_grid(gpu):
    v, f = _bent_grid()
    tv, tf = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    normals = meshes.vertex_normals(tv, tf).cpu().numpy()
    _, flat = _render(gpu, v, f, TOP, 48, 1)
    _, smooth = _render(gpu, v, f, TOP, 48, 1, face_normals=normals[f])
    assert _same_bits(flat["face_id"], smooth["face_id"]) and (flat["face_id"] >= 0).sum() > 600
    flat_step, smooth_step = _largest_step(flat["radiance"], flat["face_id"]), _largest_step(smooth["radiance"], smooth["face_id"])
    print(f"largest step between horizontal neighbours: flat {flat_step:.4f}, smooth {smooth_step:.4f}")
    assert smooth_step < flat_step
    args = (v, f, TOP, 2.0, smooth["face_id"], 1, _params17(meshes.PhongMaterial(), (1, 1, 1)), 5, normals[f], None,
            np.zeros((0, 4)), None, [])
    assert _same_bits(smooth["radiance"], sref.shade_smooth(*args, np.float32))


def test_reversed_winding_with_its_normals_permuted_gives_the_same_radiance(gpu):
    v, f, fn = _ball()
    f2, fn2 = f.copy(), fn.copy()
    which = np.arange(0, len(f), 4)
    f2[which], fn2[which] = f[which][:, [0, 2, 1]], fn[which][:, [0, 2, 1]]
    _, a = _render(gpu, v, f, THREE, 48, 2, face_normals=fn)
    _, b = _render(gpu, v, f2, THREE, 48, 2, face_normals=fn2)
    assert np.isin(a["face_id"], which).sum() > 200
    for key in ("radiance", "face_id", "depth"):
        assert _same_bits(a[key], b[key]), key


def test_a_face_seen_from_behind_is_lit_through_the_flipped_normal(gpu):
    """Wound clockwise for the top camera, its corner normals the geometric ones, which point away from the camera: c is
    put on the camera's side, so the face is lit exactly as with the normals negated, and not just ambient."""
    v, f, _ = k28._quad((0, 1), (0, 1))
    f = f[:, [0, 2, 1]]
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    away = np.cross(b - a, c - a)
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    assert (away[:, 2] < -0.9).all()                                      # the top camera sits at +z and looks along -z
    fn = np.repeat(away[:, None], 3, axis=1).astype(np.float32)
    _, back = _render(gpu, v, f, TOP, 32, 1, face_normals=fn)
    _, front = _render(gpu, v, f, TOP, 32, 1, face_normals=-fn)
    assert _same_bits(back["radiance"], front["radiance"]) and (back["face_id"] >= 0).sum() == 24 * 24
    mat = meshes.PhongMaterial()
    lit = back["radiance"][0, 16, 16]
    assert (lit > 0.8 * (mat.ambient + 0.5 * mat.diffuse)).all()         # ambient alone would be 0.12
    _, flat = _render(gpu, v, f, TOP, 32, 1)
    assert np.abs(lit - flat["radiance"][0, 16, 16]).max() < 1e-5        # the normals are the face's: flat shading's colour


def _two_material_scene(gpu, n_faces, seed=2):
    tex = k28._textures(np.random.default_rng(seed), [(2, 2)])
    uv = np.random.default_rng(seed + 1).uniform(-1, 2, (n_faces, 3, 2)).astype(np.float32)
    face_material = np.arange(n_faces) % 3 - 1                            # none, Kd, texture, ...
    materials = [[0.9, 0.2, 0.1, -1], [0, 0, 0, 0]]
    return k28._scene(gpu, face_material, materials, uv, tex), face_material, np.asarray(materials, np.float32), uv, tex


@pytest.mark.parametrize("fill", ["zero", "nan"])
def test_normals_without_a_length_reproduce_k27_and_k28_bit_for_bit(gpu, fill):
    v, f, R = k27._scene("fan")
    bg = (0.1, 0.55, 0.9)
    fn = np.zeros((len(f), 3, 3), np.float32) if fill == "zero" else np.full((len(f), 3, 3), np.nan, np.float32)
    scene = _two_material_scene(gpu, len(f))[0]
    for what, sc in (("K27, M = 0", None), ("K28, two materials", scene)):
        img0, buf0 = _render(gpu, v, f, THREE, R, 2, sc, background=bg)
        img, buf = _render(gpu, v, f, THREE, R, 2, sc, face_normals=fn, background=bg)
        assert (buf0["face_id"] >= 0).sum() > 100
        assert _same_bits(img, img0), what
        for key in ("radiance", "face_id", "depth"):
            assert _same_bits(buf[key], buf0[key]), (what, key)
    _, k28_buf = _render(gpu, v, f, THREE, R, 2, scene, background=bg)
    _, k27_buf = _render(gpu, v, f, THREE, R, 2, None, background=bg)
    assert not _same_bits(k28_buf["radiance"], k27_buf["radiance"])      # the two yardsticks differ from each other


def test_materials_give_the_base_colour_and_the_normals_the_light(gpu):
    v, f, fn = _ball()
    scene, face_material, materials, uv, tex = _two_material_scene(gpu, len(f))
    mat, bg = meshes.PhongMaterial(shininess=8), (0.2, 0.2, 0.2)
    img, buf = _render(gpu, v, f, THREE, 48, 2, scene, face_normals=fn, background=bg, material=mat)
    _, flat = _render(gpu, v, f, THREE, 48, 2, scene, background=bg, material=mat)
    assert _same_bits(buf["face_id"], flat["face_id"]) and not _same_bits(buf["radiance"], flat["radiance"])
    args = (v, f, THREE, 2.0, buf["face_id"], 2, _params17(mat, bg), mat.log2_shininess(), fn, face_material, materials,
            uv, tex)
    assert _same_bits(buf["radiance"], sref.shade_smooth(*args, np.float32))
    want, length = sref.shade_smooth(*args, np.float64, return_length=True)
    # the texel lookup's own error is K28's (test_mesh_materials_gpu._lookup_bound), added to the light's
    bound = _pixel_bound(length, 2, _params17(mat, bg), mat.shininess, 1 + 4 * EPS) + \
        k28._lookup_bound(v, f, mat, 2, tex, uv) - k27._shading_bound(v, f, meshes.PhongMaterial(
            color=(1.0, 1.0, 1.0), ambient=mat.ambient, diffuse=mat.diffuse, specular=mat.specular,
            shininess=mat.shininess, light=mat.light), 2)
    err = np.abs(buf["radiance"].astype(np.float64) - want).max(axis=-1)
    print(f"materials: largest |radiance - float64| = {err.max():.3e}, largest bound {bound.max():.3e}")
    assert bound.max() < 1 / 510 and (err <= bound).all()
    assert np.array_equal(img, np.rint(np.clip(buf["radiance"], 0, 1) * np.float32(255)).astype(np.uint8))


def test_smooth_entry_refuses_bad_arguments_before_any_launch(gpu):
    lib = _hip.load()
    v, f, face_uv = k28._quad((0, 1), (0, 1))
    tv, tf = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    views = torch.from_numpy(TOP).to(gpu)
    fm = torch.zeros(2, dtype=torch.int32, device=gpu)
    uv = torch.from_numpy(face_uv).to(gpu)
    fn = torch.zeros((2 * 9 + 1,), dtype=torch.float32, device=gpu)
    texels = torch.zeros((10, 3), dtype=torch.uint8, device=gpu)
    image = torch.full((1, 32, 32, 3), 7, dtype=torch.uint8, device=gpu)
    face_id = torch.full((1, 32, 32), 12345, dtype=torch.int32, device=gpu)
    ws_bytes = lib.fpsg_mesh_render_smooth_workspace_bytes(4, 2, 1, 32, 32, 2, 2)
    ws = torch.full((ws_bytes // 16 + 1, 2), 99, dtype=torch.int64, device=gpu)
    params = (ctypes.c_float * 17)(*([0.5] * 17))

    def call(materials, table, normals, n_texels=10):
        m = np.asarray(materials, np.float32).reshape(-1, 4)
        t = np.asarray(table, np.int32).reshape(-1, 3)
        return lib.fpsg_mesh_render_smooth(
            _hip.ptr(tv), 4, _hip.ptr(tf), 2, _hip.ptr(fm), _hip.ptr(uv), normals,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(m), t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            len(t), _hip.ptr(texels), n_texels, _hip.ptr(views), 1, 32, 32, 1, ctypes.c_float(2.0), params, 5, None,
            _hip.ptr(image), None, _hip.ptr(face_id), None, _hip.ptr(ws), ws.numel() * 8, _hip.stream_of(tv))

    good_m, good_t = [[1, 0, 0, 1], [0, 1, 0, -1]], [[0, 2, 2], [4, 3, 2]]
    assert call(good_m, good_t, None) == -1 and b"fpsg_mesh_render_smooth: null pointer 'face_normals'" in lib.fpsg_last_error()
    assert call(good_m, good_t, fn.data_ptr() + 2) == -3 and b"'face_normals' not 4-byte aligned" in lib.fpsg_last_error()
    bad = [(([[1, 0, 0, 2], [0, 1, 0, -1]], good_t), b"texture index"),
           (([[1, 0, 0, 0.5], [0, 1, 0, -1]], good_t), b"texture index"),
           ((good_m, [[0, 2, 2], [5, 3, 2]]), b"reaches outside"),
           ((good_m, [[0, 0, 2], [4, 3, 2]]), b"reaches outside")]
    for (m, t), text in bad:
        assert call(m, t, fn.data_ptr()) == -2 and text in lib.fpsg_last_error(), (m, t)
    assert call(good_m, good_t, fn.data_ptr(), n_texels=meshes.RENDER_MAX_TEXELS + 1) == -4
    torch.cuda.synchronize()
    assert (image == 7).all() and (face_id == 12345).all() and (ws == 99).all()      # nothing ran, nothing was copied
    assert call(good_m, good_t, fn.data_ptr() + 4) == 0                               # the same call, all in order
    torch.cuda.synchronize()
    assert (face_id >= 0).sum() == 24 * 24 and not (image == 7).all()
    # the wrapper checks shape, dtype and device itself
    for bad_fn in (torch.zeros((2, 3, 2), device=gpu), torch.zeros((3, 3, 3), device=gpu), torch.zeros((2, 3, 3)),
                   np.zeros((2, 3, 3), np.float32)):
        with pytest.raises(ValueError, match="face_normals"):
            meshes.render_views(tv, tf, size=32, ssaa=1, views=TOP, face_normals=bad_fn)
    with pytest.raises(TypeError, match="face_normals"):
        meshes.render_views(tv, tf, size=32, ssaa=1, views=TOP, face_normals=torch.zeros((2, 3, 3), dtype=torch.float64, device=gpu))


# ---- the decoder on a regular grid ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model_and_sample():
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    gpu = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(default_options(device="cuda", n_shot=2, n_query=2)).to(gpu).eval()
    sample = synthetic_episode(2, 2, n_pts=2048, img_size=224, seed=3, device=gpu)
    with torch.no_grad():                                                 # reconstruct's encode
        xq, pcs = sample["xq"], sample["pcs"]
        img_z = model.img_encoder(xq.reshape(-1, *xq.shape[2:]))
        pc_z = model.pc_encoder(pcs.reshape(-1, *pcs.shape[2:]).transpose(2, 1))
        hidden = torch.cat([img_z, pc_z.mean(0, keepdim=True).expand(img_z.size(0), -1)], dim=1)
    return model, sample, hidden


def _count_calls(monkeypatch, names):
    lib, seen = _hip.load(), {name: 0 for name in names}
    for name in names:
        inner = getattr(lib, name)

        def spy(*args, _inner=inner, _name=name):
            seen[_name] += 1
            return _inner(*args)

        monkeypatch.setattr(lib, name, spy)
    return seen


@pytest.mark.parametrize("g,k9,fused_bn", [(4, 1, 0), (16, 1, 4), (6, 0, 5)])
def test_reconstruct_mesh_is_the_decoder_at_the_grids_points(gpu, monkeypatch, g, k9, fused_bn):
    """g = 4: K9 and, with rows of 2 * 16 columns, the library's BatchNorm; g = 16: K9 and K5 for the other four
    layers; g = 6: P = 36 is no size of K9's, the library chain with K5 for all five."""
    model, sample, hidden = _model_and_sample()
    dec = model.pc_decoder
    verts, faces = model.reconstruct_mesh(sample, grid=g)
    assert verts.shape == (2, 16 * g * g, 3) and verts.dtype == torch.float32 and verts.is_contiguous()
    assert faces.dtype == torch.int32 and faces.device == verts.device
    assert np.array_equal(faces.cpu().numpy(), surface.patch_faces(g, 16))
    assert torch.isfinite(verts).all() and verts.abs().max() <= 1
    seen = _count_calls(monkeypatch, ["fpsg_dec1_fwd", "fpsg_bn_act_fwd"])
    with torch.no_grad():
        direct = dec.decode_grid(hidden, g)
    print(f"g = {g}: first layer {dec.first_layer_path(hidden, g * g)}, launches {seen}")
    assert seen == {"fpsg_dec1_fwd": k9, "fpsg_bn_act_fwd": fused_bn}
    assert dec.first_layer_path(hidden, g * g) == ("K9" if k9 else "library")
    monkeypatch.undo()
    torch.testing.assert_close(verts, direct, rtol=1e-4, atol=1e-5)
    # vertex k of patch p against the decoder as it was, at its own patch size of 128: the grid's points in the first
    # columns of an injected grid, the rest drawn at random
    uv = torch.from_numpy(surface.regular_grid(g)).to(gpu)
    per_patch = verts.reshape(2, 16, g * g, 3)
    filler = torch.rand((2, 2, 128), generator=torch.Generator().manual_seed(g)).to(gpu)
    with torch.no_grad():
        for start in range(0, g * g, 128):
            cols = uv[:, start:start + 128]
            patch = filler.clone()
            patch[:, :, :cols.size(1)] = cols
            old = dec(hidden, grid=[[patch] * 4] * 4).reshape(2, 16, 128, 3)
            torch.testing.assert_close(per_patch[:, :, start:start + cols.size(1)], old[:, :, :cols.size(1)],
                                       rtol=1e-4, atol=1e-5)
        alone = dec.decode_grid(hidden[1:2], g)                           # a query on its own
    torch.testing.assert_close(alone, direct[1:2], rtol=1e-4, atol=1e-5)
    assert (per_patch.std(dim=2) > 1e-5).any()


def test_reconstruct_mesh_refuses_training_mode(gpu):
    model, sample, _ = _model_and_sample()
    model.pc_encoder.train()
    try:
        with pytest.raises(RuntimeError, match="evaluation mode"):
            model.reconstruct_mesh(sample, grid=4)
    finally:
        model.eval()
    with pytest.raises(ValueError, match="grid size"):
        model.reconstruct_mesh(sample, grid=65)


def test_mesh_sheet_has_the_layout_of_the_cloud_sheet(gpu):
    from fpsg_amd import visualization
    model, sample, _ = _model_and_sample()
    verts, faces = model.reconstruct_mesh(sample, grid=8)
    gt = sample["pcq"].squeeze(0)
    sheet = visualization.render_mesh_reconstruction(verts, faces, gt, 8, size=64)
    assert sheet.dtype == np.uint8 and sheet.shape == (2 * 64, 2 * 3 * 64, 3)
    right = sheet[:, 192:].reshape(-1, 3)
    assert (right.max(axis=1).astype(int) - right.min(axis=1)).max() <= 2              # ground truth: grey
    grey = visualization.render_reconstruction(verts, gt, None, size=64)
    assert np.array_equal(sheet[:, 192:], grey[:, 192:])                               # K29's half, as it draws it
    with pytest.raises(ValueError, match="grid"):
        visualization.render_mesh_reconstruction(verts, faces, gt, 7, size=64)


# ---- the tool --------------------------------------------------------------------------------------------------------------

def test_generate_meshes_end_to_end(gpu, tmp_path):
    from PIL import Image

    from fpsg_amd.visualization import PATCH_PALETTE
    model, _, _ = _model_and_sample()
    # an untrained decoder maps every patch to a speck: weigh the patch coordinates up until the patches have extent
    state = {k: t.clone() for k, t in model.state_dict().items()}
    for key, t in state.items():
        if key.endswith("deformer.conv1.weight"):
            t *= 10
        elif ".node_pool." in key and key.endswith("conv1.weight"):
            t[:, -3:] *= 400
    os.makedirs(tmp_path / "ckpt" / "0")
    torch.save(state, tmp_path / "ckpt" / "0" / "model.pt")

    def run(tag):
        cmd = [sys.executable, os.path.join(ROOT, "generate_meshes.py"), "--synthetic", "--n_shot", "2", "--n_query", "2",
               "--grid", "6", "--max_items", "2", "--model_path", str(tmp_path / "ckpt"), "--name", "0", "--eval_model",
               "model.pt", "--output", str(tmp_path / tag)]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        files = {os.path.relpath(os.path.join(d, n), tmp_path / tag): open(os.path.join(d, n), "rb").read()
                 for d, _, names in os.walk(tmp_path / tag) for n in names}
        return out.stdout, files

    stdout, files = run("a")
    print(stdout.strip().split("\n")[-1])
    assert "2 items x 2 queries, 576 vertices and 800 faces per mesh" in stdout and "first layer library" in stdout
    objs = sorted(n for n in files if n.endswith(".obj"))
    sheets = sorted(n for n in files if n.endswith(".png"))
    assert len(objs) == 4 and len(sheets) == 2 and len(files) == 6 + len({os.path.dirname(n) for n in objs})
    assert [os.path.basename(n) for n in objs] == ["00000_q0.obj", "00000_q1.obj", "00001_q0.obj", "00001_q1.obj"]
    for name in objs:
        assert os.path.join(os.path.dirname(name), "patches.mtl") in files
        scene = meshes.load_obj_scene(str(tmp_path / "a" / name))
        assert scene.warnings == [] and scene.verts.shape == (16 * 36, 3) and len(scene.materials) == 16
        assert np.array_equal(scene.faces, surface.patch_faces(6, 16))
        assert np.array_equal(scene.face_material, surface.patch_face_material(6, 16))
        assert files[name].count(b"\nvn ") == 16 * 36
    assert not np.array_equal(meshes.load_obj_scene(str(tmp_path / "a" / objs[0])).verts,
                              meshes.load_obj_scene(str(tmp_path / "a" / objs[1])).verts)
    for name in sheets:
        sheet = np.asarray(Image.open(tmp_path / "a" / name))
        assert sheet.shape == (2 * 192, 2 * 3 * 192, 3)
        left, right = sheet[:, :576].reshape(-1, 3).astype(int), sheet[:, 576:].reshape(-1, 3).astype(int)
        assert (right.max(axis=1) - right.min(axis=1)).max() <= 2                      # ground truth: grey
        coloured = left[(left.max(axis=1) - left.min(axis=1)) > 60]
        hue = np.argmin(((coloured[:, None, :] / np.maximum(coloured.max(axis=1), 1)[:, None, None]
                          - PATCH_PALETTE[None].astype(float) / PATCH_PALETTE.max(axis=1)[None, :, None]) ** 2).sum(-1), axis=1)
        assert len(coloured) > 200 and len(np.unique(hue)) > 1                         # more than one patch colour
    again, files_b = run("b")
    assert again.replace(str(tmp_path / "b"), "") == stdout.replace(str(tmp_path / "a"), "")
    assert files_b == files                                                            # byte for byte
