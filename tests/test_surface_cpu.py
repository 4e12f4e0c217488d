"""Generated shapes as meshes (K31), the host side: the patches' topology, the regular grid, the corner table K31a walks,
the restated normals, ``.obj`` files that ``load_obj_scene`` reads back, the decoder on an injected regular grid (looped
form, CPU) and what the two new C entries and the tool refuse without a device."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import _mesh_ref as ref
import _mesh_smooth_ref as sref
from fpsg_amd import meshes, surface
from fpsg_amd.point_cloud_net import PCDecoder
from fpsg_amd.visualization import patch_materials

EPS64 = 2.0 ** -53


# ---- topology ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [2, 3, 16])
def test_patch_faces_are_a_consistently_wound_manifold_grid_per_patch(g):
    n_patches = 3
    faces = surface.patch_faces(g, n_patches)
    per = 2 * (g - 1) ** 2
    assert faces.dtype == np.int32 and faces.shape == (n_patches * per, 3)
    assert faces.min() == 0 and faces.max() == n_patches * g * g - 1
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    # the stated faces of the first cell and of the last patch's first cell
    assert faces[0].tolist() == [0, g, 1] and faces[1].tolist() == [1, g, g + 1]
    assert faces[2 * per].tolist() == [2 * g * g, 2 * g * g + g, 2 * g * g + 1]
    material = surface.patch_face_material(g, n_patches)
    assert material.dtype == np.int32 and np.array_equal(material, np.arange(n_patches).repeat(per))
    assert np.array_equal(faces // (g * g), material[:, None].repeat(3, axis=1))       # no face leaves its patch
    # edges: every interior grid edge in two faces of its patch, boundary edges in one, none shared between patches
    edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    uniq, count = np.unique(edges, axis=0, return_counts=True)
    local = uniq % (g * g)
    i0, j0, i1, j1 = local[:, 0] // g, local[:, 0] % g, local[:, 1] // g, local[:, 1] % g
    on_boundary = ((i0 == i1) & ((i0 == 0) | (i0 == g - 1))) | ((j0 == j1) & ((j0 == 0) | (j0 == g - 1)))
    assert np.array_equal(count, np.where(on_boundary, 1, 2))
    assert len(uniq) == n_patches * (2 * g * (g - 1) + (g - 1) ** 2)                    # grid edges and diagonals
    assert (uniq[:, 0] // (g * g) == uniq[:, 1] // (g * g)).all()
    # one sign of area in (u, v)
    uv = np.tile(surface.regular_grid(g).T.astype(np.float64), (n_patches, 1))
    a, b, c = uv[faces[:, 0]], uv[faces[:, 1]], uv[faces[:, 2]]
    area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    assert (area < 0).all() or (area > 0).all()
    assert np.allclose(np.abs(area), 1.0 / (g - 1) ** 2, rtol=1e-6)


def test_regular_grid_has_exact_corners_and_refuses_other_sizes():
    for g in (2, 3, 7, 16, 64):
        uv = surface.regular_grid(g)
        assert uv.dtype == np.float32 and uv.shape == (2, g * g)
        assert uv[:, 0].tolist() == [0.0, 0.0] and uv[:, -1].tolist() == [1.0, 1.0]
        assert uv[:, g - 1].tolist() == [0.0, 1.0] and uv[:, g * (g - 1)].tolist() == [1.0, 0.0]
        k = 1 * g + (g - 1)                                                            # i = 1, j = g - 1
        assert uv[0, k] == np.float32(1.0 / (g - 1)) and uv[1, k] == 1.0
        assert uv.min() == 0.0 and uv.max() == 1.0
    for bad in (1, 65, 0, -3, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="grid size"):
            surface.regular_grid(bad)
    with pytest.raises(ValueError, match="grid size"):
        surface.patch_faces(1, 4)
    with pytest.raises(ValueError, match="n_patches"):
        surface.patch_faces(4, 0)


# ---- the corner table --------------------------------------------------------------------------------------------------

def _brute_table(faces, V):
    slices = [[f for f, tri in enumerate(faces.tolist()) if all(0 <= t < V for t in tri) for t in tri if t == v]
              for v in range(V)]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in slices])])
    return offsets, np.array([f for s in slices for f in s], dtype=np.int64)


def _table_cases():
    ico = ref.icosphere(1)[1]
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 9] for k in range(9)], dtype=np.int32)
    out_of_range = np.array([[0, 1, 2], [2, 3, 7], [1, 2, 3], [-1, 0, 1], [3, 2, 0]], dtype=np.int32)
    repeated = np.array([[0, 1, 2], [1, 1, 3], [2, 2, 2], [3, 0, 1]], dtype=np.int32)
    return {"icosphere": (ico, 42), "fan": (fan, 10), "out_of_range": (out_of_range, 5), "repeated": (repeated, 4),
            "isolated_vertices": (fan, 14)}


@pytest.mark.parametrize("name", sorted(_table_cases()))
def test_corner_table_equals_a_brute_force_scan(name):
    faces, V = _table_cases()[name]
    offsets, corner_faces = meshes.corner_table(faces, V)
    want_o, want_f = _brute_table(faces, V)
    assert offsets.dtype == np.int32 and corner_faces.dtype == np.int32 and offsets.shape == (V + 1,)
    assert np.array_equal(offsets, want_o) and np.array_equal(corner_faces, want_f)
    for v in range(V):
        assert (np.diff(corner_faces[offsets[v]:offsets[v + 1]]) >= 0).all()            # ascending inside every vertex
    if name == "out_of_range":
        assert len(corner_faces) == 9 and 1 not in corner_faces and 3 not in corner_faces
    if name == "repeated":
        assert corner_faces[offsets[1]:offsets[2]].tolist() == [0, 1, 1, 3]              # once per corner
        assert corner_faces[offsets[2]:offsets[3]].tolist() == [0, 2, 2, 2]
    same = meshes.corner_table(torch.from_numpy(faces).long(), V)                        # a tensor, another width
    assert np.array_equal(same[0], offsets) and np.array_equal(same[1], corner_faces)
    with pytest.raises(ValueError):
        meshes.corner_table(faces.astype(np.float32), V)
    with pytest.raises(ValueError):
        meshes.corner_table(faces, 0)


# ---- the restated normals ----------------------------------------------------------------------------------------------

def test_restated_normals_have_the_properties_one_can_check_by_hand():
    # an icosahedron's vertex normal is its direction: the five faces around a vertex are images of one another under
    # the rotations about its axis.  In float64, on float64 vertices, to within the rounding of about 40 operations:
    # normals_bound's formula with float64's unit roundoff in place of float32's, and 4 more for the direction itself
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v64 = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                    [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]])
    v64 = v64 / np.linalg.norm(v64, axis=1, keepdims=True) * 0.5
    f = ref.icosphere(0)[1]
    assert np.array_equal(v64.astype(np.float32), ref.icosphere(0)[0])                   # the project's icosahedron
    n = sref.vertex_normals(v64, f, np.float64)
    allowed = sref.normals_bound(v64, f) * (EPS64 / sref.EPS) + 4 * EPS64
    err = np.linalg.norm(n - v64 / 0.5, axis=1)
    print(f"icosahedron: normal - direction at most {err.max():.2e}, allowed {allowed.max():.2e} ({allowed.max() / EPS64:.0f} eps)")
    assert (err <= allowed).all() and allowed.max() < 64 * EPS64
    # a planar grid: (0, 0, +-1) exactly, in both dtypes, whatever the winding
    gv, gf = ref.grid(4, 3)
    for dtype in (np.float32, np.float64):
        up = sref.vertex_normals(gv, gf, dtype)
        down = sref.vertex_normals(gv, gf[:, [0, 2, 1]], dtype)
        assert up.dtype == dtype and np.array_equal(up, np.tile([0, 0, 1], (len(gv), 1)).astype(dtype))
        assert np.array_equal(down, -up)
    # a vertex of opposed faces, an isolated vertex and a vertex of a degenerate face give zero, not NaN
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 2, 2]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1], [4, 4, 4]], dtype=np.int32)
    for dtype in (np.float32, np.float64):
        assert np.array_equal(sref.vertex_normals(v, f, dtype), np.zeros((5, 3), dtype))
    # batched input is the meshes one by one; a face out of range contributes nothing
    both = np.stack([gv, gv[:, [1, 2, 0]]])
    got = sref.vertex_normals(both, gf, np.float32)
    assert np.array_equal(got[0], sref.vertex_normals(both[0], gf, np.float32))
    assert np.array_equal(got[1], sref.vertex_normals(both[1], gf, np.float32))
    extra = np.concatenate([gf, [[0, 1, len(gv)]]]).astype(np.int32)
    assert np.array_equal(sref.vertex_normals(gv, extra, np.float32), sref.vertex_normals(gv, gf, np.float32))


def saddle(n=5, jitter_seed=None):
    """An n x n-cell grid bent into a saddle z = 0.6 x y (and, with a seed, jittered by 1 % of a cell)."""
    v, f = ref.grid(n, n)
    v = v.copy()
    v[:, 2] = np.float32(0.6) * v[:, 0] * v[:, 1]
    if jitter_seed is not None:
        v += np.random.default_rng(jitter_seed).uniform(-0.002, 0.002, v.shape).astype(np.float32)
    return v, f


def normal_shapes():
    """The meshes of the GPU test of K31a: name -> (verts [V,3] or [B,V,3], faces)."""
    sv, sf = saddle()
    return {"icosphere": ref.icosphere(1), "cube": ref.cube(), "saddle": (sv, sf),
            "three_jittered_saddles": (np.stack([saddle(5, seed)[0] for seed in (1, 2, 3)]), sf)}


@pytest.mark.parametrize("name", sorted(normal_shapes()))
def test_the_gpu_tests_shapes_keep_the_normals_bound_below_1e_4(name):
    """The condition of the GPU test, checked here with the float64 reference: a normal off by less than 1e-4 moves n.l
    by less than 1e-4, far under half a grey level (1/510).  The bound is ``_mesh_smooth_ref.normals_bound``'s, a
    function of the shapes alone; the float32 restatement must itself be inside it."""
    v, f = normal_shapes()[name]
    bound = sref.normals_bound(v, f)
    n64, n32 = sref.vertex_normals(v, f, np.float64), sref.vertex_normals(v, f, np.float32)
    assert np.isfinite(bound).all() and np.abs(np.linalg.norm(n64, axis=-1) - 1).max() < 1e-12
    err = np.linalg.norm(n32.astype(np.float64) - n64, axis=-1)
    print(f"{name}: largest bound {bound.max():.3e} ({bound.max() / sref.EPS:.0f} eps), float32 restatement off by "
          f"{err.max():.3e}")
    assert bound.max() < 1e-4
    assert (err <= bound).all()


# ---- .obj files --------------------------------------------------------------------------------------------------------

def test_obj_round_trip_through_load_obj_scene(tmp_path):
    rng = np.random.default_rng(0)
    g, n_patches = 3, 5
    faces = surface.patch_faces(g, n_patches)
    verts = rng.standard_normal((n_patches * g * g, 3)).astype(np.float32)
    verts[0] = [np.float32(1) / np.float32(3), np.nextafter(np.float32(1), np.float32(2)), -1.5e-30]
    normals = sref.vertex_normals(verts, faces, np.float32)
    material = surface.patch_face_material(g, n_patches)
    materials = patch_materials(n_patches)
    path = str(tmp_path / "mesh.obj")
    meshes.write_obj_mesh(path, verts, faces, normals=normals, face_material=material, materials=materials,
                          mtl_name="patches.mtl")
    text = open(path).read()
    assert text.startswith("mtllib patches.mtl\n") and text.count("\nvn ") == len(verts) and text.count("\nusemtl ") == 5
    assert "\nf 1//1 4//4 2//2\n" in text
    scene = meshes.load_obj_scene(path)
    assert scene.warnings == []
    assert np.array_equal(scene.verts.view(np.uint32), verts.view(np.uint32))          # %.9g keeps every bit
    assert np.array_equal(scene.faces, faces) and scene.faces.dtype == np.int32
    assert np.array_equal(scene.face_material, material)
    kd = np.array([m.kd for m in scene.materials], dtype=np.float32)[scene.face_material]
    want = np.array([c for _, c in materials], dtype=np.float32)[material]
    assert np.array_equal(kd, want) and [m.name for m in scene.materials] == [f"patch_{p}" for p in range(5)]
    lines = [ln.split()[1:] for ln in text.split("\n") if ln.startswith("vn ")]
    assert np.array_equal(np.array(lines, dtype=np.float64).astype(np.float32).view(np.uint32), normals.view(np.uint32))
    # unordered materials: a usemtl per run, faces in their order; tensors; the default .mtl name
    mixed = np.array([1, 1, 0, 2, 2, 1] + [0] * (len(faces) - 6))
    path2 = str(tmp_path / "mixed.obj")
    meshes.write_obj_mesh(path2, torch.from_numpy(verts), torch.from_numpy(faces), face_material=torch.from_numpy(mixed),
                          materials=materials)
    scene = meshes.load_obj_scene(path2)
    assert os.path.isfile(tmp_path / "mixed.mtl") and scene.warnings == []
    assert np.array_equal(scene.face_material, mixed) and np.array_equal(scene.faces, faces)
    assert open(path2).read().count("usemtl") == 5
    # plain: no vn, no materials, faces 'f a b c'; load_mesh reads it too
    path3 = str(tmp_path / "plain.obj")
    meshes.write_obj_mesh(path3, verts, faces)
    text = open(path3).read()
    assert "vn" not in text and "mtllib" not in text and "//" not in text and "\nf 1 4 2\n" in text
    v3, f3 = meshes.load_mesh(path3)
    assert np.array_equal(v3.view(np.uint32), verts.view(np.uint32)) and np.array_equal(f3, faces)
    for kw in (dict(face_material=material), dict(materials=materials),
               dict(face_material=material + 1, materials=materials), dict(normals=normals[:-1])):
        with pytest.raises(ValueError):
            meshes.write_obj_mesh(str(tmp_path / "bad.obj"), verts, faces, **kw)
    with pytest.raises(ValueError, match="face indices"):
        meshes.write_obj_mesh(str(tmp_path / "bad.obj"), verts[:-1], faces)


# ---- the decoder on a regular grid (looped form, CPU) ------------------------------------------------------------------

def _decoder(template="SQUARE", batched=False):
    conf = types.SimpleNamespace(ori_dim=2, raw_dim=3, bottleneck_size=24, num_nodes=2, num_clusters=2, device="cpu",
                                 template_type=template, activation="relu")
    torch.manual_seed(3)
    dec = PCDecoder(conf, num_pts=64, batched=batched)
    with torch.no_grad():
        for m in dec.modules():                                  # running statistics that are not the initial ones
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return dec.eval()


def test_decode_grid_rows_are_the_decodes_of_their_single_points():
    dec = _decoder()
    g, G = 6, 4                                                  # P = 36, not the decoder's own 16
    hidden = torch.randn(3, 24, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        verts = dec.decode_grid(hidden, g)
        assert verts.shape == (3, G * g * g, 3) and verts.is_contiguous()
        uv = torch.from_numpy(surface.regular_grid(g))
        for k in range(g * g):
            one = uv[:, k].reshape(1, 2, 1).expand(3, 2, 1)
            single = dec(hidden, grid=[[one, one], [one, one]])                           # [3, G, 3]
            rows = verts.reshape(3, G, g * g, 3)[:, :, k]
            torch.testing.assert_close(rows, single, rtol=1e-4, atol=1e-5)
        own = dec(hidden, generator=torch.Generator().manual_seed(0))                     # the own patch size still works
        assert own.shape == (3, 64, 3)
    assert (verts.reshape(3, G, -1, 3).std(dim=2) > 1e-4).any()                          # the patches are not points


def test_decode_grid_refuses_training_mode_and_other_templates():
    dec = _decoder()
    hidden = torch.randn(2, 24)
    before = {k: v.clone() for k, v in dec.state_dict().items()}
    dec.train()
    with pytest.raises(RuntimeError, match="evaluation mode"):
        dec.decode_grid(hidden, 4)
    dec.eval()
    dec.cluster_pool[1].node_pool[0].bn2.train()                 # one module is enough
    with pytest.raises(RuntimeError, match="evaluation mode"):
        dec.decode_grid(hidden, 4)
    assert all(torch.equal(v, before[k]) for k, v in dec.state_dict().items())            # nothing ran
    with pytest.raises(ValueError, match="SPHERE"):
        _decoder("SPHERE").decode_grid(hidden, 4)
    with pytest.raises(ValueError, match="grid size"):
        _decoder().decode_grid(hidden, 1)


def test_batched_form_takes_the_patch_size_from_the_injected_grid():
    """On the CPU the batched form runs the library chain: the same arithmetic as the looped form, at a patch size that
    is not the decoder's own, and patches of different sizes in one call are refused."""
    looped, batched = _decoder(batched=False), _decoder(batched=True)
    batched.load_state_dict(looped.state_dict())
    hidden = torch.randn(2, 24, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        torch.testing.assert_close(batched.decode_grid(hidden, 5), looped.decode_grid(hidden, 5), rtol=1e-4, atol=1e-5)
        a, b = torch.rand(2, 2, 9), torch.rand(2, 2, 16)
        with pytest.raises(ValueError, match="one size"):
            batched(hidden, grid=[[a, a], [a, b]])


# ---- refusals without a device -----------------------------------------------------------------------------------------

def test_c_entries_refuse_bad_arguments_on_the_host():
    from fpsg_amd import _hip
    lib = _hip.load()

    def normals(B=2, V=8, F=4, n=12):
        return lib.fpsg_mesh_vertex_normals(None, B, V, None, F, None, None, n, None, None)

    assert normals() == -1 and b"fpsg_mesh_vertex_normals: null pointer" in lib.fpsg_last_error()
    for bad in (dict(B=0), dict(V=0), dict(F=-1), dict(n=-1), dict(n=13)):
        assert normals(**bad) == -2, bad
    for bad in (dict(B=65536), dict(V=(1 << 24) + 1), dict(F=(1 << 24) + 1, n=0)):
        assert normals(**bad) == -4, bad
    buf = (ctypes.c_float * 64)()
    at = ctypes.addressof(buf)
    assert lib.fpsg_mesh_vertex_normals(at, 1, 4, at, 2, at, at, 6, None, None) == -1     # normals
    assert lib.fpsg_mesh_vertex_normals(at, 1, 4, at, 2, at, None, 6, at, None) == -1     # corner_faces with n > 0
    assert lib.fpsg_mesh_vertex_normals(at, 1, 4, at, 2, at + 2, at, 6, at, None) == -3 and b"offsets" in lib.fpsg_last_error()
    assert lib.fpsg_mesh_vertex_normals(at, 1, 4, at, 2, at, at + 1, 6, at, None) == -3

    params = (ctypes.c_float * 17)()

    def smooth(M=0, T=0, n_texels=0, W=64, ssaa=1):
        return lib.fpsg_mesh_render_smooth(None, 8, None, 4, None, None, None, None, M, None, T, None, n_texels, None, 2,
                                           W, 64, ssaa, ctypes.c_float(2.0), params, 5, None, None, None, None, None,
                                           None, 0, None)

    assert smooth() == -1 and b"fpsg_mesh_render_smooth: null pointer" in lib.fpsg_last_error()
    for bad in (dict(M=-1), dict(T=-1), dict(n_texels=-1), dict(W=0), dict(ssaa=5)):
        assert smooth(**bad) == -2, bad
    for bad in (dict(M=meshes.RENDER_MAX_MATERIALS + 1), dict(T=meshes.RENDER_MAX_TEXTURES + 1), dict(W=8193)):
        assert smooth(**bad) == -4, bad
    # everything but face_normals in place: the null and the misaligned normals are what is refused
    space = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(space) + 15) & ~15

    def with_normals(fn):
        return lib.fpsg_mesh_render_smooth(at, 8, at, 4, None, None, fn, None, 0, None, 0, None, 0, at, 1, 8, 8, 1,
                                           ctypes.c_float(2.0), params, 5, None, at, None, None, None, base, 1 << 15, None)

    assert with_normals(None) == -1 and b"'face_normals'" in lib.fpsg_last_error()
    assert with_normals(at + 2) == -3 and b"'face_normals'" in lib.fpsg_last_error()
    k28 = lib.fpsg_mesh_render_materials_workspace_bytes(8, 4, 2, 64, 32, 3, 2)
    assert lib.fpsg_mesh_render_smooth_workspace_bytes(8, 4, 2, 64, 32, 3, 2) == k28 > 0
    assert lib.fpsg_mesh_render_smooth_workspace_bytes(8, 4, 2, 64, 32, -1, 0) == 0


def test_wrappers_refuse_bad_shapes_before_any_gpu_work():
    v, f = ref.cube()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    from fpsg_amd._hip import FpsgHipError
    with pytest.raises(FpsgHipError):
        meshes.vertex_normals(tv, tf)                                                    # CPU tensors: no fallback
    for bad_v, bad_f in ((tv[:, :2], tf), (tv.reshape(2, 2, 2, 3), tf), (tv, tf[:, :2]), (tv, tf.float())):
        with pytest.raises(ValueError):
            meshes.vertex_normals(bad_v, bad_f)


def test_the_tool_lists_its_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "generate_meshes.py"), "--help"], capture_output=True,
                         text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for flag in ("--grid", "--output", "--max_items", "--no_sheet", "--synthetic", "--eval_model", "--sample_up"):
        assert flag in out.stdout, flag
    out = subprocess.run([sys.executable, os.path.join(ROOT, "generate_meshes.py"), "--synthetic", "--grid", "65"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode != 0 and "--grid" in out.stderr and "2 to 64" in out.stderr
