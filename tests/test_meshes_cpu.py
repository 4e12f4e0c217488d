"""Datasets from meshes, what needs no GPU: mesh files in and clouds out (``fpsg_amd.meshes``), the numpy restatement of
K26 / K27 against properties it must have (so that the GPU tests' yardstick is trusted), the list files, the C entries'
refusals, and ``prepare_dataset.py``'s command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import _mesh_ref as ref
from fpsg_amd import datasets, meshes


# ---- 1. files -------------------------------------------------------------------------------------------------------

def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


QUAD_OFF = """# a comment first
OFF
# counts
5 2 0

0 0 0
1 0 0   # trailing comment
1 1 0
0 1 0

0.5 0.5 1
4 0 1 2 3
5 0 1 2 3 4 255 0 0
"""


def test_off_with_comments_blank_lines_quads_and_ngons(tmp_path):
    v, f = meshes.load_mesh(_write(tmp_path, "q.off", QUAD_OFF))
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == (5, 3)
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]]       # fans; the colour is ignored
    assert v[4].tolist() == [0.5, 0.5, 1.0]


@pytest.mark.parametrize("fused", [False, True])
def test_off_normal_and_fused_header(tmp_path, fused):
    v0, f0 = ref.icosphere(1)
    text = ref.off_text(v0, f0, fused=fused)
    assert text.startswith("OFF42 80 0" if fused else "OFF\n42 80 0")
    v, f = meshes.load_mesh(_write(tmp_path, "s.off", text))
    assert np.array_equal(v, v0) and np.array_equal(f, f0)


def test_off_counts_on_the_keyword_line(tmp_path):
    v, f = meshes.load_mesh(_write(tmp_path, "t.off", "OFF 3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n"))
    assert v.shape == (3, 3) and f.tolist() == [[0, 1, 2]]


def test_obj_with_parts_negative_indices_and_ignored_records(tmp_path):
    text = """mtllib x.mtl
o thing
v 0 0 0
v 1 0 0
vt 0 0
vn 0 0 1
v 1 1 0
f 1/1/1 2/1/1 3/1/1
v 0 1 0
s off
usemtl m
f -4//1 -2//1 -1//1
f 1 2 3 4
vp 1 2
"""
    v, f = meshes.load_mesh(_write(tmp_path, "m.obj", text))
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3]]


def test_negative_obj_index_counts_from_the_vertices_seen_so_far(tmp_path):
    text = "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\nv 5 5 5\nf -3 -2 -1\n"
    _, f = meshes.load_mesh(_write(tmp_path, "n.obj", text))
    assert f.tolist() == [[0, 1, 2], [1, 2, 3]]


def test_out_of_range_index_raises_with_file_and_line(tmp_path):
    p = _write(tmp_path, "bad.off", "OFF\n3 2 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n3 0 1 3\n")
    with pytest.raises(ValueError, match=r"bad\.off, line 7.*out of range"):
        meshes.load_mesh(p)
    p = _write(tmp_path, "bad.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 2 4\n")
    with pytest.raises(ValueError, match=r"bad\.obj, line 5.*out of range"):
        meshes.load_mesh(p)
    p = _write(tmp_path, "zero.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")
    with pytest.raises(ValueError, match="line 4"):
        meshes.load_mesh(p)
    with pytest.raises(ValueError, match="unsupported"):
        meshes.load_mesh(_write(tmp_path, "x.stl", ""))


def test_ply_points_round_trip_through_the_dataset_reader(tmp_path):
    rng = np.random.default_rng(0)
    pts = (rng.standard_normal((300, 3)) * np.array([1e-3, 1.0, 1e3])).astype(np.float32)
    p = str(tmp_path / "c.ply")
    meshes.write_ply_points(p, pts)
    back = np.asarray(datasets.ply_reader(p), dtype=np.float32)
    assert back.shape == (300, 3) and np.array_equal(back, pts)              # %.9g keeps every bit
    assert np.asarray(datasets.ply_reader(p, max_verts=7)).shape == (7, 3)
    meshes.write_ply_points(p, torch.from_numpy(pts[:5]))
    assert np.array_equal(np.asarray(datasets.ply_reader(p), dtype=np.float32), pts[:5])


def test_normalize_mesh_on_an_off_centre_box():
    v, _ = ref.cube()
    v = v * np.array([4.0, 2.0, 1.0], dtype=np.float32) + np.array([10.0, -3.0, 7.0], dtype=np.float32)
    n = meshes.normalize_mesh(v)
    assert n.dtype == np.float32
    assert np.allclose(n.min(axis=0), [-0.5, -0.25, -0.125]) and np.allclose(n.max(axis=0), [0.5, 0.25, 0.125])
    assert np.array_equal(meshes.normalize_mesh(v, "none"), v)
    with pytest.raises(ValueError):
        meshes.normalize_mesh(v, "sphere")


# ---- 2. the restatement of K26 ---------------------------------------------------------------------------------------

def _square():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def _wide_areas():
    """Right triangles whose areas span 10^6 : 1, plus two zero-area faces."""
    sides = np.array([1.0, 1e-3, 0.37, 3e-2, 1e-3, 0.9, 5e-3], dtype=np.float32)
    v, f = [], []
    for k, s in enumerate(sides):
        o = np.float32(2.0 * k)
        v += [[o, 0, 0], [o + s, 0, 0], [o, s, 0]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    f += [[0, 0, 1], [0, 1, 1]]
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


@pytest.mark.parametrize("mesh", ["square", "wide"])
def test_stratified_face_counts_follow_the_areas(mesh):
    v, f = _square() if mesh == "square" else _wide_areas()
    area = ref.areas(v, f).astype(np.float64)
    if mesh == "wide":
        assert area[area > 0].max() / area[area > 0].min() >= 1e6 - 1
    _, C = ref.weights(v, f)
    for n in (64, 1000, 4096, 100003):
        u0 = ((np.arange(n) + 0.5) / n).astype(np.float32)
        counts = np.bincount(ref.choose_faces(C, u0), minlength=len(f))
        want = n * area / area.sum()
        assert np.abs(counts - want).max() <= 1, (n, counts, want)             # as for any inverse-CDF rule
        assert counts[area == 0].sum() == 0


def test_zero_area_faces_have_no_weight_and_are_never_chosen():
    v, f = _wide_areas()
    v = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 0, 0]]]).astype(np.float32)
    f = np.concatenate([f, [[0, 1, len(v) - 2], [0, 1, len(v) - 1]]]).astype(np.int32)
    q, C = ref.weights(v, f)
    assert (q[7:] == 0).all() and q.max() == 2 ** 32 and C[-1] == q.sum()
    rng = np.random.default_rng(1)
    u0 = np.concatenate([[0.0, np.nextafter(np.float32(1), np.float32(0))], rng.random(5000)]).astype(np.float32)
    chosen = ref.choose_faces(C, u0)
    assert (q[chosen] > 0).all() and chosen[0] == 0 and chosen[1] == 6


def test_every_sample_lies_in_its_triangle():
    v, f = ref.icosphere(2)
    rng = np.random.default_rng(2)
    u = rng.random((20000, 3)).astype(np.float32)
    u[:4] = [[0, 0, 0], [0.5, 1 - 2.0 ** -24, 0], [0.5, 1 - 2.0 ** -24, 1 - 2.0 ** -24], [0.25, 0, 1 - 2.0 ** -24]]
    pts, fidx = ref.sample(v, f, u)
    bary, dist = ref.barycentric64(v, f, pts, fidx)
    assert bary.min() >= -1e-6 and dist.max() <= 1e-6 * 1.0                 # the sphere's extent is 1
    assert len(np.unique(fidx)) == len(f)


# ---- 3. the restatement of K27 ---------------------------------------------------------------------------------------

TOP = meshes.camera_views(0.0, [0.0])            # theta = 0: right = +x, up = +y, looking down -z


def _pix(i, j, R):
    """The world (x, y) that the top view at ortho_scale 2 puts on pixel coordinate (i, j) of an R x R image."""
    return (i / R - 0.5) * 2.0, (0.5 - j / R) * 2.0


def test_top_view_camera_and_the_twelve_views():
    assert np.allclose(TOP[0], [1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 3], atol=1e-7)
    m = meshes.camera_views()
    assert m.shape == (12, 12) and m.dtype == np.float32
    for row in m.astype(np.float64):
        r, u, f, c = row[0:3], row[3:6], row[6:9], row[9:12]
        assert np.allclose([r @ r, u @ u, f @ f], 1, atol=1e-6) and np.allclose([r @ u, r @ f, u @ f], 0, atol=1e-6)
        assert np.allclose(np.cross(r, u), -f, atol=1e-6)                    # x right, y up, looking along +z
        assert np.allclose(np.linalg.norm(c), 3, atol=1e-6) and np.allclose(c[2], 1.5, atol=1e-6)
        assert u[2] > 0
    y = meshes.camera_views(60.0, [0.0], up="y")[0]
    assert np.allclose(y[9:12], [0, 1.5, 3 * np.sin(np.pi / 3)], atol=1e-6) and y[4] > 0


def test_square_of_two_triangles_sharing_a_diagonal_covers_every_pixel_once():
    R = 16
    x0, y0 = _pix(3, 3, R)
    x1, y1 = _pix(11, 11, R)                     # vertices on pixel corners: the diagonal runs through pixel centres
    v = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], dtype=np.float32)
    for f in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 2, 3]], [[1, 2, 3], [1, 3, 0]]):
        fid, depth, hits = ref.rasterize(v, np.asarray(f), TOP, 2.0, R, R)
        want = np.zeros((R, R), np.int32)
        want[3:11, 3:11] = 1
        assert np.array_equal(hits[0], want)
        assert (fid[0][want == 1] >= 0).all() and (fid[0][want == 0] == -1).all()
        assert np.array_equal(depth[0][want == 1], np.full(64, 3.0, np.float32))


def test_fan_of_64_triangles_around_a_vertex_on_a_pixel_centre_is_watertight():
    R = 32
    cx, cy = _pix(16.5, 15.5, R)                 # a pixel centre
    ang = np.linspace(0, 2 * np.pi, 64, endpoint=False) + 0.01
    rim = np.stack([cx + 0.7 * np.cos(ang), cy + 0.7 * np.sin(ang), np.zeros(64)], axis=1)
    v = np.concatenate([[[cx, cy, 0.0]], rim]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % 64] for k in range(64)], dtype=np.int32)
    f[::3] = f[::3][:, [0, 2, 1]]                # mixed windings
    _, snapped, _ = ref.project(v, TOP, 2.0, R, R)
    assert tuple(snapped[0, 0]) == (256 * 16 + 128, 256 * 15 + 128)
    fid, _, hits = ref.rasterize(v, f, TOP, 2.0, R, R)
    assert hits.max() == 1                       # none double-counted
    jj, ii = np.mgrid[0:R, 0:R]
    px, py = _pix(ii + 0.5, jj + 0.5, R)
    inside = (px - cx) ** 2 + (py - cy) ** 2 < (0.7 * np.cos(np.pi / 64) - 1e-3) ** 2
    assert (hits[0][inside] == 1).all() and hits[0, 15, 16] == 1            # none missed, the centre pixel included
    assert inside.sum() > 300


def test_nearest_face_wins_and_the_lower_index_on_equal_depth():
    R = 8
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-1, -1, 0.5], [1, -1, 0.5], [1, 1, 0.5]],
                 dtype=np.float32)
    f = np.array([[0, 1, 2], [2, 1, 0], [4, 5, 6], [0, 2, 3]], dtype=np.int32)
    fid, depth, hits = ref.rasterize(v, f, TOP, 2.0, R, R)
    assert hits.max() == 3 and set(np.unique(fid)) == {2, 3}
    assert np.array_equal(np.unique(depth[0][fid[0] == 2]), [2.5])          # z = 0.5 is nearer the camera at z = 3
    fid2, _, _ = ref.rasterize(v, f[[0, 1, 3]], TOP, 2.0, R, R)
    assert set(np.unique(fid2)) == {0, 2} and (fid2[0] == 0).sum() + (fid2[0] == 2).sum() == R * R


# ---- 4. list files ---------------------------------------------------------------------------------------------------

def _placeholder_tree(root, classes, views=("b.1.png", "b.0.png", "b.10.png")):
    for label, items in classes.items():
        for split, names in items.items():
            for item in names:
                d = os.path.join(root, "img", label, split, item)
                os.makedirs(d, exist_ok=True)
                for vname in views:
                    open(os.path.join(d, vname.replace("b.", item + ".")), "w").close()
                os.makedirs(os.path.join(root, "pc", label, split), exist_ok=True)
                open(os.path.join(root, "pc", label, split, item + ".ply"), "w").close()


def test_write_modelnet_lists_on_placeholder_files(tmp_path):
    root = str(tmp_path)
    _placeholder_tree(root, {"chair": {"train": ["chair_2", "chair_1"], "test": ["chair_9"]},
                             "cup": {"train": ["cup_1"], "test": ["cup_2"]},
                             "xbox": {"train": ["xbox_1"]},
                             "sofa": {"train": ["sofa_1"]}})
    os.makedirs(os.path.join(root, "img", "sofa", "test", "sofa_empty"))    # an item without views is left out
    img, pc, out = (os.path.join(root, d) for d in ("img", "pc", "out"))
    res = meshes.write_modelnet_lists(img, pc, out)
    assert res == {"train": 4, "test": 2, "classes": ["chair", "cup", "sofa"]}

    def line(label, split, item):
        return f"{img}/{label}/{split}/{item}/{item}.0.png\t{pc}/{label}/{split}/{item}.ply"

    train = open(os.path.join(out, "modelnet_train.txt")).read()
    assert train == "\n".join([line("chair", "train", "chair_1"), line("chair", "train", "chair_2"),
                               line("chair", "test", "chair_9"), line("sofa", "train", "sofa_1")])
    test = open(os.path.join(out, "modelnet_test.txt")).read()
    assert test == "\n".join([line("cup", "train", "cup_1"), line("cup", "test", "cup_2")])
    assert sorted(os.listdir(os.path.join(out, "modelnet_files"))) == ["modelnet+chair.txt", "modelnet+cup.txt",
                                                                      "modelnet+sofa.txt"]
    cup = open(os.path.join(out, "modelnet_files", "modelnet+cup.txt")).read()
    assert cup == test and not cup.endswith("\n")
    # the lines are what the dataset classes split: '<img>\t<pc>', the label fourth from the end of the image path
    assert train.split("\n")[0].split("\t")[0].split("/")[-4] == "chair"
    res = meshes.write_modelnet_lists(img, pc, out, train_classes=["xbox"], test_classes=["sofa", "xbox"])
    assert res == {"train": 0, "test": 2, "classes": ["sofa", "xbox"]}       # a novel class wins over a base class
    assert open(os.path.join(out, "modelnet_train.txt")).read() == ""
    assert meshes.MODELNET_TRAIN_CLASSES == ("airplane", "bathtub", "bed", "chair", "desk", "dresser", "monitor", "sofa",
                                             "table", "toilet")
    assert meshes.MODELNET_TEST_CLASSES == ("cup", "keyboard", "door", "laptop", "bowl")


# ---- 5. the C entries and the wrappers without a device -------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    import ctypes
    assert lib.fpsg_mesh_cdf(None, 0, None, 4, None, None, 0, None) == -2
    assert lib.fpsg_mesh_cdf(None, 8, None, (1 << 24) + 1, None, None, 0, None) == -4
    assert lib.fpsg_mesh_cdf(None, 8, None, 4, None, None, 0, None) == -1
    assert lib.fpsg_mesh_cdf_workspace_bytes(8, 5000) == 8 + 5 * 8 + 5000 * 4
    assert lib.fpsg_mesh_cdf_workspace_bytes(8, (1 << 24) + 1) == 0 and lib.fpsg_mesh_cdf_workspace_bytes(0, 4) == 0
    assert lib.fpsg_mesh_sample(None, 8, None, 4, None, 0, None, 16, None, None, None) == -2
    assert b"no area" in lib.fpsg_last_error()
    assert lib.fpsg_mesh_sample(None, 8, None, 4, None, (4 << 32) + 1, None, 16, None, None, None) == -2
    assert lib.fpsg_mesh_sample(None, 8, None, 4, None, 1 << 32, None, 0, None, None, None) == -2
    assert lib.fpsg_mesh_sample(None, 8, None, 4, None, 1 << 32, None, 16, None, None, None) == -1
    f = ctypes.c_float
    params = (ctypes.c_float * 15)()

    def render(V=8, F=4, NV=2, W=64, H=64, ssaa=1, ortho=2.0, log2s=5):
        return lib.fpsg_mesh_render(None, V, None, F, None, NV, W, H, ssaa, f(ortho), params, log2s, None, None, None,
                                    None, None, None, 0, None)

    assert render() == -1
    for bad in (dict(V=0), dict(F=0), dict(NV=0), dict(W=0), dict(ssaa=0), dict(ssaa=5), dict(W=66, ssaa=4),
                dict(ortho=0.0), dict(ortho=float("inf")), dict(log2s=-1), dict(log2s=11)):
        assert render(**bad) == -2, bad
    for bad in (dict(W=8193, H=8193), dict(NV=1025), dict(F=1 << 24, NV=1024)):
        assert render(**bad) == -4, bad
    assert lib.fpsg_mesh_render_workspace_bytes(8, 4, 2, 64, 32) == 2 * 8 * 32 + 2 * 64 * 32 * 8 + 32 + 16
    assert lib.fpsg_mesh_render_workspace_bytes(8, 4, 2, 8193, 32) == 0


def test_mesh_render_refusals_their_codes_and_their_prefix(lib):
    """``fpsg_mesh_render``'s own refusals, all in front of the first launch, so made-up aligned addresses do.  The
    codes are those the library returned when the entry still had its own copy of the checks."""
    import ctypes
    params = (ctypes.c_float * 15)()
    need = lib.fpsg_mesh_render_workspace_bytes(8, 4, 2, 64, 64)
    good = dict(verts=0x1000, V=8, faces=0x2000, W=64, ssaa=1, image=0x5000, radiance=None, ws=0x10000, ws_bytes=need)

    def render(**kw):
        a = {**good, **kw}
        rc = lib.fpsg_mesh_render(a["verts"], a["V"], a["faces"], 4, 0x3000, 2, a["W"], 64, a["ssaa"], ctypes.c_float(2.0),
                                  params, 5, None, a["image"], a["radiance"], None, None, a["ws"], a["ws_bytes"], None)
        assert lib.fpsg_last_error().startswith(b"fpsg_mesh_render:"), lib.fpsg_last_error()
        return rc, lib.fpsg_last_error()

    for kw, code, text in [(dict(V=0), -2, b"must be positive"),
                           (dict(W=66, ssaa=4), -2, b"a divisor of W and H"),
                           (dict(verts=None), -1, b"null pointer 'verts'"),
                           (dict(radiance=0x6002), -3, b"an output is not 4-byte aligned"),
                           (dict(image=None), -1, b"no output requested"),
                           (dict(ws=0x10008), -3, b"'ws' must be 16-byte aligned"),
                           (dict(ws_bytes=need - 1), -2, b"workspace of %d bytes, %d needed" % (need - 1, need))]:
        rc, message = render(**kw)
        assert rc == code and text in message, (kw, rc, message)


def test_wrappers_have_no_cpu_fallback_and_check_shapes_first():
    from fpsg_amd._hip import FpsgHipError
    v, f = ref.cube()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(FpsgHipError):
        meshes.sample_surface(tv, tf, 16)
    with pytest.raises(FpsgHipError):
        meshes.render_views(tv, tf, size=16)
    with pytest.raises(ValueError):
        meshes.sample_surface(tv, tf, 0)
    with pytest.raises(ValueError):
        meshes.sample_surface(tv[:, :2], tf, 4)
    with pytest.raises(ValueError):
        meshes.render_views(tv, tf, size=16, ssaa=3, material=meshes.PhongMaterial(shininess=24))
    with pytest.raises(ValueError):
        meshes.render_views(tv, tf, size=16, ssaa=8)
    assert meshes.PhongMaterial().log2_shininess() == 5
    p = meshes.PhongMaterial().params((0.1, 0.2, 0.3))
    assert p.dtype == np.float32 and p.shape == (15,) and np.allclose(np.linalg.norm(p[9:12]), 1, atol=1e-6)
    assert p[0:3].max() + p[3:6].max() + p[6:9].max() <= 1.0               # the defaults never clip


# ---- 6. prepare_dataset.py ------------------------------------------------------------------------------------------

def test_prepare_dataset_help_and_defaults():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "prepare_dataset.py"), "--help"], capture_output=True,
                         text=True, cwd=ROOT)
    assert out.returncode == 0
    for flag in ("--mesh_root", "--img_root", "--pc_root", "--output", "--n_points", "--oversample", "--views", "--size",
                 "--ssaa", "--background", "--normalize", "--up", "--seed", "--classes", "--train_classes",
                 "--test_classes", "--overwrite"):
        assert flag in out.stdout, flag
    import prepare_dataset
    opt = prepare_dataset.build_parser().parse_args(["--mesh_root", "m", "--img_root", "i", "--pc_root", "p",
                                                     "--output", "o"])
    assert (opt.n_points, opt.oversample, opt.views, opt.size, opt.ssaa) == (2048, 4, 12, 600, 2)
    assert (opt.normalize, opt.up, opt.seed, opt.overwrite, opt.background) == ("bbox", "z", 0, False, "1,1,1")
    assert opt.classes is None and opt.train_classes is None and opt.test_classes is None
    assert prepare_dataset.MAX_WORKERS == 16 and 1 <= opt.workers <= 16
    a, b = prepare_dataset.item_seed(0, "chair/train/chair_0001.off"), prepare_dataset.item_seed(1, "chair/train/chair_0001.off")
    assert a != b and 0 <= a < 2 ** 63 and a == prepare_dataset.item_seed(0, "chair/train/chair_0001.off")
