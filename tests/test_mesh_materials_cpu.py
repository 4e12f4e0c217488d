"""ShapeNet from meshes, what needs no GPU: the ``.obj`` / ``.mtl`` parser, texture packing, the list files, the split,
``prepare_dataset.py``'s two sets of defaults and its refusals, K28's refusals that come before any pointer is used,
and properties the numpy restatement of the texture lookup must have (so that the GPU tests' yardstick is trusted)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT

import _mesh_material_ref as mref
from fpsg_amd import datasets, meshes


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


# ---- 1. the parser -----------------------------------------------------------------------------------------------------

MTL = """# exported
newmtl red
Ka 0 0 0
Kd 1 0 0.25
Ks 0.4 0.4 0.4
Ns 10
d 0.5
illum 2
fancy_key 1 2 3
newmtl wood
Kd 0 0 0
map_Kd -s 1 1 1 a b\\c.png
newmtl lost
Kd 0.5 0.5 0.5
map_Kd -clamp on nowhere.png
"""


def test_obj_scene_reads_materials_uv_and_fans(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "a b"))
    Image.fromarray(np.full((2, 3, 3), 200, np.uint8)).save(os.path.join(root, "a b", "c.png"))
    _write(os.path.join(root, "m.mtl"), MTL)
    _write(os.path.join(root, "m.obj"), """
usemtl wood
v 0 0 0
v 1 0 0
v 1 1 0
vt 0 0
vt 1 0 0.5
vt 1 1
f 1/1 2/2 3/3
mtllib m.mtl
v 0 1 0
v -0.5 0.5 0
vt 0 1
vt -0.25 0.5
usemtl red
f -5/-5/1 -4/-4/1 -3/-3/1 -2/-2/1 -1/-1/1
usemtl nobody
f 1 2 3
usemtl lost
f 1//1 2//1 3//1
""")
    s = meshes.load_obj_scene(os.path.join(root, "m.obj"))
    assert s.verts.shape == (5, 3) and s.verts.dtype == np.float32
    assert s.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 2], [0, 1, 2]]
    assert [m.name for m in s.materials] == ["red", "wood", "lost"]
    assert s.materials[0].kd == (1.0, 0.0, 0.25) and s.materials[0].texture is None
    assert s.materials[1].texture == os.path.join(root, "a b", "c.png")       # options skipped, blank kept, \\ turned
    assert s.materials[2].texture is None and s.materials[2].kd == (0.5, 0.5, 0.5)   # missing file: Kd
    # usemtl before the mtllib line counts; an unknown name is no material
    assert s.face_material.tolist() == [1, 0, 0, 0, -1, 2] and s.face_material.dtype == np.int32
    uv = s.face_uv
    assert uv.shape == (6, 3, 2) and uv.dtype == np.float32
    assert uv[0].tolist() == [[0, 0], [1, 0], [1, 1]]                          # the third number of a vt is ignored
    # the pentagon with negative vt indices: a fan about its first corner, uv carried with the corners
    assert uv[1].tolist() == [[0, 0], [1, 0], [1, 1]] and uv[2].tolist() == [[0, 0], [1, 1], [0, 1]]
    assert uv[3].tolist() == [[0, 0], [0, 1], [-0.25, 0.5]]
    assert np.isnan(uv[4]).all() and np.isnan(uv[5]).all()                     # corners without vt
    text = "\n".join(s.warnings)
    assert "nowhere.png" in text and "nobody" in text and len(s.warnings) == 2
    # load_mesh reads the same geometry
    v, f = meshes.load_mesh(os.path.join(root, "m.obj"))
    assert np.array_equal(v, s.verts) and np.array_equal(f, s.faces)


def test_obj_scene_without_its_mtl_is_a_warning(tmp_path):
    path = os.path.join(str(tmp_path), "x.obj")
    _write(path, "mtllib gone.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nusemtl m\nf 1/1 2/1 3/9\n")
    s = meshes.load_obj_scene(path)
    assert s.materials == [] and s.face_material.tolist() == [-1]
    assert s.face_uv[0, :2].tolist() == [[0, 0], [0, 0]] and np.isnan(s.face_uv[0, 2]).all()   # vt 9 does not exist
    text = "\n".join(s.warnings)
    assert "gone.mtl" in text and "'m'" in text and "out of range" in text
    _write(path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match="line 4"):
        meshes.load_obj_scene(path)


# ---- 2. pack_textures ------------------------------------------------------------------------------------------------

def test_pack_textures_downsizes_and_packs_each_file_once(tmp_path):
    root = str(tmp_path)
    rng = np.random.default_rng(3)
    small = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)                    # 5 wide, 3 high
    Image.fromarray(small).save(os.path.join(root, "small.png"))
    Image.fromarray(rng.integers(0, 256, (40, 100, 3), dtype=np.uint8)).save(os.path.join(root, "big.png"))
    Image.fromarray(np.full((4, 4), 77, np.uint8)).save(os.path.join(root, "grey.png"))      # one channel -> RGB
    _write(os.path.join(root, "broken.png"), "not an image")
    mats = [meshes.ObjMaterial("a", (0.1, 0.2, 0.3), os.path.join(root, "small.png")),
            meshes.ObjMaterial("b", (0.4, 0.5, 0.6), None),
            meshes.ObjMaterial("c", (0, 0, 0), os.path.join(root, "big.png")),
            meshes.ObjMaterial("d", (1, 1, 1), os.path.join(root, "small.png")),
            meshes.ObjMaterial("e", (0.7, 0.7, 0.7), os.path.join(root, "broken.png")),
            meshes.ObjMaterial("f", (0, 0, 0), os.path.join(root, "grey.png"))]
    p = meshes.pack_textures(mats, max_size=10)
    assert p.tex_table.dtype == np.int32 and p.tex_table.tolist() == [[0, 5, 3], [15, 10, 4], [55, 4, 4]]
    assert p.texels.dtype == np.uint8 and p.texels.shape == (15 + 40 + 16, 3)
    assert np.array_equal(p.texels[:15].reshape(3, 5, 3), small)               # rows from the top, as PIL gives them
    assert (p.texels[55:] == 77).all()
    assert p.materials.dtype == np.float32 and p.materials[:, 3].tolist() == [0, -1, 1, 0, -1, 2]
    assert np.allclose(p.materials[1, :3], (0.4, 0.5, 0.6)) and np.allclose(p.materials[4, :3], 0.7)
    assert len(p.warnings) == 1 and "broken.png" in p.warnings[0]
    q = meshes.pack_textures(mats[:4])                                          # the default leaves 100 x 40 alone
    assert q.tex_table.tolist() == [[0, 5, 3], [15, 100, 40]]
    empty = meshes.pack_textures([])
    assert empty.texels.shape == (0, 3) and empty.tex_table.shape == (0, 3) and empty.materials.shape == (0, 4)


# ---- 3. the lists ----------------------------------------------------------------------------------------------------

def test_shapenet_lists_round_trip_through_the_dataset(tmp_path):
    """The layout of test_entrypoints_cpu.py::test_shapenet_file_layout, with the lists written instead of typed."""
    rng = np.random.default_rng(1)
    root, out = str(tmp_path / "ShapeNet"), str(tmp_path / "out")
    for syn in ("02880940", "03797390", "03001627", "02773838"):               # bowl, mug: novel; chair: base; bag: neither
        names = []
        for i in (3, 1, 0, 2):
            item = os.path.join(root, syn, f"m{i}", "models")
            os.makedirs(os.path.join(item, "images"))
            if not (syn == "03797390" and i == 2):                             # an item without views is not listed
                Image.fromarray(rng.integers(0, 255, (256, 256, 3), dtype=np.uint8)).save(
                    os.path.join(item, "images", "00.png"))
            if not (syn == "03001627" and i == 1):                             # nor one without a cloud
                np.save(os.path.join(item, "npy_file.npy"), rng.standard_normal((15000, 3)).astype(np.float32))
            names.append(f"m{i}")
        _write(os.path.join(root, f"{syn}_train.txt"), "\n".join(names[:3]) + "\n")
        _write(os.path.join(root, f"{syn}_test.txt"), names[3] + "\n")
    got = meshes.write_shapenet_lists(root, out)
    assert got == {"train": 3, "test": 7, "classes": ["02880940", "03001627", "03797390"]}
    assert sorted(os.listdir(os.path.join(out, "shapenet_files"))) == [
        "shapenet+02880940.txt", "shapenet+03001627.txt", "shapenet+03797390.txt"]
    text = open(os.path.join(out, "shapenet_test.txt")).read()
    assert not text.endswith("\n")
    assert text.split("\n") == [os.path.join(root, "02880940", f"m{i}", "models") for i in range(4)] + \
        [os.path.join(root, "03797390", f"m{i}", "models") for i in (0, 1, 3)]
    assert open(os.path.join(out, "shapenet_train.txt")).read().split("\n") == \
        [os.path.join(root, "03001627", f"m{i}", "models") for i in (0, 2, 3)]
    assert open(os.path.join(out, "shapenet_files", "shapenet+03797390.txt")).read().split("\n") == \
        [os.path.join(root, "03797390", f"m{i}", "models") for i in (0, 1, 3)]
    ds = datasets.FewShotShapeNet(os.path.join(out, "shapenet_test.txt"), os.path.join(out, "shapenet_files"),
                                  n_classes=1, n_support=1, n_query=2, transform=datasets.shapenet_transform())
    assert len(ds) == 7
    ep = ds[5]
    assert ep["class"] == "mug" and ep["xq"].shape == (2, 3, 224, 224) and ep["pcs"].shape == (1, 2048, 3)
    # other classes on request
    got = meshes.write_shapenet_lists(root, str(tmp_path / "other"), train_classes=["02773838"], test_classes=["02880940"])
    assert got == {"train": 4, "test": 4, "classes": ["02773838", "02880940"]}


def test_default_classes_are_the_references():
    names = datasets.SHAPENET_ID2NAME
    assert [names[s] for s in meshes.SHAPENET_TRAIN_CLASSES] == ["airplane", "camera", "car", "clock", "chair", "faucet",
                                                                 "printer", "rocket"]
    assert [names[s] for s in meshes.SHAPENET_TEST_CLASSES] == ["bowl", "cellphone", "jar", "mug", "monitor"]


# ---- 4. the split ------------------------------------------------------------------------------------------------------

def test_split_is_a_function_of_seed_and_path_and_about_80_20():
    import prepare_dataset as tool
    n, p = 1000, 0.8
    names = [f"03001627/{k:032x}/models/model_normalized.obj" for k in range(n)]
    first = [tool.is_train_item(0, name) for name in names]
    again = {name: tool.is_train_item(0, name) for name in reversed(names)}    # another order of the walk
    assert first == [again[name] for name in names]
    assert first != [tool.is_train_item(1, name) for name in names]
    assert tool.is_train_item(0, names[0].replace("/", os.sep)) == first[0]
    # a binomial share: three sigma = 3 sqrt(p (1 - p) / n) = 0.0379 at n = 1000, p = 0.8
    band = 3 * math.sqrt(p * (1 - p) / n)
    assert abs(sum(first) / n - p) <= band, (sum(first), band)
    quarter = sum(tool.is_train_item(0, name, 0.25) for name in names) / n
    assert abs(quarter - 0.25) <= 3 * math.sqrt(0.25 * 0.75 / n)
    assert all(tool.is_train_item(0, name, 1.0) for name in names) and not any(tool.is_train_item(0, name, 0.0) for name in names)


# ---- 5. prepare_dataset.py's command line ------------------------------------------------------------------------------

def test_defaults_of_both_data_sets():
    import prepare_dataset as tool
    need = ["--mesh_root", "m", "--pc_root", "p", "--output", "o"]
    opt = tool.build_parser("shapenet").parse_args(need + ["--dataset", "shapenet"])
    assert (opt.size, opt.n_points, opt.oversample, opt.normalize, opt.up) == (256, 15000, 1, "none", "y")
    assert (opt.max_texture, opt.no_materials, opt.train_fraction, opt.img_root, opt.views, opt.ssaa) == \
        (1024, False, 0.8, None, 12, 2)
    opt = tool.build_parser().parse_args(need + ["--img_root", "i"])
    assert (opt.dataset, opt.size, opt.n_points, opt.oversample, opt.normalize, opt.up) == \
        ("modelnet", 600, 2048, 4, "bbox", "z")
    assert opt.n_points * opt.oversample <= 16384 and 15000 <= 16384           # both defaults pass the refusal below


def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "prepare_dataset.py"), *args], capture_output=True,
                          text=True, cwd=ROOT, timeout=120)


def test_refusals_come_before_any_work(tmp_path):
    need = ["--mesh_root", str(tmp_path), "--pc_root", str(tmp_path / "pc"), "--output", str(tmp_path / "out")]
    out = _tool("--dataset", "shapenet", *need, "--img_root", str(tmp_path / "img"))
    assert out.returncode == 2 and "--img_root is not used with --dataset shapenet" in out.stderr
    out = _tool(*need)
    assert out.returncode == 2 and "the following arguments are required: --img_root" in out.stderr
    out = _tool("--dataset", "shapenet", *need, "--oversample", "2")           # 30000 samples
    assert out.returncode == 1 and "30000 samples are more than farthest point sampling thins (16384)" in out.stderr
    out = _tool(*need, "--img_root", str(tmp_path / "img"), "--n_points", "4097")
    assert out.returncode == 1 and "16388 samples" in out.stderr
    assert not os.path.exists(tmp_path / "pc") and not os.path.exists(tmp_path / "out")
    out = _tool("--dataset", "shapenet", "--help")
    for flag in ("--dataset", "--max_texture", "--no_materials", "--train_fraction"):
        assert flag in out.stdout, flag


# ---- 6. K28's entry: what it refuses before it uses a pointer --------------------------------------------------------

def test_c_entry_refuses_counts_over_the_limits():
    from fpsg_amd import _hip
    lib = _hip.load()
    params = (ctypes.c_float * 17)()

    def render(M=0, T=0, n_texels=0, W=64, ssaa=1):
        return lib.fpsg_mesh_render_materials(None, 8, None, 4, None, None, None, M, None, T, None, n_texels, None, 2, W,
                                              64, ssaa, ctypes.c_float(2.0), params, 5, None, None, None, None, None,
                                              None, 0, None)

    assert render() == -1                                                      # shapes and limits pass: a null pointer
    for bad in (dict(M=-1), dict(T=-1), dict(n_texels=-1), dict(W=0), dict(ssaa=5)):
        assert render(**bad) == -2, bad
    for bad in (dict(M=meshes.RENDER_MAX_MATERIALS + 1), dict(T=meshes.RENDER_MAX_TEXTURES + 1),
                dict(n_texels=meshes.RENDER_MAX_TEXELS + 1), dict(W=8193)):
        assert render(**bad) == -4, bad
    assert render(M=meshes.RENDER_MAX_MATERIALS + 1) == -4 and b"M <= 65536, T <= 4096" in lib.fpsg_last_error()
    assert render(M=meshes.RENDER_MAX_MATERIALS, T=meshes.RENDER_MAX_TEXTURES, n_texels=meshes.RENDER_MAX_TEXELS) == -1
    k27 = lib.fpsg_mesh_render_workspace_bytes(8, 4, 2, 64, 32)
    assert lib.fpsg_mesh_render_materials_workspace_bytes(8, 4, 2, 64, 32, 0, 0) == k27
    assert lib.fpsg_mesh_render_materials_workspace_bytes(8, 4, 2, 64, 32, 3, 2) == k27 + 3 * 16 + 32
    assert lib.fpsg_mesh_render_materials_workspace_bytes(8, 4, 2, 64, 32, meshes.RENDER_MAX_MATERIALS + 1, 0) == 0
    assert lib.fpsg_mesh_render_materials_workspace_bytes(8, 4, 2, 64, 32, 0, -1) == 0


# ---- 7. the restatement's lookup ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_lookup_hits_texel_centres_repeats_and_is_continuous_across_the_seam(dtype):
    rng = np.random.default_rng(0)
    tex = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)                      # 3 wide, 5 high
    want = tex.astype(dtype) / dtype(255)
    for i in range(3):
        for j in range(5):                                                     # v = 0 is the bottom row
            u, v = np.array([(i + 0.5) / 3], dtype), np.array([1 - (j + 0.5) / 5], dtype)
            for du, dv in ((0, 0), (2, -3), (-1, 1)):
                got = mref.lookup(tex, u + dtype(du), v + dtype(dv))[0]
                # a coordinate of size 4 is off by up to 2 eps, times the texture's size 5, times a step of at most 1
                assert np.abs(got - want[j, i]).max() <= 64 * np.finfo(dtype).eps, (i, j, du, dv)
    # either side of u = 0 (and of 1): the same colour up to the step's size times the slope
    tiny = dtype(1e-6)
    v = np.array([0.3], dtype)
    a, b = mref.lookup(tex, np.array([-tiny], dtype), v), mref.lookup(tex, np.array([tiny], dtype), v)
    assert np.abs(a - b).max() <= 2 * 3 * tiny * 1.0 + 1e-6
    one = mref.lookup(np.full((1, 1, 3), 51, np.uint8), np.array([0.2, -7.5, 1e30, np.inf], dtype), np.array([0.9, 3, 1, 0], dtype))
    assert np.abs(one - dtype(51) / dtype(255)).max() <= 4 * np.finfo(dtype).eps   # 1 x 1: one colour everywhere
