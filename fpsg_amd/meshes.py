"""Datasets from meshes: mesh files in, sampled clouds (K26) and rendered views (K27, with materials and textures K28)
out, plus the list files that ``fpsg_amd.datasets`` reads.  The definitions of the kernels are in ``include/fpsg_hip.h``.

The host part (``load_mesh``, ``load_obj_scene``, ``pack_textures``, ``normalize_mesh``, ``write_ply_points``,
``camera_views``, ``write_modelnet_lists``, ``write_shapenet_lists``) needs no GPU.  ``sample_surface``,
``render_views`` and ``render_points`` (K29: views of point clouds as shaded spheres) run on the GPU only: a CPU tensor
raises ``FpsgHipError``.

Generated meshes (K31): ``corner_table`` and ``write_obj_mesh`` are host code; ``vertex_normals`` (K31a) and
``render_views(face_normals=...)`` (K31b, smooth shading) run on the GPU only.

Mesh accuracy (K32): ``point_mesh_distance`` (the nearest triangle of every point) and ``mesh_accuracy`` (that distance
and K26 + K1 the other way round, for one mesh and one cloud) run on the GPU only.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
import re

import numpy as np
import torch

from . import _hip

MESH_MAX_FACES = 1 << 24        # FPSG_MESH_MAX_FACES (include/fpsg_hip.h)
RENDER_MAX_SIZE = 8192          # FPSG_RENDER_MAX_SIZE
RENDER_MAX_SSAA = 4             # FPSG_RENDER_MAX_SSAA

# the reference's TRAIN_SET_DIC['modelnet'] / TEST_SET_DIC['modelnet'] (generate_dataset.py): base and novel classes
MODELNET_TRAIN_CLASSES = ("airplane", "bathtub", "bed", "chair", "desk", "dresser", "monitor", "sofa", "table",
                          "toilet")
MODELNET_TEST_CLASSES = ("cup", "keyboard", "door", "laptop", "bowl")
# TRAIN_SET_DIC['shapenet'] / TEST_SET_DIC['shapenet'] there, as synset ids (datasets.SHAPENET_ID2NAME)
SHAPENET_TRAIN_CLASSES = ("02691156", "02942699", "02958343", "03046257", "03001627", "03325088", "04004475", "04099429")
SHAPENET_TEST_CLASSES = ("02880940", "02992529", "03593526", "03797390", "03211117")
RENDER_MAX_MATERIALS = 65536    # FPSG_RENDER_MAX_MATERIALS
RENDER_MAX_TEXTURES = 4096      # FPSG_RENDER_MAX_TEXTURES
RENDER_MAX_TEXELS = 1 << 28     # FPSG_RENDER_MAX_TEXELS
POINTS_MAX_N = 16384            # FPSG_POINTS_MAX_N
POINTS_MAX_RADIUS_PX = 64       # FPSG_POINTS_MAX_RADIUS_PX
POINT_MESH_MAX_POINTS = 1 << 20  # FPSG_POINT_MESH_MAX_POINTS
POINT_MESH_MAX_MESHES = 65535   # FPSG_POINT_MESH_MAX_MESHES
POINT_MESH_MAX_TOTAL = 1 << 26  # FPSG_POINT_MESH_MAX_TOTAL
POINT_MESH_MAX_CHUNKS = 64      # FPSG_POINT_MESH_MAX_CHUNKS


# ------------------------------------------------------------------------------------------ files
def _lines(path: str):
    """-> (stripped non-empty lines without comments as a numpy array of str, their 1-based line numbers)."""
    with open(path, "r", errors="replace") as f:
        text = f.read()
    text = re.sub(r"#[^\n]*", "", text)
    text = re.sub(r"[ \t\r\f\v]+", " ", text)
    arr = np.char.strip(np.array(text.split("\n"), dtype=np.str_))
    keep = arr != ""
    return arr[keep], np.nonzero(keep)[0] + 1


def _numbers(lines, dtype, path, what):
    if len(lines) == 0:
        return np.zeros((0,), dtype)
    try:
        return np.array(" ".join(lines.tolist()).split(), dtype=np.float64).astype(dtype)
    except ValueError as e:
        raise ValueError(f"{path}: bad {what}: {e}") from None


def _fan(flat, starts, counts, lineno):
    """Polygons ``flat[starts[k] : starts[k] + counts[k]]`` -> fan triangles [T,3] and each triangle's line number."""
    ok = counts >= 3
    starts, counts, lineno = starts[ok], counts[ok], lineno[ok]
    per = counts - 2
    total = int(per.sum())
    if total == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0,), np.int64)
    owner = np.repeat(np.arange(len(per)), per)
    k = np.arange(total) - np.repeat(np.cumsum(per) - per, per)           # 0 .. per-1 inside each polygon
    s = starts[owner]
    return np.stack([flat[s], flat[s + 1 + k], flat[s + 2 + k]], axis=1), lineno[owner]


def _check_range(tri, tri_line, n_verts, path):
    bad = (tri < 0) | (tri >= n_verts)
    if bad.any():
        row = int(np.nonzero(bad.any(axis=1))[0][0])
        raise ValueError(f"{path}, line {int(tri_line[row])}: face index out of range "
                         f"({tri[row].tolist()} with {n_verts} vertices)")


def _load_off(path):
    lines, lineno = _lines(path)
    if len(lines) == 0 or not lines[0].upper().startswith("OFF"):
        raise ValueError(f"{path}: not an OFF file")
    rest = lines[0][3:].strip()          # 'OFF123 456 0': the counts fused to the keyword, as the reference tolerates
    body = 1
    if not rest:
        if len(lines) < 2:
            raise ValueError(f"{path}: no counts")
        rest, body = lines[1], 2
    try:
        nv, nf = (int(t) for t in rest.split()[:2])
    except ValueError:
        raise ValueError(f"{path}, line {int(lineno[body - 1])}: bad counts {rest!r}") from None
    if nv < 0 or nf < 0 or len(lines) < body + nv + nf:
        raise ValueError(f"{path}: {nv} vertices and {nf} faces announced, {len(lines) - body} lines present")
    verts = _numbers(lines[body:body + nv], np.float32, path, "vertex")
    if verts.size != nv * 3:
        raise ValueError(f"{path}: vertex lines do not hold 3 numbers each")
    flines, fno = lines[body + nv:body + nv + nf], lineno[body + nv:body + nv + nf]
    flat = _numbers(flines, np.int64, path, "face")
    ntok = np.char.count(flines, " ") + 1 if nf else np.zeros((0,), np.int64)
    starts = np.cumsum(ntok) - ntok
    counts = flat[starts] if nf else flat[:0]
    short = counts + 1 > ntok            # colours may follow the indices, fewer tokens than announced may not
    if short.any():
        raise ValueError(f"{path}, line {int(fno[np.nonzero(short)[0][0]])}: face with fewer indices than its count")
    tri, tri_line = _fan(flat, starts + 1, counts, fno)
    _check_range(tri, tri_line, nv, path)
    return verts.reshape(nv, 3), tri.astype(np.int32)


def _load_obj(path):
    lines, lineno = _lines(path)
    is_v = np.char.startswith(lines, "v ")
    is_f = np.char.startswith(lines, "f ")
    vlines = np.char.partition(lines[is_v], " ")[:, 2] if is_v.any() else lines[:0]
    vals = _numbers(vlines, np.float32, path, "vertex")
    nv = int(is_v.sum())
    per = np.char.count(vlines, " ") + 1 if nv else np.zeros((0,), np.int64)
    if nv and (per < 3).any():
        raise ValueError(f"{path}: a 'v' record with fewer than 3 numbers")
    if nv and not (per == per[0]).all():
        raise ValueError(f"{path}: 'v' records of different lengths")
    verts = vals.reshape(nv, -1)[:, :3] if nv else np.zeros((0, 3), np.float32)
    flines, fno = lines[is_f], lineno[is_f]
    if len(flines) == 0:
        return np.ascontiguousarray(verts), np.zeros((0, 3), np.int32)
    ftext = np.char.partition(flines, " ")[:, 2]
    ntok = np.char.count(ftext, " ") + 1
    tokens = np.array(" ".join(ftext.tolist()).split(), dtype=np.str_)
    try:
        flat = np.char.partition(tokens, "/")[:, 0].astype(np.int64)      # v, v/vt, v/vt/vn, v//vn
    except ValueError as e:
        raise ValueError(f"{path}: bad face record: {e}") from None
    # a negative index counts back from the vertices defined so far; a positive one is 1-based; 0 is no vertex
    seen = np.cumsum(is_v)[is_f]
    seen_tok = np.repeat(seen, ntok)
    flat = np.where(flat < 0, flat + seen_tok, np.where(flat > 0, flat - 1, -1))
    starts = np.cumsum(ntok) - ntok
    tri, tri_line = _fan(flat, starts, ntok, fno)
    _check_range(tri, tri_line, nv, path)
    return np.ascontiguousarray(verts), tri.astype(np.int32)


# ------------------------------------------------------------------------ .obj with materials (K28)
@dataclasses.dataclass
class ObjMaterial:
    name: str
    kd: tuple = (0.8, 0.8, 0.8)          # the value a .mtl record without Kd gets from common importers
    texture: str | None = None           # map_Kd, resolved relative to the .mtl; None when absent or not found


@dataclasses.dataclass
class ObjScene:
    """A ``.obj`` with what its ``.mtl`` says about colour.  ``face_material [F]`` int32 indexes ``materials`` (-1: none);
    ``face_uv [F,3,2]`` float32 holds the corners' ``vt`` in the faces' vertex order, NaN where a corner has none."""
    verts: np.ndarray
    faces: np.ndarray
    face_material: np.ndarray
    face_uv: np.ndarray
    materials: list
    warnings: list


# options of a map_Kd statement and how many numbers may follow each (o, s, t: one to three)
_MAP_OPTIONS = {"-blendu": 1, "-blendv": 1, "-cc": 1, "-clamp": 1, "-imfchan": 1, "-texres": 1, "-bm": 1, "-boost": 1,
                "-type": 1, "-mm": 2, "-o": 3, "-s": 3, "-t": 3}


def _is_number(tok):
    try:
        float(tok)
        return True
    except ValueError:
        return False


def _map_file(rest: str) -> str:
    """The file name of a ``map_Kd`` statement: options in front skipped, blanks inside kept, backslashes turned."""
    toks = rest.split()
    i = 0
    while i < len(toks) and toks[i] in _MAP_OPTIONS:
        n, opt = _MAP_OPTIONS[toks[i]], toks[i]
        i += 1
        if opt in ("-o", "-s", "-t"):
            k = 0
            while k < n and i < len(toks) - 1 and _is_number(toks[i]):   # the last token is the name, number or not
                i, k = i + 1, k + 1
        else:
            i += n
    return " ".join(toks[i:]).strip().replace("\\", "/")


def _load_mtl(path, warnings):
    """-> [ObjMaterial] in the file's order.  Only ``newmtl``, ``Kd`` and ``map_Kd`` are read."""
    out = []
    with open(path, "r", errors="replace") as f:
        for raw in f:
            line = raw.split("#", 1)[0].strip()
            key, _, rest = line.partition(" ")
            rest = rest.strip()
            if key == "newmtl":
                out.append(ObjMaterial(rest))
            elif not out:
                continue
            elif key == "Kd":
                try:
                    kd = [float(t) for t in rest.split()[:3]]
                    out[-1].kd = tuple(kd) if len(kd) == 3 else (kd[0],) * 3
                except (ValueError, IndexError):
                    warnings.append(f"{path}: bad Kd {rest!r} in material {out[-1].name!r}")
            elif key == "map_Kd":
                name = _map_file(rest)
                tex = os.path.normpath(os.path.join(os.path.dirname(path), name))
                if name and os.path.isfile(tex):
                    out[-1].texture = tex
                else:
                    warnings.append(f"{path}: texture {name!r} of material {out[-1].name!r} not found")
    return out


def _obj_verts(vrecords, path):
    """The ``v`` records of an ``.obj`` -> float32 [V,3], with ``_load_obj``'s checks."""
    nv = len(vrecords)
    if nv == 0:
        return np.zeros((0, 3), np.float32)
    vlines = np.char.partition(vrecords, " ")[:, 2]
    per = np.char.count(vlines, " ") + 1
    if (per < 3).any():
        raise ValueError(f"{path}: a 'v' record with fewer than 3 numbers")
    if not (per == per[0]).all():
        raise ValueError(f"{path}: 'v' records of different lengths")
    return np.ascontiguousarray(_numbers(vlines, np.float32, path, "vertex").reshape(nv, -1)[:, :3])


def load_obj_scene(path: str) -> ObjScene:
    """``.obj`` -> ``ObjScene``: what ``load_mesh`` reads, plus ``vt``, ``usemtl`` and the ``mtllib`` files beside it.

    Polygons are fan-triangulated with their ``uv`` and material.  ``v/vt`` and ``v/vt/vn`` corners, negative indices
    for both.  A ``usemtl`` counts from its line on, wherever the ``mtllib`` stands.  In a ``.mtl`` only ``newmtl``,
    ``Kd`` and ``map_Kd`` are read (``d``, ``illum``, ``Ka``, ``Ks``, ``Ns`` and unknown keys are ignored); options in
    front of a texture's name are skipped, the name may hold blanks and backslashes and is resolved relative to the
    ``.mtl``.  A missing ``.mtl``, a missing texture, an unknown material and a ``vt`` index out of range are entries in
    ``warnings``, not errors: the faces fall back to no material, to ``Kd``, or to NaN ``uv`` (which K28 shades with
    ``Kd``).  Face indices outside the vertices raise ``ValueError`` as in ``load_mesh``."""
    lines, lineno = _lines(path)
    warnings = []
    is_v, is_vt, is_f = (np.char.startswith(lines, k) for k in ("v ", "vt ", "f "))
    is_use = np.char.startswith(lines, "usemtl")
    verts = _obj_verts(lines[is_v], path)
    nv = len(verts)
    vt_rows = [(t.split() + ["0", "0"])[1:3] for t in lines[is_vt].tolist()]   # u, v; a third number is ignored
    try:
        vts = np.array(vt_rows, dtype=np.float64).astype(np.float32).reshape(-1, 2)
    except ValueError as e:
        raise ValueError(f"{path}: bad 'vt' record: {e}") from None
    materials = []
    for lib in lines[np.char.startswith(lines, "mtllib ")].tolist():
        name = lib.partition(" ")[2].strip().replace("\\", "/")
        mtl = os.path.join(os.path.dirname(path), name)
        if os.path.isfile(mtl):
            materials += _load_mtl(mtl, warnings)
        else:
            warnings.append(f"{path}: material library {name!r} not found")
    index = {}
    for k, m in enumerate(materials):
        index.setdefault(m.name, k)
    flines, fno = lines[is_f], lineno[is_f]
    if len(flines) == 0:
        return ObjScene(verts, np.zeros((0, 3), np.int32), np.zeros((0,), np.int32), np.zeros((0, 3, 2), np.float32),
                        materials, warnings)
    ftext = np.char.partition(flines, " ")[:, 2]
    ntok = np.char.count(ftext, " ") + 1
    tokens = np.array(" ".join(ftext.tolist()).split(), dtype=np.str_)
    parts = np.char.partition(tokens, "/")
    vt_text = np.char.partition(parts[:, 2], "/")[:, 0]
    try:
        vi = parts[:, 0].astype(np.int64)
        ti = np.where(vt_text == "", "0", vt_text).astype(np.int64)             # 0 is no index in OBJ
    except ValueError as e:
        raise ValueError(f"{path}: bad face record: {e}") from None
    seen_v = np.repeat(np.cumsum(is_v)[is_f], ntok)
    seen_t = np.repeat(np.cumsum(is_vt)[is_f], ntok)
    vi = np.where(vi < 0, vi + seen_v, np.where(vi > 0, vi - 1, -1))
    ti = np.where(ti < 0, ti + seen_t, np.where(ti > 0, ti - 1, -1))
    starts = np.cumsum(ntok) - ntok
    pos, tri_line = _fan(np.arange(len(tokens)), starts, ntok, fno)           # token positions of every triangle
    tri = vi[pos]
    _check_range(tri, tri_line, nv, path)
    tri_t = ti[pos]
    has = (tri_t >= 0) & (tri_t < len(vts))
    if ((tri_t >= len(vts)) | ((tri_t < 0) & (vt_text[pos] != ""))).any():
        warnings.append(f"{path}: 'vt' index out of range; those corners have no uv")
    uv = np.full(tri.shape + (2,), np.nan, np.float32)
    if len(vts):
        uv[has] = vts[tri_t[has]]
    # the usemtl in force at each face line
    use_names = [t.partition(" ")[2].strip() for t in lines[is_use].tolist()]
    use_idx = np.array([index.get(n, -1) for n in use_names] + [-1], dtype=np.int32)   # the last slot: no usemtl yet
    for n in sorted({n for n in use_names if n not in index}):
        warnings.append(f"{path}: unknown material {n!r}")
    which = np.cumsum(is_use)[is_f] - 1                                        # -1 picks the last slot
    owner = np.repeat(np.arange(len(flines)), ntok)[pos[:, 0]] if len(pos) else np.zeros((0,), np.int64)
    return ObjScene(verts, tri.astype(np.int32), use_idx[which][owner].astype(np.int32), uv, materials, warnings)


@dataclasses.dataclass
class PackedTextures:
    """What K28 reads: ``texels`` uint8 ``[n,3]`` (every texture's rows from the top, back to back), ``tex_table`` int32
    ``[T,3]`` (texel offset, width, height) and ``materials`` float32 ``[M,4]`` (``Kd``, texture index or -1)."""
    texels: np.ndarray
    tex_table: np.ndarray
    materials: np.ndarray
    warnings: list


def pack_textures(materials, max_size: int = 1024) -> PackedTextures:
    """Decodes the materials' texture files with PIL, each file once however many materials name it; one larger than
    ``max_size`` on a side is scaled down to it, keeping its aspect.  A file that does not decode is a warning and its
    materials fall back to ``Kd``."""
    from PIL import Image
    if max_size < 1:
        raise ValueError(f"max_size must be positive, got {max_size}")
    slot, blocks, table, warnings = {}, [], [], []
    mats = np.full((len(materials), 4), -1.0, np.float32)
    offset = 0
    for k, m in enumerate(materials):
        mats[k, :3] = m.kd
        if m.texture is None:
            continue
        if m.texture not in slot:
            try:
                with Image.open(m.texture) as im:
                    im = im.convert("RGB")
                    w, h = im.size
                    if max(w, h) > max_size:
                        scale = max_size / max(w, h)
                        im = im.resize((max(1, round(w * scale)), max(1, round(h * scale))), Image.BILINEAR)
                    arr = np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
            except (OSError, ValueError, SyntaxError) as e:
                warnings.append(f"{m.texture}: not decoded ({e})")
                slot[m.texture] = -1
            else:
                slot[m.texture] = len(table)
                table.append((offset, arr.shape[1], arr.shape[0]))
                blocks.append(arr.reshape(-1, 3))
                offset += arr.shape[0] * arr.shape[1]
        mats[k, 3] = slot[m.texture]
    texels = np.concatenate(blocks) if blocks else np.zeros((0, 3), np.uint8)
    return PackedTextures(texels, np.asarray(table, dtype=np.int32).reshape(-1, 3), mats, warnings)


@dataclasses.dataclass
class RenderScene:
    """The per-face colour inputs of K28 for ``render_views(scene=...)``: ``face_material`` int32 ``[F]`` and ``face_uv``
    float32 ``[F,3,2]`` on the mesh's device (either may be None without materials / textures), the host tables
    ``materials [M,4]`` and ``tex_table [T,3]``, and ``texels`` uint8 ``[n,3]`` on the device."""
    face_material: torch.Tensor | None
    face_uv: torch.Tensor | None
    materials: np.ndarray
    tex_table: np.ndarray
    texels: torch.Tensor | None


def scene_tensors(scene: ObjScene, packed: PackedTextures, device) -> RenderScene:
    """An ``ObjScene`` and its packed textures moved to ``device`` for ``render_views``."""
    T = len(packed.tex_table)
    return RenderScene(torch.from_numpy(scene.face_material).to(device) if len(packed.materials) else None,
                       torch.from_numpy(scene.face_uv).to(device) if T else None, packed.materials, packed.tex_table,
                       torch.from_numpy(packed.texels).to(device) if T else None)


def load_mesh(path: str):
    """``.off`` or ``.obj`` -> ``(verts float32 [V,3], faces int32 [F,3])``, polygons fan-triangulated.

    OFF: comments (``#``) and blank lines anywhere, the counts on the keyword's line (``OFF 8 6 0``), fused to it
    (``OFF8 6 0``, which ModelNet40 has and the reference's ``off2ply`` tolerates) or on the next; colours behind a
    face's indices are ignored.  OBJ: ``v`` and ``f`` records only, ``f`` with ``/vt/vn`` parts and negative
    (relative) indices; everything else is ignored.  A face index outside the vertices raises ``ValueError`` with the
    file and the line.  The text is parsed by numpy over the split file, not line by line."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".off":
        return _load_off(path)
    if ext == ".obj":
        return _load_obj(path)
    raise ValueError(f"{path}: unsupported mesh format {ext!r} (.off and .obj are read)")


def normalize_mesh(verts, mode: str = "bbox") -> np.ndarray:
    """``"bbox"``: the bounding box's centre to the origin and its largest extent to 1 (what ``phong.py``'s
    ``center_model`` / ``normalize_model`` did for ModelNet); ``"none"``: unchanged (ShapeNet's ``model_normalized.obj``).
    -> float32 ``[V,3]``.  A mesh without extent is only centred."""
    v = np.asarray(verts, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"expected [V,3] vertices, got {v.shape}")
    if mode == "none" or v.shape[0] == 0:
        return np.ascontiguousarray(v, dtype=np.float32)
    if mode != "bbox":
        raise ValueError(f"mode must be 'bbox' or 'none', got {mode!r}")
    lo, hi = v.min(axis=0), v.max(axis=0)
    extent = float((hi - lo).max())
    v = v - (lo + hi) / 2.0
    if extent > 0 and math.isfinite(extent):
        v = v / extent
    return np.ascontiguousarray(v, dtype=np.float32)


def write_ply_points(path: str, pts, normals=None) -> None:
    """The ASCII vertex-only PLY that ``datasets.ply_reader`` reads back; ``%.9g`` keeps every float32 bit.  With
    ``normals`` ``[N,3]`` the vertices also carry ``nx ny nz`` (what a Poisson reconstruction reads): six columns."""
    p = np.asarray(pts.detach().cpu() if isinstance(pts, torch.Tensor) else pts, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"expected [N,3] points, got {p.shape}")
    head = ("ply\nformat ascii 1.0\n"
            f"element vertex {p.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n")
    if normals is None:
        body = "\n".join("%.9g %.9g %.9g" % (x, y, z) for x, y, z in p.tolist())
    else:
        n = np.asarray(normals.detach().cpu() if isinstance(normals, torch.Tensor) else normals, dtype=np.float32)
        if n.shape != p.shape:
            raise ValueError(f"expected {p.shape} normals, got {n.shape}")
        head += "property float nx\nproperty float ny\nproperty float nz\n"
        body = "\n".join("%.9g %.9g %.9g %.9g %.9g %.9g" % tuple(row) for row in np.concatenate([p, n], axis=1).tolist())
    with open(path, "w") as f:
        f.write(head + "end_header\n" + body + "\n")


def write_obj_mesh(path: str, verts, faces, *, normals=None, face_material=None, materials=None, mtl_name=None) -> None:
    """A triangle mesh as a Wavefront ``.obj`` that ``load_obj_scene`` reads back: ``v`` records, with ``normals``
    ``[V,3]`` also ``vn`` records and faces ``f a//a b//b c//c`` (vertex ``k`` has normal ``k``), without them ``f a b c``.
    ``%.9g`` keeps every float32 bit.

    ``face_material`` int ``[F]`` with ``materials``, a list of ``(name, (r, g, b))``: a ``usemtl`` line in front of
    every run of faces with one material (faces stay in their order) and, beside the file, ``mtl_name`` (default: the
    file's name with ``.mtl``) with a ``newmtl`` / ``Kd`` record per material.  An index outside the list is a
    ``ValueError``, and so is one of the two arguments without the other."""
    def host(a, dtype):
        return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=dtype)

    v, f = host(verts, np.float32), host(faces, np.int64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"expected [V,3] vertices, got {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"expected [F,3] faces, got {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"face indices must be in [0, {len(v)}), got {int(f.min())}..{int(f.max())}")
    if (face_material is None) != (materials is None):
        raise ValueError("face_material and materials go together")
    lines = []
    if materials is not None:
        fm = host(face_material, np.int64).reshape(-1)
        if fm.shape != (len(f),):
            raise ValueError(f"face_material must have one entry per face ({len(f)}), got {fm.shape}")
        if fm.size and (fm.min() < 0 or fm.max() >= len(materials)):
            raise ValueError(f"face_material must index the {len(materials)} materials, got {int(fm.min())}..{int(fm.max())}")
        mtl_name = mtl_name or os.path.splitext(os.path.basename(path))[0] + ".mtl"
        lines.append(f"mtllib {mtl_name}")
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]
    if normals is not None:
        vn = host(normals, np.float32)
        if vn.shape != v.shape:
            raise ValueError(f"normals must be {v.shape}, got {vn.shape}")
        lines += ["vn %.9g %.9g %.9g" % tuple(p) for p in vn.tolist()]
        corner = "%d//%d"
        rows = ["f " + " ".join(corner % (k, k) for k in t) for t in (f + 1).tolist()]
    else:
        rows = ["f %d %d %d" % tuple(t) for t in (f + 1).tolist()]
    if materials is not None:
        starts = np.nonzero(np.concatenate([[True], fm[1:] != fm[:-1]]))[0] if len(fm) else []
        for k in reversed(list(starts)):
            rows.insert(int(k), f"usemtl {materials[int(fm[k])][0]}")
    with open(path, "w") as out:
        out.write("\n".join(lines + rows) + "\n")
    if materials is not None:
        with open(os.path.join(os.path.dirname(path), mtl_name), "w") as out:
            out.write("".join("newmtl %s\nKd %.9g %.9g %.9g\n" % (name, *kd) for name, kd in materials))


# -------------------------------------------------------------------------------------------- K26
def _mesh_tensors(verts, faces):
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.size(1) != 3 or verts.size(0) < 1:
        raise ValueError(f"expected [V,3] vertices, got {tuple(getattr(verts, 'shape', ()))}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.size(1) != 3 or faces.size(0) < 1:
        raise ValueError(f"expected [F,3] faces, got {tuple(getattr(faces, 'shape', ()))}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must be int32 or int64, got {faces.dtype}")
    if faces.size(0) > MESH_MAX_FACES:
        raise ValueError(f"meshes of more than {MESH_MAX_FACES} faces are not supported (got {faces.size(0)})")
    verts = verts.detach()
    _hip.dev_tensor(verts, torch.float32, "verts")
    if faces.device != verts.device:
        raise ValueError(f"faces are on {faces.device}, verts on {verts.device}")
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= verts.size(0):
        raise ValueError(f"face indices must be in [0, {verts.size(0)}), got {lo}..{hi}")
    return verts, faces.to(torch.int32).contiguous()


def surface_cdf(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """The integer CDF of K26: ``[F]`` int64 (the kernel's uint64, below 2^57), ``cdf[-1]`` the total weight."""
    verts, faces = _mesh_tensors(verts, faces)
    return _cdf(verts, faces)


def _cdf(verts, faces):
    V, F = verts.size(0), faces.size(0)
    lib = _hip.load()
    cdf = torch.empty((F,), dtype=torch.int64, device=verts.device)
    ws_bytes = lib.fpsg_mesh_cdf_workspace_bytes(V, F)
    ws = torch.empty((ws_bytes // 8 + 1,), dtype=torch.int64, device=verts.device)
    with torch.cuda.device(verts.device):
        rc = lib.fpsg_mesh_cdf(_hip.ptr(verts), V, _hip.ptr(faces), F, _hip.ptr(cdf), _hip.ptr(ws), ws.numel() * 8,
                               _hip.stream_of(verts))
    _hip.check(rc, "fpsg_mesh_cdf")
    return cdf


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, n: int, *, generator=None, u=None, oversample: int = 1):
    """``n`` points on the surface of the mesh, area-weighted (K26) -> ``(points [n,3] float32, face_idx [n] int64)``.

    ``u`` ``[n * oversample, 3]`` float32 in [0, 1) picks the samples: column 0 the face through the integer CDF,
    columns 1 and 2 the point in it.  When it is not given it is drawn with ``torch.rand`` from ``generator`` (on the
    generator's device, the CPU without one).  The kernel is a pure function of ``(verts, faces, u)``, bitwise the same
    on every run.  With ``oversample > 1`` the ``n * oversample`` samples are thinned to ``n`` well-spread ones by
    farthest point sampling (K16, start index 0), the role of PCL's ``-leaf_size``.

    ``ValueError`` for bad shapes or face indices outside the vertices; ``FpsgHipError`` for CPU tensors and for a
    mesh without area (every face degenerate): that one is found on the device, and no sampling kernel is launched."""
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f"n must be a positive integer, got {n}")
    if isinstance(oversample, bool) or int(oversample) != oversample or int(oversample) < 1:
        raise ValueError(f"oversample must be a positive integer, got {oversample}")
    n, oversample = int(n), int(oversample)
    m = n * oversample
    verts, faces = _mesh_tensors(verts, faces)
    dev = verts.device
    if u is None:
        gdev = generator.device if generator is not None else torch.device("cpu")
        u = torch.rand((m, 3), generator=generator, device=gdev, dtype=torch.float32)
    if not isinstance(u, torch.Tensor) or tuple(u.shape) != (m, 3):
        raise ValueError(f"u must have shape ({m}, 3), got {tuple(getattr(u, 'shape', ()))}")
    u = u.detach().to(dev)
    _hip.dev_tensor(u, torch.float32, "u")
    V, F = verts.size(0), faces.size(0)
    cdf = _cdf(verts, faces)
    total = int(cdf[-1])                                   # one read-back: a mesh without area is refused on the host
    points = torch.empty((m, 3), dtype=torch.float32, device=dev)
    face_idx = torch.empty((m,), dtype=torch.int32, device=dev)
    lib = _hip.load()
    with torch.cuda.device(dev):
        rc = lib.fpsg_mesh_sample(_hip.ptr(verts), V, _hip.ptr(faces), F, _hip.ptr(cdf), total, _hip.ptr(u), m,
                                  _hip.ptr(points), _hip.ptr(face_idx), _hip.stream_of(verts))
    _hip.check(rc, "fpsg_mesh_sample")
    face_idx = face_idx.long()
    if oversample > 1:
        from .sampling import farthest_point_sample
        keep = farthest_point_sample(points.unsqueeze(0), n)[0]
        points, face_idx = points[keep].contiguous(), face_idx[keep].contiguous()
    return points, face_idx


# -------------------------------------------------------------------------------------------- K27
@dataclasses.dataclass(frozen=True)
class PhongMaterial:
    """Flat Phong shading of K27: ``ambient * color + diffuse * color * max(n.l, 0) + specular * max(r.v, 0)^shininess``
    with one directional light fixed in the camera frame (x right, y up, z along the view; ``light`` points from the
    surface towards the light and is normalised here).  The defaults are a light grey object lit from the upper left
    behind the camera; their largest radiance is 0.8 (0.15 + 0.75) + 0.25 = 0.97, so nothing clips.  ``shininess`` is a
    power of two (the kernel squares log2(shininess) times, no ``powf``)."""
    color: tuple = (0.8, 0.8, 0.8)
    ambient: float = 0.15
    diffuse: float = 0.75
    specular: float = 0.25
    shininess: int = 32
    light: tuple = (-0.35, 0.5, -0.8)

    def log2_shininess(self) -> int:
        s = int(self.shininess)
        if s != self.shininess or s < 1 or s & (s - 1) or s > 1024:
            raise ValueError(f"shininess must be a power of two from 1 to 1024, got {self.shininess}")
        return s.bit_length() - 1

    def params(self, background=(1.0, 1.0, 1.0)) -> np.ndarray:
        """The 15 floats of ``fpsg_mesh_render``: ka[3], kd[3], ks[3], l[3], bg[3]; products formed in float64."""
        c = np.asarray(self.color, dtype=np.float64).reshape(3)
        l = np.asarray(self.light, dtype=np.float64).reshape(3)
        norm = float(np.sqrt((l * l).sum()))
        if not norm > 0:
            raise ValueError("light must not be the zero vector")
        return np.concatenate([self.ambient * c, self.diffuse * c, np.full(3, float(self.specular)), l / norm,
                               np.asarray(background, dtype=np.float64).reshape(3)]).astype(np.float32)


def camera_views(elevations_deg=60.0, azimuths_deg=range(0, 360, 30), radius: float = 3.0, up: str = "z") -> np.ndarray:
    """View matrices ``[n_views, 12]`` float32 (right, up, forward, position), one per (elevation, azimuth), elevation
    outermost.  ``phong.py``'s camera: at ``c = radius (sin t cos p, sin t sin p, cos t)``, ``t`` measured from the pole,
    looking at the origin (its TRACK_TO constraint): forward ``f = -c / |c|``, right ``normalize(f x up)`` (``+x`` when
    ``f`` is parallel to ``up``: the top view ``t = 0``), camera up ``right x f``.  ``up="y"``: the same camera for a
    y-up mesh, the axes permuted cyclically (z -> y, y -> x, x -> z).  Built in float64, rounded once."""
    if up not in ("z", "y"):
        raise ValueError(f"up must be 'z' or 'y', got {up!r}")
    if not radius > 0:
        raise ValueError(f"radius must be positive, got {radius}")
    els = np.atleast_1d(np.asarray(elevations_deg, dtype=np.float64))
    azs = np.atleast_1d(np.asarray(list(azimuths_deg) if not np.isscalar(azimuths_deg) else azimuths_deg,
                                   dtype=np.float64))
    pole = np.array([0.0, 0.0, 1.0])
    rows = []
    for t in np.deg2rad(els):
        for p in np.deg2rad(azs):
            c = radius * np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])
            f = -c / np.linalg.norm(c)
            r = np.cross(f, pole)
            r = r / np.linalg.norm(r) if np.linalg.norm(r) > 1e-12 else np.array([1.0, 0.0, 0.0])
            cu = np.cross(r, f)
            vecs = [r, cu, f, c]
            if up == "y":
                vecs = [np.array([v[1], v[2], v[0]]) for v in vecs]
            rows.append(np.concatenate(vecs))
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


def _scene_arguments(scene, F, dev):
    """Shapes, types and devices of a ``RenderScene``; what the values must satisfy is the C entry's to refuse."""
    mat_table = np.ascontiguousarray(np.asarray(scene.materials, dtype=np.float32).reshape(-1, 4))
    tex_table = np.ascontiguousarray(np.asarray(scene.tex_table, dtype=np.int32).reshape(-1, 3))

    def dev_input(t, shape, dtype, name, needed):
        if t is None:
            if needed:
                raise ValueError(f"scene.{name} is needed")
            return None
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dim() != len(shape) or \
                any(want not in (-1, have) for want, have in zip(shape, t.shape)):
            raise ValueError(f"scene.{name} must be a tensor {shape} on {dev}, got {tuple(getattr(t, 'shape', ()))} "
                             f"on {getattr(t, 'device', None)}")
        t = t.detach().contiguous()
        _hip.dev_tensor(t, dtype, f"scene.{name}")
        return t

    face_material = dev_input(scene.face_material, (F,), torch.int32, "face_material", len(mat_table) > 0)
    face_uv = dev_input(scene.face_uv, (F, 3, 2), torch.float32, "face_uv", len(tex_table) > 0)
    texels = dev_input(scene.texels, (-1, 3), torch.uint8, "texels", len(tex_table) > 0)
    return mat_table, tex_table, face_material, face_uv, texels


def _opt(t):
    return None if t is None else _hip.ptr(t)


class _RenderJob:
    """What ``render_views`` and ``render_points`` share, in three steps because both raise their own errors in between:
    the image size, ``ssaa`` and ``ortho_scale``; the views, the background and the shading parameters; on the device,
    the uploads, the output buffers and the arguments every render entry takes."""

    def __init__(self, size, ssaa, allowed, allowed_text, ortho_scale):
        """``allowed``: the caller's ``ssaa`` values, ``allowed_text``: how its message names them."""
        H, W = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        if isinstance(ssaa, bool) or int(ssaa) != ssaa or int(ssaa) not in allowed:
            raise ValueError(f"ssaa must be {allowed_text}, got {ssaa}")
        ssaa = int(ssaa)
        if H < 1 or W < 1 or H * ssaa > RENDER_MAX_SIZE or W * ssaa > RENDER_MAX_SIZE:
            raise ValueError(f"size * ssaa must be from 1 to {RENDER_MAX_SIZE}, got {(H, W)} * {ssaa}")
        if not (ortho_scale > 0 and math.isfinite(ortho_scale)):
            raise ValueError(f"ortho_scale must be positive and finite, got {ortho_scale}")
        self.H, self.W, self.ssaa, self.ortho_scale = H, W, ssaa, float(ortho_scale)
        self.RW, self.RH = W * ssaa, H * ssaa

    def camera(self, material, background, views, *camera):
        """The view matrices (``views``, or ``camera_views(*camera)``), the background colour or image and ``params``."""
        self.mats = camera_views(*camera) if views is None else \
            np.ascontiguousarray(np.asarray(views, dtype=np.float32).reshape(-1, 12))
        self.n_views = self.mats.shape[0]
        if self.n_views < 1:
            raise ValueError("no views")
        self.bg_img = None
        if isinstance(background, (np.ndarray, torch.Tensor)) and background.ndim == 3:
            self.bg_img = torch.as_tensor(background)
            if self.bg_img.dtype != torch.uint8 or tuple(self.bg_img.shape) != (self.H, self.W, 3):
                raise ValueError(f"a background image must be uint8 [{self.H},{self.W},3], got {self.bg_img.dtype} "
                                 f"{tuple(self.bg_img.shape)}")
        self.material = material
        self.params = material.params() if self.bg_img is not None else material.params(background)

    def allocate(self, dev, lead, id_name, return_buffers):
        """Views and background image to ``dev``; the outputs, ``lead`` in front of their shapes.  Only the image
        without ``return_buffers``."""
        self.d_views = torch.from_numpy(self.mats).to(dev)
        if self.bg_img is not None:
            self.bg_img = self.bg_img.to(dev).contiguous()
        lead = (*lead, self.n_views)
        self.image = torch.empty((*lead, self.H, self.W, 3), dtype=torch.uint8, device=dev)
        self.id_name, self.buffers = id_name, None
        if return_buffers:
            self.buffers = {id_name: torch.empty((*lead, self.RH, self.RW), dtype=torch.int32, device=dev),
                            "depth": torch.empty((*lead, self.RH, self.RW), dtype=torch.float32, device=dev),
                            "radiance": torch.empty((*lead, self.H, self.W, 3), dtype=torch.float32, device=dev)}

    def view_args(self):
        return _hip.ptr(self.d_views), self.n_views, self.RW, self.RH, self.ssaa, self.ortho_scale

    def shade_args(self, log2s, ws, stream, base_colors=True):
        """``base_colors``: the 17-float ``params`` of the entries that scale a base colour, K27's 15 otherwise."""
        scales = [float(self.material.ambient), float(self.material.diffuse)] if base_colors else []
        c_params = (ctypes.c_float * (15 + len(scales)))(*self.params.tolist(), *scales)
        b = self.buffers or {}
        return (c_params, log2s, _opt(self.bg_img), _hip.ptr(self.image), _opt(b.get("radiance")),
                _opt(b.get(self.id_name)), _opt(b.get("depth")), _hip.ptr(ws), ws.numel() * 8, stream)

    def result(self):
        return self.image if self.buffers is None else (self.image, self.buffers)


def render_views(verts: torch.Tensor, faces: torch.Tensor, *, size=600, elevations_deg=60.0,
                 azimuths_deg=range(0, 360, 30), radius: float = 3.0, ortho_scale: float = 2.0, up: str = "z",
                 ssaa: int = 2, background=(1.0, 1.0, 1.0), material: PhongMaterial = PhongMaterial(),
                 return_buffers: bool = False, views=None, scene: RenderScene | None = None, face_normals=None):
    """Orthographic, flat-shaded Phong views of a mesh (K27) -> uint8 ``[n_views, H, W, 3]`` on the mesh's device.

    ``size``: an int (square) or ``(H, W)``; the mesh is rasterised at ``size * ssaa`` and every output pixel is the
    mean of its ``ssaa^2`` samples over ``background``, an ``(r, g, b)`` in [0, 1] or a uint8 image ``[H, W, 3]`` (array
    or tensor) shared by the views.  The camera is ``camera_views(elevations_deg, azimuths_deg, radius, up)`` unless
    ``views [n,12]`` gives the matrices; ``ortho_scale`` world units span the image's larger side.  Both windings of
    a face are drawn and lit (ModelNet's are inconsistent).  With ``return_buffers`` also a dict: ``face_id`` int32 and
    ``depth`` float32 ``[n_views, H ssaa, W ssaa]`` (-1 / +inf where empty) and ``radiance`` float32 ``[n_views,H,W,3]``,
    of which the image is ``rint(clamp(radiance, 0, 1) * 255)``.  Bitwise the same on every run.

    With ``scene`` (a ``RenderScene``, see ``scene_tensors``) the shade pass is K28's: a face with a material takes its
    base colour from the material's ``Kd`` or texture in place of ``material.color``, scaled by ``material.ambient`` and
    ``material.diffuse``; a face without one is shaded as without ``scene``, and so are ``face_id`` and ``depth``.

    With ``face_normals`` (float32 ``[F,3,3]`` on the mesh's device: a world-space normal per corner, in the layout of
    ``face_uv``) the views are smooth-shaded (K31b): the light's terms take the normal interpolated at the sample, put
    on the side of the face the camera sees; where it has no length (zero or NaN corners) the face's own normal stays.
    Colours are ``scene``'s when it is given as well, ``material.color`` otherwise; ``face_id`` and ``depth`` do not change.

    ``ValueError`` for bad shapes and options, ``FpsgHipError`` for CPU tensors."""
    job = _RenderJob(size, ssaa, range(1, RENDER_MAX_SSAA + 1), f"an integer from 1 to {RENDER_MAX_SSAA}", ortho_scale)
    log2s = material.log2_shininess()
    job.camera(material, background, views, elevations_deg, azimuths_deg, radius, up)
    verts, faces = _mesh_tensors(verts, faces)
    dev = verts.device
    V, F = verts.size(0), faces.size(0)
    lib = _hip.load()
    if face_normals is not None:
        if not isinstance(face_normals, torch.Tensor) or face_normals.device != dev or \
                tuple(face_normals.shape) != (F, 3, 3):
            raise ValueError(f"face_normals must be a tensor {(F, 3, 3)} on {dev}, got "
                             f"{tuple(getattr(face_normals, 'shape', ()))} on {getattr(face_normals, 'device', None)}")
        face_normals = face_normals.detach().contiguous()
        _hip.dev_tensor(face_normals, torch.float32, "face_normals")
        if scene is None:                    # no materials: K27's colours
            scene = RenderScene(None, None, np.zeros((0, 4), np.float32), np.zeros((0, 3), np.int32), None)
    entry, scene_args, M, T = "fpsg_mesh_render", [], 0, 0
    if scene is not None:
        mat_table, tex_table, face_material, face_uv, texels = _scene_arguments(scene, F, dev)
        M, T = len(mat_table), len(tex_table)
        entry = "fpsg_mesh_render_materials" if face_normals is None else "fpsg_mesh_render_smooth"
        scene_args = [_opt(face_material), _opt(face_uv), *([] if face_normals is None else [_hip.ptr(face_normals)]),
                      mat_table.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if M else None, M,
                      tex_table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if T else None, T, _opt(texels),
                      0 if texels is None else texels.size(0)]
    # K27's workspace is K28's without tables
    ws_bytes = lib.fpsg_mesh_render_materials_workspace_bytes(V, F, job.n_views, job.RW, job.RH, M, T)
    if ws_bytes == 0:
        raise ValueError(f"unsupported render shape (V={V}, F={F}, views={job.n_views}, {job.RW}x{job.RH})")
    ws = torch.empty((ws_bytes // 16 + 1, 2), dtype=torch.int64, device=dev)
    job.allocate(dev, (), "face_id", return_buffers)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(_hip.ptr(verts), V, _hip.ptr(faces), F, *scene_args, *job.view_args(),
                                 *job.shade_args(log2s, ws, _hip.stream_of(verts), base_colors=scene is not None))
    _hip.check(rc, entry)
    return job.result()


# -------------------------------------------------------------------------------------------- K31a
def corner_table(faces, V: int):
    """The incidence table K31a walks -> ``(offsets int32 [V+1], corner_faces int32 [n])``: the slice
    ``corner_faces[offsets[v]:offsets[v+1]]`` lists the faces that name vertex ``v`` in ascending order, once per corner
    that names it.  A face with an index outside ``[0, V)`` is listed nowhere (K27 does not draw it either).  Built on the
    host by a stable numpy sort, once per topology: the meshes of a decoder share it."""
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"expected integer [F,3] faces, got {f.dtype} {f.shape}")
    if isinstance(V, bool) or int(V) != V or int(V) < 1:
        raise ValueError(f"V must be a positive integer, got {V}")
    V = int(V)
    f = f.astype(np.int64)
    ok = ((f >= 0) & (f < V)).all(axis=1)
    face = np.repeat(np.arange(len(f), dtype=np.int64)[ok], 3)       # ascending, a face's three corners side by side
    vert = f[ok].reshape(-1)
    order = np.argsort(vert, kind="stable")                          # stable: ascending faces inside every vertex
    offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(vert, minlength=V), out=offsets[1:])
    return offsets.astype(np.int32), face[order].astype(np.int32)


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor, table=None) -> torch.Tensor:
    """Area-weighted unit vertex normals (K31a) of one mesh ``[V,3]`` or of ``B`` meshes ``[B,V,3]`` that share
    ``faces [F,3]`` -> float32 of ``verts``' shape.  A vertex's normal is the sum of the un-normalised face normals
    ``(b - a) x (c - a)`` of the faces around it, divided by its length; ``(0, 0, 0)`` where that sum is zero or not
    finite (an isolated vertex, opposed faces).  ``table``: ``corner_table(faces, V)`` when the caller keeps it for a
    topology, built here otherwise; either array may be a numpy array or a tensor.  Bitwise the same on every run.

    ``ValueError`` for bad shapes, ``FpsgHipError`` for CPU tensors."""
    if not isinstance(verts, torch.Tensor) or verts.dim() not in (2, 3) or verts.size(-1) != 3 or verts.numel() == 0:
        raise ValueError(f"expected [V,3] or [B,V,3] vertices, got {tuple(getattr(verts, 'shape', ()))}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.size(1) != 3 or faces.size(0) < 1:
        raise ValueError(f"expected [F,3] faces, got {tuple(getattr(faces, 'shape', ()))}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must be int32 or int64, got {faces.dtype}")
    batch = verts.detach().reshape(-1, verts.size(-2), 3).contiguous()
    _hip.dev_tensor(batch, torch.float32, "verts")
    dev = batch.device
    if faces.device != dev:
        raise ValueError(f"faces are on {faces.device}, verts on {dev}")
    B, V, F = batch.size(0), batch.size(1), faces.size(0)
    if table is None:
        table = corner_table(faces, V)
    offsets, corner_faces = (torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous() for t in table)
    n = corner_faces.numel()
    if offsets.shape != (V + 1,) or corner_faces.dim() != 1 or n > 3 * F:
        raise ValueError(f"table must be (offsets [{V + 1}], corner_faces [n <= {3 * F}]), got {tuple(offsets.shape)} and "
                         f"{tuple(corner_faces.shape)}")
    faces = faces.to(torch.int32).contiguous()
    normals = torch.empty_like(batch)
    with torch.cuda.device(dev):
        rc = _hip.load().fpsg_mesh_vertex_normals(_hip.ptr(batch), B, V, _hip.ptr(faces), F, _hip.ptr(offsets),
                                                  _hip.ptr(corner_faces) if n else None, n, _hip.ptr(normals),
                                                  _hip.stream_of(batch))
    _hip.check(rc, "fpsg_mesh_vertex_normals")
    return normals.reshape(verts.shape)


# -------------------------------------------------------------------------------------------- K32
def _batched_mesh_tensors(verts, faces):
    """``_mesh_tensors``' checks for vertices ``[V,3]`` or ``[B,V,3]`` -> (verts detached and contiguous, faces int32)."""
    if not isinstance(verts, torch.Tensor) or verts.dim() not in (2, 3) or verts.size(-1) != 3 or verts.numel() == 0:
        raise ValueError(f"expected [V,3] or [B,V,3] vertices, got {tuple(getattr(verts, 'shape', ()))}")
    if verts.dtype != torch.float32:
        raise ValueError(f"verts must be float32, got {verts.dtype}")
    if verts.dim() == 2:
        return _mesh_tensors(verts.contiguous(), faces)
    V = verts.size(1)
    if V > MESH_MAX_FACES:
        raise ValueError(f"meshes of more than {MESH_MAX_FACES} vertices are not supported (got {V})")
    _, faces = _mesh_tensors(verts[0].contiguous(), faces)       # the faces' checks, against the V every mesh has
    return verts.detach().contiguous(), faces


def point_mesh_distance(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, *, closest: bool = False,
                        bary: bool = False, chunks=None) -> dict:
    """The nearest point of a triangle mesh for every point of a cloud (K32), exact, by brute force over the faces.

    ``points``: ``[N,3]`` (B = 1) or ``[B,N,3]`` float32; ``verts``: ``[V,3]``, one mesh for all clouds, or ``[B,V,3]``, a
    mesh per cloud; ``faces``: ``[F,3]`` int32 or int64, shared.  -> a dict: ``"dist2"`` float32 ``[B,N]``, the squared
    distance to the surface; ``"face"`` int64 ``[B,N]``, the nearest face (the lowest id on ties); with ``closest`` also
    ``"closest"`` float32 ``[B,N,3]``, the nearest point, and with ``bary`` ``"bary"`` float32 ``[B,N,3]``, its weights on
    the face's corners.  A point with a non-finite coordinate gets ``+inf``, ``-1`` and NaN.  Faces without area count as
    their edges.  ``chunks`` (1..64) splits the faces over that many workgroups per block of points; the bits do not
    depend on it, and the library chooses when it is None.  Forward only: inputs are detached.  Bitwise the same on
    every run.

    ``ValueError`` for bad shapes, dtypes or face indices outside the vertices; ``FpsgHipError`` for CPU tensors."""
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.size(-1) != 3 or points.numel() == 0:
        raise ValueError(f"expected [N,3] or [B,N,3] points, got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if chunks is not None and (isinstance(chunks, bool) or int(chunks) != chunks or
                               not 1 <= int(chunks) <= POINT_MESH_MAX_CHUNKS):
        raise ValueError(f"chunks must be None or an integer from 1 to {POINT_MESH_MAX_CHUNKS}, got {chunks}")
    pts = points.detach().reshape(-1, points.size(-2), 3).contiguous()
    B, N = pts.size(0), pts.size(1)
    verts, faces = _batched_mesh_tensors(verts, faces)
    per_mesh = verts.dim() == 3
    if per_mesh and verts.size(0) != B:
        raise ValueError(f"{verts.size(0)} meshes for {B} clouds")
    _hip.dev_tensor(pts, torch.float32, "points")
    dev = verts.device
    if pts.device != dev:
        raise ValueError(f"points are on {pts.device}, verts on {dev}")
    V, F = verts.size(-2), faces.size(0)
    if N > POINT_MESH_MAX_POINTS or B > POINT_MESH_MAX_MESHES or B * N > POINT_MESH_MAX_TOTAL:
        raise ValueError(f"up to {POINT_MESH_MAX_POINTS} points per cloud, {POINT_MESH_MAX_MESHES} clouds and "
                         f"{POINT_MESH_MAX_TOTAL} points in all are supported, got {B} x {N}")
    lib = _hip.load()
    c = 0 if chunks is None else int(chunks)
    ws_bytes = lib.fpsg_point_mesh_workspace_bytes(B, N, F, c)
    if ws_bytes == 0:
        raise ValueError(f"unsupported shape (B={B}, N={N}, F={F}, chunks={chunks})")
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    dist2 = torch.empty((B, N), dtype=torch.float32, device=dev)
    face = torch.empty((B, N), dtype=torch.int32, device=dev)
    q = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if closest else None
    w = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if bary else None
    with torch.cuda.device(dev):
        rc = lib.fpsg_point_mesh_distance(_hip.ptr(pts), B, N, _hip.ptr(verts), V, int(per_mesh), _hip.ptr(faces), F, c,
                                          _hip.ptr(dist2), _hip.ptr(face), None if q is None else _hip.ptr(q),
                                          None if w is None else _hip.ptr(w), _hip.ptr(ws), ws.numel() * 8,
                                          _hip.stream_of(pts))
    _hip.check(rc, "fpsg_point_mesh_distance")
    out = {"dist2": dist2, "face": face.long()}
    if closest:
        out["closest"] = q
    if bary:
        out["bary"] = w
    return out


def mesh_accuracy(verts: torch.Tensor, faces: torch.Tensor, cloud: torch.Tensor, *, n_samples=None, generator=None,
                  u=None) -> dict:
    """How well one mesh ``(verts [V,3], faces [F,3])`` reconstructs one ground-truth ``cloud [N,3]`` -> Python floats:

    - ``"completeness"``: the mean distance from the cloud's points to the surface (K32);
    - ``"accuracy"``: the mean distance from ``n_samples`` area-weighted surface samples (K26; default: the cloud's size;
      ``generator`` and ``u`` as in ``sample_surface``) to their nearest cloud points (K1);
    - ``"chamfer"``: the two directions' mean squared distances, summed;
    - ``"hausdorff"``: the larger of the two directions' largest distances.

    Square roots and means are taken in float64 on the device; the four numbers come back in one read.
    ``ValueError`` and ``FpsgHipError`` as ``point_mesh_distance`` and ``sample_surface``."""
    from .metrics import nearest_rows
    if not isinstance(cloud, torch.Tensor) or cloud.dim() != 2 or cloud.size(1) != 3 or cloud.size(0) < 1:
        raise ValueError(f"expected a [N,3] cloud, got {tuple(getattr(cloud, 'shape', ()))}")
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2:
        raise ValueError(f"expected [V,3] vertices, got {tuple(getattr(verts, 'shape', ()))}")
    n = cloud.size(0) if n_samples is None else n_samples
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f"n_samples must be a positive integer, got {n_samples}")
    cloud = cloud.detach().contiguous()
    to_surface = point_mesh_distance(cloud, verts, faces)["dist2"][0].to(torch.float64)
    samples, _ = sample_surface(verts, faces, int(n), generator=generator, u=u)
    to_cloud = nearest_rows(samples.unsqueeze(0), cloud.unsqueeze(0))[0][0].to(torch.float64)
    values = torch.stack([to_surface.sqrt().mean(), to_cloud.sqrt().mean(), to_surface.mean() + to_cloud.mean(),
                          torch.maximum(to_surface.max(), to_cloud.max()).sqrt()]).tolist()
    return dict(zip(("completeness", "accuracy", "chamfer", "hausdorff"), values))


def mesh_normal_consistency(verts: torch.Tensor, faces: torch.Tensor, cloud: torch.Tensor, *, k: int = 16, n_samples=None,
                            generator=None, u=None, cloud_normals=None) -> dict:
    """How well the surface directions of one mesh ``(verts [V,3], faces [F,3])`` agree with those of one ground-truth
    ``cloud [N,3]`` -> Python floats in [0, 1], signs not counted:

    - ``"to_surface"``: the mean over the cloud's points of ``|n_p . g_f|``, ``n_p`` the point's normal (K33 over ``k``
      neighbours with ``orient="none"``, or ``cloud_normals [N,3]``) and ``g_f`` the unit geometric normal of its nearest
      face (K32), zero for a face without area;
    - ``"to_cloud"``: the mean over ``n_samples`` surface samples (K26; default: the cloud's size; ``generator`` and ``u``
      as in ``sample_surface``) of ``|g_face(sample) . n_q|``, ``q`` the sample's nearest cloud point (K1);
    - ``"normal_consistency"``: their mean.

    Means are taken in float64 on the device; the three numbers come back in one read.  ``ValueError`` and
    ``FpsgHipError`` as ``point_mesh_distance``, ``sample_surface`` and ``normals.estimate_normals``."""
    from .metrics import nearest_rows
    from .normals import estimate_normals
    if not isinstance(cloud, torch.Tensor) or cloud.dim() != 2 or cloud.size(1) != 3 or cloud.size(0) < 1:
        raise ValueError(f"expected a [N,3] cloud, got {tuple(getattr(cloud, 'shape', ()))}")
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2:
        raise ValueError(f"expected [V,3] vertices, got {tuple(getattr(verts, 'shape', ()))}")
    n = cloud.size(0) if n_samples is None else n_samples
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f"n_samples must be a positive integer, got {n_samples}")
    cloud = cloud.detach().contiguous()
    if cloud_normals is None:
        cloud_normals = estimate_normals(cloud, k, orient="none")
    elif not isinstance(cloud_normals, torch.Tensor) or cloud_normals.shape != cloud.shape:
        raise ValueError(f"cloud_normals must have the cloud's shape {tuple(cloud.shape)}, got "
                         f"{tuple(getattr(cloud_normals, 'shape', ()))}")
    face = point_mesh_distance(cloud, verts, faces)["face"][0]
    samples, sample_face = sample_surface(verts, faces, int(n), generator=generator, u=u)
    nearest = nearest_rows(samples.unsqueeze(0), cloud.unsqueeze(0))[2][0].long()
    with torch.no_grad():
        corners = verts.detach().to(torch.float64)[faces.long()]                      # [F,3,3]
        g = torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
        length = g.norm(dim=1, keepdim=True)
        g = torch.where(length > 0, g / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(g))
        cn = cloud_normals.detach().to(device=cloud.device, dtype=torch.float64)
        to_surface = (cn * g[face.clamp(min=0)]).sum(-1).abs()
        to_surface = torch.where(face >= 0, to_surface, torch.zeros_like(to_surface)).mean()
        to_cloud = (g[sample_face] * cn[nearest]).sum(-1).abs().mean()
        values = torch.stack([to_surface, to_cloud, 0.5 * (to_surface + to_cloud)]).tolist()
    return dict(zip(("to_surface", "to_cloud", "normal_consistency"), values))


# -------------------------------------------------------------------------------------------- K29
def render_points(points: torch.Tensor, *, colors=None, size=256, elevations_deg=60.0, azimuths_deg=(0, 120, 240),
                  radius_cam: float = 3.0, ortho_scale: float = 2.0, up: str = "z", ssaa: int = 2,
                  point_radius: float = 0.02, background=(1.0, 1.0, 1.0), material: PhongMaterial = PhongMaterial(),
                  views=None, return_buffers: bool = False):
    """Orthographic Phong views of point clouds, every point a sphere of ``point_radius`` world units (K29) -> uint8
    ``[B, n_views, H, W, 3]`` on the clouds' device.

    ``points``: ``[N,3]`` (one cloud, B = 1) or ``[B,N,3]`` float32; ``colors``: uint8 of the same shape, a base colour per
    point in place of ``material.color`` (scaled by ``material.ambient`` and ``material.diffuse``, as ``render_views``
    does with a ``scene``).  ``size``, ``ssaa``, ``background``, ``ortho_scale``, ``up``, ``material`` and ``views`` mean
    what they mean in ``render_views``; the camera is ``camera_views(elevations_deg, azimuths_deg, radius_cam, up)``
    unless ``views`` gives the matrices, and every cloud is seen by all of them.  The nearest sphere wins each sample,
    the lowest point index on equal depth.  With ``return_buffers`` also a dict: ``point_id`` int32 and ``depth`` float32
    ``[B, n_views, H ssaa, W ssaa]`` (-1 / +inf where empty) and ``radiance`` float32 ``[B, n_views, H, W, 3]``, of which
    the image is ``rint(clamp(radiance, 0, 1) * 255)``.  Bitwise the same on every run, and a cloud's views do not depend
    on the batch it is rendered in.

    ``ValueError`` for bad shapes and options, before any GPU work; ``FpsgHipError`` for CPU tensors."""
    job = _RenderJob(size, ssaa, (1, 2, 4), "1, 2 or 4", ortho_scale)
    if not (point_radius > 0 and math.isfinite(point_radius)):
        raise ValueError(f"point_radius must be positive and finite, got {point_radius}")
    RW, RH = job.RW, job.RH
    # the entry's R, from the float32 values it is given
    R = round(256.0 * (float(np.float32(point_radius)) / float(np.float32(ortho_scale))) * max(RW, RH))
    if not 1 <= R <= 256 * POINTS_MAX_RADIUS_PX:
        raise ValueError(f"point_radius {point_radius} is {R / 256.0:.6g} sample pixels, from 1/256 to "
                         f"{POINTS_MAX_RADIUS_PX} are supported")
    log2s = material.log2_shininess()
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.size(-1) != 3 or points.numel() == 0:
        raise ValueError(f"expected [N,3] or [B,N,3] points, got {tuple(getattr(points, 'shape', ()))}")
    points = points.detach()
    if points.dim() == 2:
        points = points.unsqueeze(0)
        if isinstance(colors, torch.Tensor) and colors.dim() == 2:
            colors = colors.unsqueeze(0)
    B, N = points.size(0), points.size(1)
    if N > POINTS_MAX_N:
        raise ValueError(f"clouds of more than {POINTS_MAX_N} points are not supported (got {N})")
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or colors.dtype != torch.uint8 or tuple(colors.shape) != (B, N, 3):
            raise ValueError(f"colors must be a uint8 tensor {(B, N, 3)}, got {getattr(colors, 'dtype', None)} "
                             f"{tuple(getattr(colors, 'shape', ()))}")
        if colors.device != points.device:
            raise ValueError(f"colors are on {colors.device}, points on {points.device}")
    job.camera(material, background, views, elevations_deg, azimuths_deg, radius_cam, up)
    n_views = job.n_views
    if B * n_views >= 65536:
        raise ValueError(f"clouds * views must be below 65536, got {B} * {n_views}")
    points = points.contiguous()
    _hip.dev_tensor(points, torch.float32, "points")
    dev = points.device
    if colors is not None:
        colors = colors.detach().contiguous()
    lib = _hip.load()
    ws_bytes = lib.fpsg_points_render_workspace_bytes(B, N, n_views, RW, RH)
    if ws_bytes == 0:
        raise ValueError(f"unsupported render shape (B={B}, N={N}, views={n_views}, {RW}x{RH})")
    ws = torch.empty((ws_bytes // 16, 2), dtype=torch.int64, device=dev)
    job.allocate(dev, (B,), "point_id", return_buffers)
    with torch.cuda.device(dev):
        rc = lib.fpsg_points_render(_hip.ptr(points), _opt(colors), B, N, *job.view_args(), float(point_radius),
                                    *job.shade_args(log2s, ws, _hip.stream_of(points)))
    _hip.check(rc, "fpsg_points_render")
    return job.result()


# ------------------------------------------------------------------------------------- list files
def _write_pairs(path, pairs):
    with open(path, "w") as f:
        f.write("\n".join(f"{img}\t{pc}" for img, pc in pairs))     # no trailing newline, as the reference writes


def write_modelnet_lists(img_root: str, pc_root: str, output: str, train_classes=None, test_classes=None) -> dict:
    """The list files of the reference's ``generate_dataset.py`` (``--dataset modelnet``) for an existing tree
    ``<img_root>/<label>/<train|test>/<item>/<view>.png`` + ``<pc_root>/<label>/<split>/<item>.ply``:
    ``<output>/modelnet_train.txt`` (items of the base classes), ``<output>/modelnet_test.txt`` (novel classes) and
    ``<output>/modelnet_files/modelnet+<label>.txt`` for every class of either kind, every line
    ``<first view>\\t<item>.ply``, no newline after the last.  A novel class wins over a base class of the same name,
    other classes appear nowhere, items without views are left out -- all as there.  Unlike there, labels, items and
    views are taken in sorted order, so the files do not depend on the file system, and the view listed is the first
    of the sorted ones.  No GPU.  -> ``{"train": n, "test": n, "classes": [labels written]}``."""
    train_classes = MODELNET_TRAIN_CLASSES if train_classes is None else tuple(train_classes)
    test_classes = MODELNET_TEST_CLASSES if test_classes is None else tuple(test_classes)
    train, test, written = [], [], []
    os.makedirs(os.path.join(output, "modelnet_files"), exist_ok=True)
    for label in sorted(os.listdir(img_root)):
        if not os.path.isdir(os.path.join(img_root, label)):
            continue
        pairs = []
        for split in ("train", "test"):
            c_path = os.path.join(img_root, label, split)
            if not os.path.isdir(c_path):
                continue
            for item in sorted(os.listdir(c_path)):
                item_dir = os.path.join(c_path, item)
                if not os.path.isdir(item_dir):
                    continue
                views = sorted(os.listdir(item_dir))
                if views:
                    pairs.append((os.path.join(item_dir, views[0]), os.path.join(pc_root, label, split, f"{item}.ply")))
        if label in test_classes:
            test += pairs
        elif label in train_classes:
            train += pairs
        else:
            continue
        _write_pairs(os.path.join(output, "modelnet_files", f"modelnet+{label}.txt"), pairs)
        written.append(label)
    _write_pairs(os.path.join(output, "modelnet_train.txt"), train)
    _write_pairs(os.path.join(output, "modelnet_test.txt"), test)
    return {"train": len(train), "test": len(test), "classes": written}


def write_shapenet_lists(root: str, output: str, train_classes=None, test_classes=None) -> dict:
    """The list files of the reference's ``generate_dataset.py`` (``--dataset shapenet``) for an existing tree
    ``<root>/<synset>/<item>/models/{npy_file.npy, images/*}`` with its split files ``<root>/<synset>_train.txt`` and
    ``<root>/<synset>_test.txt`` (one item per line): ``<output>/shapenet_train.txt`` (every item of the base classes,
    of both splits, as there), ``<output>/shapenet_test.txt`` (novel classes) and
    ``<output>/shapenet_files/shapenet+<synset>.txt``, every line ``<root>/<synset>/<item>/models``, no newline after
    the last.  A synset of both kinds is listed in both files, as there.  Unlike there, items are taken in sorted order,
    only items that have ``npy_file.npy`` and at least one view are listed, and a class file is written only for a class
    that has a split file (the reference wrote one for each of the 55 synsets, mostly empty).  No GPU.
    -> ``{"train": n, "test": n, "classes": [synsets written]}``."""
    train_classes = SHAPENET_TRAIN_CLASSES if train_classes is None else tuple(train_classes)
    test_classes = SHAPENET_TEST_CLASSES if test_classes is None else tuple(test_classes)
    train, test, written = [], [], []
    os.makedirs(os.path.join(output, "shapenet_files"), exist_ok=True)
    for synset in sorted(set(train_classes) | set(test_classes)):
        names, found = set(), False
        for split in ("train", "test"):
            path = os.path.join(root, f"{synset}_{split}.txt")
            if os.path.isfile(path):
                found = True
                with open(path, "r") as f:
                    names |= {line.strip() for line in f if line.strip()}
        if not found:
            continue
        items = []
        for name in sorted(names):
            models = os.path.join(root, synset, name, "models")
            views = os.path.join(models, "images")
            if os.path.isfile(os.path.join(models, "npy_file.npy")) and os.path.isdir(views) and os.listdir(views):
                items.append(models)
        if synset in train_classes:
            train += items
        if synset in test_classes:
            test += items
        with open(os.path.join(output, "shapenet_files", f"shapenet+{synset}.txt"), "w") as f:
            f.write("\n".join(items))
        written.append(synset)
    for name, rows in (("shapenet_train.txt", train), ("shapenet_test.txt", test)):
        with open(os.path.join(output, name), "w") as f:
            f.write("\n".join(rows))
    return {"train": len(train), "test": len(test), "classes": written}


# -------------------------------------------------------------------------------------------- K34: checks of a mesh
def mesh_topology(faces, n_verts: int) -> dict:
    """What kind of surface the triangles ``faces [F,3]`` on ``n_verts`` vertices are, on the host in numpy -> a dict:

    - ``"edges"``: the undirected edges;
    - ``"boundary_edges"``: edges of one triangle; ``"nonmanifold_edges"``: edges of more than two;
    - ``"inconsistent_edges"``: edges of two triangles that run along them in the same direction (opposed windings);
    - ``"euler"``: ``n_verts - edges + F``, 2 for a sphere, 0 for a torus (every vertex counts, used or not);
    - ``"components"``: the connected components of the triangles (two triangles connect through a shared vertex);
    - ``"watertight"``: at least one triangle and none of the three kinds of edges above: a closed, consistently
      oriented manifold surface.

    ``ValueError`` for a shape other than ``[F,3]``, a non-integer type or an index outside ``[0, n_verts)``."""
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"expected integer [F,3] faces, got {f.dtype} {f.shape}")
    if isinstance(n_verts, bool) or int(n_verts) != n_verts or int(n_verts) < 0:
        raise ValueError(f"n_verts must be a non-negative integer, got {n_verts}")
    V, f = int(n_verts), f.astype(np.int64)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError(f"face indices must be in [0, {V}), got {int(f.min())}..{int(f.max())}")
    a, b = f.reshape(-1), f[:, (1, 2, 0)].reshape(-1)                  # the directed edges a -> b
    key = np.minimum(a, b) * max(V, 1) + np.maximum(a, b)
    uniq, inverse, count = np.unique(key, return_inverse=True, return_counts=True)
    forward = np.bincount(inverse, weights=(a < b), minlength=len(uniq))
    inconsistent = int(((count == 2) & (forward != 1)).sum())
    label = np.arange(V, dtype=np.int64)                               # components: the smallest vertex id reachable
    while f.size:
        low = label[f].min(axis=1)
        new = label.copy()
        np.minimum.at(new, f.reshape(-1), np.repeat(low, 3))
        new = new[new]                                                 # pointer jumping
        if np.array_equal(new, label):
            break
        label = new
    boundary, nonmanifold = int((count == 1).sum()), int((count > 2).sum())
    return {"edges": len(uniq), "boundary_edges": boundary, "nonmanifold_edges": nonmanifold,
            "inconsistent_edges": inconsistent, "euler": V - len(uniq) + len(f),
            "components": len(np.unique(label[f[:, 0]])) if f.size else 0,
            "watertight": bool(len(f) and not boundary and not nonmanifold and not inconsistent)}


def mesh_volume(verts, faces) -> float:
    """The signed volume a closed mesh encloses, ``sum a . (b x c) / 6`` over its triangles in float64 on the host:
    positive for a mesh that is counter-clockwise seen from outside, negative when its normals look inward.  For an
    open mesh the number depends on the origin."""
    v = np.asarray(verts.detach().cpu() if isinstance(verts, torch.Tensor) else verts, dtype=np.float64)
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"expected [V,3] vertices, got {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"expected integer [F,3] faces, got {f.dtype} {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"face indices must be in [0, {len(v)}), got {int(f.min())}..{int(f.max())}")
    f = f.astype(np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
