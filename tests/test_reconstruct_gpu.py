"""K34 on the GPU: the implicit field bit for bit against the dense float32 restatement (``_iso_ref.field32`` culls
nothing, so every bit also proves the kernel's cull conservative), against float64 within a derived bound, the marching-
tetrahedra kernels against the restatement's extraction, the Python layer end to end and ``generate_meshes.py
--implicit_grid``."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _iso_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TILE, BRICK = R.TILE, R.BRICK           # the LDS point tile and the brick side of fpsg_implicit_field


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cloud(B, N, seed):
    """B clouds on spheres of different radii and centres with their exact normals."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((B, N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    radii = np.linspace(0.8, 0.5, B)[:, None, None]
    centres = rng.uniform(-0.1, 0.1, (B, 1, 3))
    return (centres + radii * d).astype(R.F32), d.astype(R.F32)


def _run_field(gpu, P, Q, origin, cell, radius, G):
    from fpsg_amd import reconstruct
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu) for a in (P, Q, origin, cell, radius)]
    field, weight = reconstruct.field_on_grid(*dev, G, return_weight=True)
    alone = reconstruct.field_on_grid(*dev, G)                           # weight = NULL: the same field
    assert torch.equal(field.view(torch.int32), alone.view(torch.int32))
    return field.cpu().numpy(), weight.cpu().numpy()


def _compare_field(gpu, P, Q, origin, cell, radius, G):
    got_f, got_w = _run_field(gpu, P, Q, origin, cell, radius, G)
    out = []
    for b in range(len(P)):
        want_f, want_w = R.field32(P[b], Q[b], origin[b], cell[b], radius[b], G)
        assert np.array_equal(_bits(got_w[b]), _bits(want_w)), f"cloud {b}: weight"
        assert np.array_equal(_bits(got_f[b]), _bits(want_f)), f"cloud {b}: field (NaN pattern included)"
        out.append(want_f)
    return out


# ---- (a) the field, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, B, N, G", [
    ("N = 1", 1, 1, BRICK + 1),
    ("N = TILE - 1", 1, TILE - 1, BRICK + 1),
    ("N = TILE + 1", 1, TILE + 1, 12),
    ("G = 2", 1, 100, 2),
    ("G = BRICK + 1", 1, 100, BRICK + 1),
    ("G = 2 BRICK + 1", 1, 300, 2 * BRICK + 1),
    ("B = 3, N and G ragged", 3, 2 * TILE + 44, 13),
])
def test_field_bit_for_bit(gpu, name, B, N, G):
    P, Q = _cloud(B, N, 100 + N + G)
    # three different origins, cells and radii; the radius well below a brick's width, so whole tiles are culled
    cell = (np.asarray([2.4, 2.0, 2.9][:B]) / (G - 1)).astype(R.F32)
    origin = (np.asarray([[-1.2, -1.2, -1.2], [-1.0, -0.9, -1.1], [-1.5, -1.4, -1.45]][:B])).astype(R.F32)
    radius = np.asarray([0.3, 0.22, 0.41][:B], R.F32)
    fields = _compare_field(gpu, P, Q, origin, cell, radius, G)
    if G > BRICK and N > 1:
        for f in fields:                                    # both kinds of nodes occur: reached and not
            assert np.isnan(f).any() and np.isfinite(f).any()


# ---- (b) the field on an adversarial cloud ---------------------------------------------------------------------------------------
def test_field_adversarial_cloud(gpu):
    """Cell 1/8, radius 1/4: r r = 1/16 and inv = 16 are exact.  Cloud 0 has its nodes at -1 + i / 8, so node 8, the first
    of the second brick, lies at 0; cloud 1 at -7/8 + i / 8, so node 7, the last of the first brick, lies at 0.  Per axis a
    point sits exactly 1/4 from that node on the far side of the brick's face (-1/4 for cloud 0, +1/4 for cloud 1: d2 inv
    == 1, t = 0) and a second one ulp nearer (d2 inv = 1 - 2^-23: w = 2^-69).  No other point reaches those nodes, so a cull
    that dropped the nearer point would turn the node's finite value into NaN."""
    G, h, r = 2 * BRICK + 1, R.F32(0.125), R.F32(0.25)
    origin = np.asarray([[-1.0] * 3, [-0.875] * 3], R.F32)
    base_p, base_n = R.sphere_cloud(200, radius=0.3, seed=5)
    base_p = (base_p + R.F32(-0.5)).astype(R.F32)                         # in the first brick's corner, far from the nodes below
    P, Q, nodes, orders = [], [], [], []
    for b, (node_i, side) in enumerate(((BRICK, -1.0), (BRICK - 1, +1.0))):
        other = int(round((0.5 - float(origin[b, 0])) / 0.125))           # the node index at 0.5 on the other two axes
        special_p, special_n, at = [], [], []
        for axis in range(3):
            exact = np.full(3, 0.5, R.F32)
            exact[axis] = R.F32(side * 0.25)                              # a power of two, exactly the radius from the node at 0
            nearer = exact.copy()
            nearer[axis] = np.nextafter(exact[axis], R.F32(0))
            normal = np.zeros(3, R.F32)
            normal[axis] = side
            special_p += [exact, nearer]
            special_n += [normal, normal]
            idx = [other] * 3
            idx[axis] = node_i
            at.append(tuple(idx))
        p = np.concatenate([base_p, np.asarray(special_p, R.F32)])
        q = np.concatenate([base_n, np.asarray(special_n, R.F32)])
        p[3, 1] = np.nan                                                  # a NaN coordinate
        q[7, 2] = np.inf                                                  # an infinite normal component
        q[11] = 0.0                                                       # a zero normal
        p[20], q[20] = p[19], q[19]                                       # two identical points
        order = np.random.default_rng(9 + b).permutation(len(p))          # the special points anywhere in the tile
        P.append(p[order]); Q.append(q[order]); nodes.append(at); orders.append(order)
    P, Q = np.stack(P), np.stack(Q)
    cell, radius = np.asarray([h, h]), np.asarray([r, r])
    want = _compare_field(gpu, P, Q, origin, cell, radius, G)
    for b in range(2):
        ax = R.node_axes(origin[b], h, G)
        _, weight = R.field32(P[b], Q[b], origin[b], h, r, G)
        for axis, node in enumerate(nodes[b]):                            # only the nearer point gives these nodes a value
            assert ax[axis][node[axis]] == 0 and weight[node] == R.F32(2.0 ** -69) and np.isfinite(want[b][node]), (b, node)
        # dropping the nearer points (what a cull one ulp too eager would do) shows in the restatement
        keep = ~np.isin(orders[b], 200 + np.arange(1, 6, 2))
        dropped, _ = R.field32(P[b][keep], Q[b][keep], origin[b], h, r, G)
        assert all(np.isnan(dropped[node]) for node in nodes[b])


# ---- (c) the field against float64 ---------------------------------------------------------------------------------------------
def test_field_against_float64(gpu):
    G = 13
    P, Q = _cloud(1, 300, 77)
    origin, cell, radius = np.full((1, 3), -1.2, R.F32), np.asarray([2.4 / (G - 1)], R.F32), np.asarray([0.3], R.F32)
    got, _ = _run_field(gpu, P, Q, origin, cell, radius, G)
    f64, bound, scale, comparable = R.field64(P[0], Q[0], origin[0], cell[0], radius[0], G)
    assert comparable.sum() > 500
    assert np.isfinite(got[0][comparable]).all()
    err = np.abs(got[0].astype(np.float64) - f64)[comparable]
    print(f"K34a vs float64: max err / scale {np.max(err / scale[comparable]):.3e}, bound / scale median "
          f"{np.median(bound[comparable] / scale[comparable]):.3e} max {np.max(bound[comparable] / scale[comparable]):.3e}, "
          f"max err / bound {np.max(err / bound[comparable]):.3f}")
    assert (err <= bound[comparable]).all()


# ---- (d) the isosurface on uploaded analytic fields ------------------------------------------------------------------------------
def _fields():
    corner = np.ones((2, 2, 2), R.F32)
    corner[0, 0, 0] = -1
    return {"sphere": R.sphere_field(12), "torus": R.torus_field(16), "two_spheres": R.two_spheres_field(16),
            "positive": np.full((5, 5, 5), 0.25), "G = 2": corner, "zeros": R.zeros_field(12),
            "nan_slab": R.nan_slab_field(12)}


def _compare_surface(gpu, fields, origins, cells):
    """fields [B,G,G,G], origins [B,3], cells [B] (numpy float32) through the kernels against the restatement."""
    from fpsg_amd import reconstruct
    B, G = fields.shape[0], fields.shape[1]
    dev = [torch.from_numpy(a).to(gpu) for a in (fields, origins, cells)]
    out = reconstruct.iso_surface_packed(*dev)
    want = [R.extract(fields[b], origins[b], cells[b]) for b in range(B)]
    node_edges = np.concatenate([w["node_edges"] for w in want])
    cell_tris = np.concatenate([w["cell_tris"] for w in want])
    assert np.array_equal(out["node_edges"].cpu().numpy().reshape(-1), node_edges)
    assert np.array_equal(out["cell_tris"].cpu().numpy().reshape(-1), cell_tris)
    assert np.array_equal(out["edge_offset"].cpu().numpy(), np.cumsum(node_edges, dtype=np.int64) - node_edges)
    assert np.array_equal(out["tri_offset"].cpu().numpy(), np.cumsum(cell_tris, dtype=np.int64) - cell_tris)
    v_range = [0] + np.cumsum([len(w["verts"]) for w in want]).tolist()
    f_range = [0] + np.cumsum([len(w["faces"]) for w in want]).tolist()
    assert out["vert_range"] == v_range and out["face_range"] == f_range
    assert out["ranges"].cpu().tolist() == [v_range, f_range]            # as the kernel wrote them
    verts, faces = out["verts"].cpu().numpy(), out["faces"].cpu().numpy()
    assert verts.shape == (v_range[-1], 3) and faces.shape == (f_range[-1], 3) and faces.dtype == np.int32
    for b in range(B):
        v, f = verts[v_range[b]:v_range[b + 1]], faces[f_range[b]:f_range[b + 1]]
        assert np.array_equal(_bits(v), _bits(want[b]["verts"])), f"field {b}: vertices"
        assert np.array_equal(R.canonical_faces(f), R.canonical_faces(want[b]["faces"])), f"field {b}: faces"
    again = reconstruct.iso_surface_packed(*dev)                         # bitwise the same on every run, order included
    assert torch.equal(again["verts"].view(torch.int32), out["verts"].view(torch.int32))
    assert torch.equal(again["faces"], out["faces"])
    split = reconstruct.iso_surface(*dev)
    for b in range(B):
        assert torch.equal(split[b][0], out["verts"][v_range[b]:v_range[b + 1]])
        assert torch.equal(split[b][1], out["faces"][f_range[b]:f_range[b + 1]])
    return want


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "positive", "G = 2", "zeros", "nan_slab"])
def test_isosurface_on_analytic_fields(gpu, name):
    from fpsg_amd import meshes
    field = _fields()[name].astype(R.F32)
    origin, cell = R.unit_grid(field.shape[0])
    want = _compare_surface(gpu, field[None], origin[None], np.asarray([cell]))[0]
    topo = meshes.mesh_topology(want["faces"], len(want["verts"]))
    expect = {"sphere": (True, 2), "torus": (True, 0), "two_spheres": (True, 4), "zeros": (True, 2)}
    if name in expect:
        assert (topo["watertight"], topo["euler"]) == expect[name]
    elif name == "positive":
        assert len(want["verts"]) == 0 and len(want["faces"]) == 0
    else:
        assert topo["boundary_edges"] > 0 and topo["nonmanifold_edges"] == 0 and topo["inconsistent_edges"] == 0


def test_isosurface_of_three_fields(gpu):
    """B = 3 with three different fields, origins and cells: the ranges and the local indices."""
    fields = np.stack([_fields()[n].astype(R.F32) for n in ("sphere", "nan_slab", "zeros")])
    origins = np.asarray([[-1, -1, -1], [0.5, -2.0, 3.0], [-7.0, 0.25, 1.0]], R.F32)
    cells = np.asarray([2.0 / 11, 0.37, 1.5], R.F32)
    want = _compare_surface(gpu, fields, origins, cells)
    assert all(len(w["faces"]) > 0 and w["faces"].max() == len(w["verts"]) - 1 for w in want)
    empty = np.stack([fields[0], np.full_like(fields[0], 1.0), fields[2]])          # a cloud without a surface in the middle
    want = _compare_surface(gpu, empty, origins, cells)
    assert len(want[1]["verts"]) == 0 and len(want[2]["verts"]) > 0


# ---- (e) end to end -----------------------------------------------------------------------------------------------------------
def test_reconstruct_sphere_cloud_end_to_end(gpu):
    from fpsg_amd import meshes, reconstruct
    G = 24
    p, n = R.sphere_cloud(512, radius=0.8, seed=1)
    pts, nrm = torch.from_numpy(p).to(gpu), torch.from_numpy(n).to(gpu)
    field, origin, cell = reconstruct.implicit_field(pts, nrm, grid=G, radius_scale=1.5)
    radius = reconstruct.default_radius(pts[None], 16, 1.5)
    same, _, _ = reconstruct.implicit_field(pts, nrm, grid=G, radius=radius)          # the default radius, given
    assert torch.equal(field.view(torch.int32), same.view(torch.int32))
    o, c, r = origin.cpu().numpy()[0], cell.cpu().numpy()[0], radius.cpu().numpy()[0]
    e = float((p.max(axis=0) - p.min(axis=0)).max())
    assert abs(c - (e + 2 * r) / (G - 3)) < 1e-6 and np.abs(o + c * (G - 1) / 2 - (p.max(axis=0) + p.min(axis=0)) / 2).max() < 1e-6
    # the radius: 1.5 mean distances to the 16th neighbour, here by brute force in float64
    d = np.sqrt(((p[:, None].astype(np.float64) - p[None]) ** 2).sum(-1))
    assert abs(r - 1.5 * np.sort(d, axis=1)[:, 16].mean()) < 1e-5
    want_f, _ = R.field32(p, n, o, c, r, G)
    assert np.array_equal(_bits(field.cpu().numpy()[0]), _bits(want_f))
    want = R.extract(want_f, o, c)
    verts, faces = reconstruct.reconstruct_surface(pts, nrm, grid=G, radius_scale=1.5)
    assert np.array_equal(_bits(verts.cpu().numpy()), _bits(want["verts"]))
    assert np.array_equal(R.canonical_faces(faces.cpu().numpy()), R.canonical_faces(want["faces"]))
    topo = meshes.mesh_topology(faces, verts.size(0))
    print(f"K34 end to end: radius {r:.6f}, V {verts.size(0)}, F {faces.size(0)}, {topo}, volume "
          f"{meshes.mesh_volume(verts, faces):.6f}")
    assert topo["watertight"] and topo["euler"] == 2 and topo["components"] == 1
    assert (verts.size(0), faces.size(0)) == (2836, 5668)                # what the restatement gave for this input
    assert (topo["boundary_edges"], topo["nonmanifold_edges"]) == (0, 0)
    ball = 4.0 / 3.0 * np.pi * 0.8 ** 3
    assert 0.9 * ball < meshes.mesh_volume(verts, faces) < 1.25 * ball   # positive, and a sphere swollen by the field
    # vertex normals (K31a) look outward
    _, _, vn = reconstruct.reconstruct_surface(pts, nrm, grid=G, vertex_normals=True)
    assert float((vn * torch.nn.functional.normalize(verts, dim=1)).sum(-1).min()) > 0.5
    # normals=None: K33, oriented along the spanning forest; a batch returns a list
    meshes_b = reconstruct.reconstruct_surface(torch.stack([pts, pts * 0.5]), grid=G, orient="mst")
    assert isinstance(meshes_b, list) and len(meshes_b) == 2
    for scale, (v, f) in zip((1.0, 0.5), meshes_b):
        t = meshes.mesh_topology(f, v.size(0))
        assert t["watertight"] and t["euler"] == 2
        assert 0.9 * ball * scale ** 3 < meshes.mesh_volume(v, f) < 1.25 * ball * scale ** 3


# ---- (f) generate_meshes.py ------------------------------------------------------------------------------------------------------
def test_generate_meshes_with_implicit_grid(gpu, tmp_path):
    def run(tag, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "generate_meshes.py"), "--synthetic", "--n_shot", "2", "--n_query", "2",
               "--max_items", "1", "--grid", "4", "--metrics", "--output", str(tmp_path / tag), *extra]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        files = {os.path.relpath(os.path.join(d, n), tmp_path / tag): open(os.path.join(d, n), "rb").read()
                 for d, _, names in os.walk(tmp_path / tag) for n in names}
        return out.stdout.replace(str(tmp_path / tag), ""), files

    stdout, files = run("surface", "--implicit_grid", "24")
    surfaces = sorted(n for n in files if n.endswith("_surface.obj"))
    assert len(surfaces) == 2 and all(os.path.basename(n) == f"00000_q{k}_surface.obj" for k, n in enumerate(surfaces))
    for n in surfaces:
        rows = files[n].decode().split("\n")
        assert sum(ln.startswith("v ") for ln in rows) == sum(ln.startswith("vn ") for ln in rows) > 0
        assert sum(ln.startswith("f ") for ln in rows) > 0 and all("//" in ln for ln in rows if ln.startswith("f "))
    report = json.loads(files["metrics.json"])
    lines = [ln for ln in stdout.split("\n") if ln.startswith("Class: ")]
    print("\n".join(lines))
    assert report["surface"]["grid"] == 24 and sorted(report["surface"]["classes"]) == sorted(report["classes"])
    for name, row in report["surface"]["classes"].items():
        assert sorted(row) == ["accuracy", "chamfer", "completeness", "hausdorff", "meshes", "watertight"]
        assert row["meshes"] == 2 and 0 <= row["watertight"] <= 1
        line = next(ln for ln in lines if ln.startswith(f"Class: {name} [surface] -- "))
        parts = line.split(" -- ")[1].split("; ")
        assert [part.split(": ")[0] for part in parts] == ["P2S", "S2P", "Mesh CD", "Mesh HD", "Watertight"]
        assert float(parts[-1].split(": ")[1]) == row["watertight"]
    assert len(lines) == 2 * len(report["classes"])
    assert stdout.strip().split("\n")[-1].endswith("surfaces K33 + K34 on 24^3)")
    # without the flag: the files of before, byte for byte, and the flag changes none of them
    plain_out, plain = run("plain")
    assert not any("surface" in n for n in plain) and "surface" not in json.loads(plain["metrics.json"])
    assert "[surface]" not in plain_out and "K34" not in plain_out
    for n, data in plain.items():
        if n == "metrics.json":
            trimmed = {k: v for k, v in report.items() if k != "surface"}
            assert json.loads(data) == trimmed
        else:
            assert files[n] == data, n
    assert [ln for ln in lines if "[surface]" not in ln] == [ln for ln in plain_out.split("\n") if ln.startswith("Class: ")]
    with open(os.path.join(GOLDEN, "generate_meshes_grid4_sha256.json")) as fh:
        golden = json.load(fh)                       # recorded from the commit before --implicit_grid existed
    assert {n: hashlib.sha256(d).hexdigest() for n, d in plain.items()} == golden["files"]
    assert hashlib.sha256(plain_out.encode()).hexdigest() == golden["stdout"]
