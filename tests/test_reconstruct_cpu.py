"""K34 without a GPU: the marching-tetrahedra table generated from the header's rule, the numpy restatement of the
extraction on analytic fields, ``meshes.mesh_topology`` / ``mesh_volume``, the C ABI's refusals (on the host, before any
HIP call) and the Python layer's and the tools' argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _iso_ref as R
import _mesh_ref
from conftest import ROOT

FPSG_E_NULL, FPSG_E_SHAPE, FPSG_E_LIMIT = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def _mesh(field, G, dtype=R.F32):
    origin, cell = R.unit_grid(G)
    m = R.extract(np.asarray(field, dtype), origin, cell, dtype)
    return m, R.topology(m["faces"], len(m["verts"]))


# ---- (a) the table ---------------------------------------------------------------------------------------------------
def test_table_follows_the_rule():
    seen = set()
    for t in range(6):
        pos = np.asarray(R.tet_corners(t), np.float64)
        seen.add(tuple(map(tuple, pos.astype(int))))
        assert (pos[0] == 0).all() and (pos[3] == 1).all() and ((pos[1:] - pos[:-1]).sum(axis=1) == 1).all()
        for m in range(16):
            tris = R.case_triangles(t, m)
            inside = [p for p in range(4) if m >> p & 1]
            outside = [p for p in range(4) if not m >> p & 1]
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[len(inside)], (t, m)
            for tri in tris:
                assert len(set(tri)) == 3
                for p, q in tri:                          # every vertex sits on an edge from inside to outside
                    assert p < q and (p in inside) != (q in inside)
                mid = [0.5 * (pos[p] + pos[q]) for p, q in tri]
                normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                assert np.dot(normal, pos[outside].mean(axis=0) - pos[inside].mean(axis=0)) > 0, (t, m, tri)
            if len(tris) == 2:                            # the quad's two halves share its diagonal
                assert len(set(tris[0]) & set(tris[1])) == 2
    assert len(seen) == 6                                 # six different paths: the Kuhn split
    assert R.CLASSES == ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


# ---- (b) the restatement on analytic fields -------------------------------------------------------------------------------
@pytest.mark.parametrize("name, G, euler", [("sphere", 12, 2), ("torus", 16, 0), ("two_spheres", 16, 4)])
def test_restatement_closes_analytic_surfaces(name, G, euler):
    from fpsg_amd import meshes
    field = {"sphere": R.sphere_field, "torus": R.torus_field, "two_spheres": R.two_spheres_field}[name](G)
    m, topo = _mesh(field, G)
    assert topo == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0, "euler": euler}
    assert len(m["verts"]) == m["node_edges"].sum() and len(m["faces"]) == m["cell_tris"].sum()
    assert m["node_edges"].max() <= 7 and m["cell_tris"].max() <= 12
    assert (m["cell_tris"].reshape(G, G, G)[-1] == 0).all() and (m["cell_tris"].reshape(G, G, G)[:, :, -1] == 0).all()
    assert R.volume(m["verts"], m["faces"]) > 0          # counter-clockwise seen from outside
    ours = meshes.mesh_topology(m["faces"], len(m["verts"]))
    assert ours["watertight"] and ours["euler"] == euler and ours["components"] == (2 if name == "two_spheres" else 1)


def test_restatement_edge_cases():
    from fpsg_amd import meshes
    m, _ = _mesh(np.full((5, 5, 5), 0.25), 5)            # all positive: nothing
    assert m["verts"].shape == (0, 3) and m["faces"].shape == (0, 3) and not m["node_edges"].any()
    m, _ = _mesh(np.full((5, 5, 5), -0.25), 5)           # all negative: nothing either
    assert m["verts"].shape == (0, 3) and m["faces"].shape == (0, 3)
    corner = np.ones((2, 2, 2), R.F32)                   # G = 2: one cell, one corner inside
    corner[0, 0, 0] = -1
    m, topo = _mesh(corner, 2)
    assert len(m["verts"]) == 7 and len(m["faces"]) == 6 and topo["nonmanifold"] == 0 and topo["inconsistent"] == 0
    assert topo["boundary"] == 6                         # a fan around the corner, open at the cube's faces
    assert np.array_equal(np.sort(np.abs(m["verts"]).min(axis=1)), np.zeros(7, R.F32))      # t = 1/2 on every edge
    # exact zeros and -0.0 at nodes: not inside, vertices at t = 0 or 1, faces without area allowed, still a manifold
    zeros = R.zeros_field(12)
    assert (zeros == 0).sum() > 50 and np.signbit(zeros[zeros == 0]).any() and not np.signbit(zeros[zeros == 0]).all()
    m, topo = _mesh(zeros, 12)
    assert topo == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0, "euler": 2}
    assert np.isfinite(m["verts"]).all()
    # a NaN slab: the surface stops there and stays a manifold; no vertex on an edge with a NaN end
    slab = R.nan_slab_field(12)
    m, topo = _mesh(slab, 12)
    assert topo["boundary"] > 0 and topo["nonmanifold"] == 0 and topo["inconsistent"] == 0
    origin, cell = R.unit_grid(12)
    y_nan = R.node_axes(origin, cell, 12)[1][6]
    assert np.isfinite(m["verts"]).all() and np.abs(m["verts"][:, 1] - y_nan).min() >= 0.999 * cell
    ours = meshes.mesh_topology(m["faces"], len(m["verts"]))
    assert not ours["watertight"] and ours["boundary_edges"] == topo["boundary"] and ours["components"] == 2


# ---- (c) volumes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, G, exact, measured", [
    ("sphere", 12, 4.0 / 3.0 * np.pi * 0.7 ** 3, -0.0340),      # measured with the float64 restatement: -3.40 %
    ("torus", 16, 2.0 * np.pi ** 2 * 0.6 * 0.25 ** 2, -0.0483),  # -4.83 %: the chord error of a coarse grid
])
def test_volume_of_the_float64_restatement(name, G, exact, measured):
    field = {"sphere": R.sphere_field, "torus": R.torus_field}[name](G)
    m, _ = _mesh(field, G, np.float64)
    err = R.volume(m["verts"], m["faces"]) / exact - 1.0
    print(f"{name} G={G}: volume error {err:+.4%} (measured {measured:+.2%}, allowed {2 * abs(measured):.2%})")
    assert abs(err) <= 2 * abs(measured)
    m32, _ = _mesh(field, G)                                     # float32 moves the vertices by roundings only
    assert abs(R.volume(m32["verts"], m32["faces"]) / exact - 1.0 - err) < 1e-5


# ---- (d) mesh_topology and mesh_volume ----------------------------------------------------------------------------------------
def test_mesh_topology_and_volume_on_cubes():
    from fpsg_amd import meshes
    v, f = _mesh_ref.cube(-0.5, 1.0)
    topo = meshes.mesh_topology(f, len(v))
    assert topo == {"edges": 18, "boundary_edges": 0, "nonmanifold_edges": 0, "inconsistent_edges": 0, "euler": 2,
                    "components": 1, "watertight": True}
    assert abs(abs(meshes.mesh_volume(v, f)) - 1.5 ** 3) < 1e-12
    sign = np.sign(meshes.mesh_volume(v, f))
    assert meshes.mesh_volume(v, f[:, ::-1]) == -meshes.mesh_volume(v, f)
    assert meshes.mesh_volume(torch.from_numpy(v), torch.from_numpy(f)) == meshes.mesh_volume(v, f)
    assert R.volume(v, f) == meshes.mesh_volume(v, f) and sign != 0
    opened = meshes.mesh_topology(f[2:], len(v))                # one face (two triangles) removed
    assert opened["boundary_edges"] == 4 and opened["edges"] == 17 and not opened["watertight"]
    assert opened["nonmanifold_edges"] == 0 and opened["inconsistent_edges"] == 0 and opened["euler"] == 8 - 17 + 10
    flipped = f.copy()
    flipped[5] = flipped[5, ::-1]                               # one triangle reversed
    turned = meshes.mesh_topology(flipped, len(v))
    assert turned["inconsistent_edges"] == 3 and turned["boundary_edges"] == 0 and not turned["watertight"]
    assert turned["euler"] == 2
    two = meshes.mesh_topology(np.concatenate([f, f + 8]), 16)
    assert two["components"] == 2 and two["euler"] == 4 and two["watertight"]
    fin = meshes.mesh_topology(np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]]), 5)        # three triangles on one edge
    assert fin["nonmanifold_edges"] == 1 and not fin["watertight"]
    empty = meshes.mesh_topology(np.zeros((0, 3), np.int32), 0)
    assert empty["components"] == 0 and not empty["watertight"] and empty["euler"] == 0
    for bad in (np.zeros((3, 2), np.int32), np.zeros((2, 3), np.float32), np.array([[0, 1, 9]])):
        with pytest.raises(ValueError):
            meshes.mesh_topology(bad, 8)
    with pytest.raises(ValueError):
        meshes.mesh_volume(v, np.array([[0, 1, 8]]))
    # the same counts as the tests' own edge census
    for faces in (f, f[2:], flipped):
        ours, theirs = meshes.mesh_topology(faces, len(v)), R.topology(faces, len(v))
        assert (ours["boundary_edges"], ours["nonmanifold_edges"], ours["inconsistent_edges"], ours["euler"]) == \
               (theirs["boundary"], theirs["nonmanifold"], theirs["inconsistent"], theirs["euler"])


# ---- (e) the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_bound_and_refuse_on_the_host(lib):
    from fpsg_amd import _hip
    for name in ("fpsg_implicit_field", "fpsg_iso_classify", "fpsg_iso_emit"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    p = 0x100000                                                 # a fake, well-aligned, non-null pointer: never reached

    def field(B=1, N=8, G=8, ptr=p):
        return lib.fpsg_implicit_field(ptr, ptr, B, N, ptr, ptr, ptr, G, ptr, None, None)

    def classify(B=1, G=8, ptr=p):
        return lib.fpsg_iso_classify(ptr, B, G, ptr, ptr, None)

    def emit(B=1, G=8, nv=1, nf=1, ptr=p):
        return lib.fpsg_iso_emit(ptr, ptr, ptr, B, G, ptr, ptr, nv, nf, ptr, ptr, None, None, None)

    for call in (field, classify, emit):
        assert call(G=1) == FPSG_E_SHAPE and b"G" in lib.fpsg_last_error()
        assert call(G=1, ptr=None) == FPSG_E_SHAPE               # shapes and limits in front of the pointers
        assert call(B=0) == FPSG_E_SHAPE
        assert call(G=257) == FPSG_E_LIMIT and b"256" in lib.fpsg_last_error()
        assert call(G=257, ptr=None) == FPSG_E_LIMIT
        assert call(B=17, G=256) == FPSG_E_LIMIT and b"nodes" in lib.fpsg_last_error()      # 17 * 2^24 > 2^28
        assert call(B=(1 << 25) + 1, G=2) == FPSG_E_LIMIT
        assert call(ptr=None) == FPSG_E_NULL and b"null pointer" in lib.fpsg_last_error()
        assert call(ptr=p + 2) == -3                             # FPSG_E_ALIGN
    assert field(N=0) == FPSG_E_SHAPE and field(N=0, G=257) == FPSG_E_SHAPE
    assert field(N=16385) == FPSG_E_LIMIT and field(N=16385, ptr=None) == FPSG_E_LIMIT
    assert emit(nv=-1) == FPSG_E_SHAPE and emit(nf=-1) == FPSG_E_SHAPE
    assert emit(ptr=p + 4) == -3                                 # the 64-bit arrays: 8 bytes
    # verts and faces may be NULL with a zero count, and only then
    assert lib.fpsg_iso_emit(p, p, p, 1, 8, p, p, 1, 0, None, None, None, None, None) == FPSG_E_NULL
    assert lib.fpsg_iso_emit(p, p, p, 1, 8, p, p, 0, 1, None, None, None, None, None) == FPSG_E_NULL
    header = open(os.path.join(ROOT, "include", "fpsg_hip.h")).read()
    for word in ("#define FPSG_ISO_MIN_GRID 2", "#define FPSG_ISO_MAX_GRID 256", "#define FPSG_ISO_MAX_NODES (1 << 28)",
                 f"#define FPSG_FIELD_TILE {R.TILE}", f"#define FPSG_FIELD_BRICK {R.BRICK}", "K34", "parity UNPINNED"):
        assert word in header, word


# ---- (f) the Python layer and the tools ----------------------------------------------------------------------------------------
def test_python_errors_come_before_any_gpu_work():
    from fpsg_amd import reconstruct
    from fpsg_amd._hip import FpsgHipError
    pts, nrm = torch.rand(40, 3), torch.rand(40, 3)
    for kw in ({"grid": 3}, {"grid": 257}, {"grid": 8.0}, {"grid": True}, {"radius": 0.0}, {"radius": -1.0},
               {"radius": float("nan")}, {"radius": torch.ones(2)}, {"radius_scale": 0}, {"k": 2}, {"k": 33}, {"k": 40}):
        with pytest.raises(ValueError):
            reconstruct.implicit_field(pts, nrm, **kw)
        with pytest.raises(ValueError):
            reconstruct.reconstruct_surface(pts, nrm, **kw)
    for bad_p, bad_n in ((torch.rand(40, 2), torch.rand(40, 2)), (pts, nrm[:30]), (pts.double(), nrm.double()),
                         (pts, nrm.double()), (pts, None), (torch.rand(1, 16385, 3), torch.rand(1, 16385, 3))):
        with pytest.raises(ValueError):
            reconstruct.implicit_field(bad_p, bad_n)
    with pytest.raises(ValueError):
        reconstruct.implicit_field(torch.rand(17, 40, 3), torch.rand(17, 40, 3), grid=256)          # 17 * 2^24 nodes
    for kw in ({"orient": "none"}, {"orient": "up"}, {"up": "w"}, {"orient": torch.zeros(3)}, {"k": 40}):
        with pytest.raises(ValueError):
            reconstruct.reconstruct_surface(pts, **kw)
    origin, cell = torch.zeros(1, 3), torch.ones(1)
    for field in (torch.zeros(4, 4), torch.zeros(4, 4, 5), torch.zeros(1, 1, 1), torch.zeros(4, 4, 4).double(),
                  torch.zeros(257, 257, 257)):
        with pytest.raises(ValueError):
            reconstruct.iso_surface(field, origin, cell)
    with pytest.raises(ValueError):
        reconstruct.iso_surface(torch.zeros(2, 4, 4, 4), origin, cell)
    with pytest.raises(ValueError):
        reconstruct.iso_surface(torch.zeros(4, 4, 4), origin, torch.ones(2))
    # good arguments on the CPU: no fallback
    with pytest.raises(FpsgHipError):
        reconstruct.implicit_field(pts, nrm, grid=8)
    with pytest.raises(FpsgHipError):
        reconstruct.reconstruct_surface(pts, grid=8)
    with pytest.raises(FpsgHipError):
        reconstruct.iso_surface(torch.zeros(4, 4, 4), origin, cell)


def _tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, name), *args], capture_output=True, text=True, cwd=ROOT,
                          timeout=120)


def test_reconstruct_surface_tool_lists_and_checks_its_options(tmp_path):
    import reconstruct_surface as tool
    opt = tool.build_parser().parse_args(["--input", "a.npy", "b.ply"])
    assert (opt.input, opt.output, opt.grid, opt.k, opt.radius_scale, opt.orient, opt.up, opt.flip) == \
           (["a.npy", "b.ply"], "surfaces", 64, 16, 1.5, "mst", "z", False)
    opt = tool.build_parser().parse_args(["--input", "a.npy", "--grid", "32", "--k", "8", "--radius_scale", "2", "--orient",
                                          "outward", "--up", "y", "--flip", "--output", "o"])
    assert (opt.grid, opt.k, opt.radius_scale, opt.orient, opt.up, opt.flip, opt.output) == (32, 8, 2.0, "outward", "y", True, "o")
    for bad in (["--orient", "none"], ["--up", "x"], []):
        with pytest.raises(SystemExit):
            tool.build_parser().parse_args(bad if not bad else ["--input", "a.npy"] + bad)
    np.save(tmp_path / "few.npy", np.zeros((5, 3), np.float32))
    for args, word in ((("--grid", "3"), "--grid"), (("--grid", "257"), "--grid"), (("--k", "2"), "--k"),
                       (("--radius_scale", "0"), "--radius_scale"), (("--k", "8"), "too few")):
        out = _tool("reconstruct_surface.py", "--input", str(tmp_path / "few.npy"), "--output", str(tmp_path / "o"), *args)
        assert out.returncode != 0 and word in out.stderr and "Traceback" not in out.stderr, (args, out.stderr)
    assert not os.path.exists(tmp_path / "o")


def test_generate_meshes_lists_and_checks_implicit_grid():
    out = _tool("generate_meshes.py", "--help")
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stdout.replace("\n", " ")
    assert "--implicit_grid G" in text and "[default: 0 = off]" in text
    for value in ("3", "257", "-4"):
        out = _tool("generate_meshes.py", "--synthetic", "--implicit_grid", value)
        assert out.returncode != 0 and "--implicit_grid" in out.stderr and "4 to 256" in out.stderr, out.stderr
        assert "Traceback" not in out.stderr
