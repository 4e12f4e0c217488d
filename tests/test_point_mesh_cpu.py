"""K32 (the nearest triangle of every point), what needs no GPU: the numpy restatement of the header against an
independently written region algorithm and on exact cases, its float32 evaluation inside the derived bound, the C
entry's argument checks and the tool's options."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import _point_mesh_ref as ref

UNIT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
ONE_FACE = np.array([[0, 1, 2]], np.int32)


def random_triangles(size, F=200, N=400, seed=0):
    """F separate triangles of extent ``size`` and N points in [-1, 1]^3 -> (points, verts [3F,3], faces), float32."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (F, 3))
    tri = np.stack([a, a + rng.uniform(-size, size, (F, 3)), a + rng.uniform(-size, size, (F, 3))], axis=1)
    return (rng.uniform(-1, 1, (N, 3)).astype(np.float32), tri.reshape(-1, 3).astype(np.float32),
            np.arange(3 * F, dtype=np.int32).reshape(F, 3))


@pytest.mark.parametrize("size", [1.0, 0.1, 0.01])
def test_the_float64_restatement_equals_the_region_algorithm(size):
    pts, verts, faces = random_triangles(size)
    R = ref.face_records(verts, faces, np.float64)
    d = ref.pair_candidates(pts.astype(np.float64), R, np.float64)[0]
    tri = verts.reshape(-1, 3, 3).astype(np.float64)
    want = ref.ericson(pts[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    assert np.abs(d.min(axis=-1) - want).max() <= 1e-12
    # and over the faces: the minimum, the lowest face id
    d2, face, closest, bary = ref.point_mesh(pts, verts, faces, np.float64)
    assert np.array_equal(face, np.argmin(want, axis=1)) and np.abs(d2 - want.min(axis=1)).max() <= 1e-12
    corners = tri[face]
    assert np.abs((bary[:, :, None] * corners).sum(axis=1) - closest).max() <= 1e-12
    assert np.abs(((pts - closest) ** 2).sum(-1) - d2).max() <= 1e-12


REGIONS = [((.25, .25, 2), 4), ((-1, -1, 0), 2), ((2, 0, 0), 1), ((0, 3, 0), 4), ((.5, -1, 0), 1), ((-2, .5, 0), 4),
           ((1, 1, 0), 0.5), ((.25, .25, 0), 0), ((0, 0, 0), 0)]


def test_one_point_per_voronoi_region_is_exact_in_float32():
    pts = np.array([p for p, _ in REGIONS], np.float32)
    d2, face, closest, bary = ref.point_mesh(pts, UNIT, ONE_FACE, np.float32)
    assert d2.dtype == np.float32 and np.array_equal(d2, np.array([d for _, d in REGIONS], np.float32))
    assert np.array_equal(face, np.zeros(len(pts), np.int64))
    want_q = np.array([(.25, .25, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (.5, 0, 0), (0, .5, 0), (.5, .5, 0), (.25, .25, 0),
                       (0, 0, 0)], np.float32)
    assert np.array_equal(closest, want_q)
    assert np.array_equal((bary[:, :, None] * UNIT[None]).sum(axis=1), want_q) and np.array_equal(bary.sum(axis=1), np.ones(9))
    # q0 wins the tie at the corner a (both edges through it and no interior: the first candidate)
    assert np.array_equal(bary[8], [1, 0, 0]) and np.array_equal(bary[1], [1, 0, 0])


def test_degenerate_faces_degrade_to_their_edges():
    pts = np.array([[1, 2, 2], [0.25, 0, 1], [5, 0, 0], [-3, 4, 0]], np.float32)
    point = np.array([[1, 0, 0]] * 3, np.float32)                        # a face collapsed to one point
    d2, face, closest, bary = ref.point_mesh(pts, point, ONE_FACE, np.float32)
    assert np.array_equal(d2, ((pts - point[0]) ** 2).sum(-1)) and np.array_equal(face, np.zeros(4, np.int64))
    assert np.array_equal(closest, np.broadcast_to(point[0], (4, 3))) and np.array_equal(bary, [[1, 0, 0]] * 4)
    line = np.array([[0, 0, 0], [1, 0, 0], [4, 0, 0]], np.float32)        # collinear: the segment from 0 to 4
    d2, face, closest, _ = ref.point_mesh(pts, line, ONE_FACE, np.float32)
    assert np.array_equal(d2, np.array([8, 1, 1, 25], np.float32))
    assert np.array_equal(closest, np.array([[1, 0, 0], [.25, 0, 0], [4, 0, 0], [0, 0, 0]], np.float32))
    for v in (point, line):
        assert not np.isnan(ref.point_mesh(pts, v, ONE_FACE, np.float64)[0]).any()


def test_skipped_faces_and_non_finite_points():
    faces = np.array([[0, 1, 3], [0, 1, 2], [-1, 1, 2], [0, 1, 2]], np.int32)
    pts = np.array([[.25, .25, 2], [np.nan, 0, 0], [0, np.inf, 0], [.5, -1, 0]], np.float32)
    d2, face, closest, bary = ref.point_mesh(pts, UNIT, faces, np.float32)
    assert np.array_equal(face, [1, -1, -1, 1]) and np.array_equal(d2, np.array([4, np.inf, np.inf, 1], np.float32))
    assert np.isnan(closest[1:3]).all() and np.isnan(bary[1:3]).all() and not np.isnan(closest[[0, 3]]).any()
    d2, face, _, _ = ref.point_mesh(pts, UNIT, faces[[0, 2]], np.float32)
    assert np.array_equal(face, [-1] * 4) and np.isinf(d2).all()


@pytest.mark.parametrize("size", [1.0, 0.1, 0.01])
def test_the_float32_restatement_stays_inside_the_derived_bound(size):
    """The reference alone must meet its own bound: as a mesh of all the triangles, and pair by pair."""
    pts, verts, faces = random_triangles(size, seed=1)
    d32 = ref.point_mesh(pts, verts, faces, np.float32)[0].astype(np.float64)
    d64 = ref.point_mesh(pts, verts, faces, np.float64)[0]
    bound = ref.dist2_bound(pts, verts, faces)
    err = np.abs(d32 - d64)
    print(f"size {size}: largest error {err.max() / ref.EPS:.2f} eps, bound from {bound.min() / ref.EPS:.2f} to "
          f"{bound.max() / ref.EPS:.1f} eps, largest error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all() and np.isfinite(bound).all()
    assert bound.max() <= 2e-3 * max(d64.max(), 1e-3)                    # a bound that says something
    finite = 0
    for j in range(40):
        one = verts[3 * j:3 * j + 3]
        x32 = ref.point_mesh(pts, one, ONE_FACE, np.float32)[0].astype(np.float64)
        x64 = ref.point_mesh(pts, one, ONE_FACE, np.float64)[0]
        b = ref.dist2_bound(pts, one, ONE_FACE)
        assert (np.abs(x32 - x64) <= b).all()
        finite += int(np.isfinite(b).sum())
    assert finite > 0.9 * 40 * len(pts)


# ---- the C entry -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def test_entry_refuses_bad_arguments_before_any_hip_call(lib):
    from fpsg_amd import _hip, meshes
    assert "fpsg_point_mesh_distance" in _hip.SIGNATURES and "fpsg_point_mesh_workspace_bytes" in _hip.SIGNATURES
    assert lib.fpsg_point_mesh_workspace_bytes.restype is ctypes.c_size_t

    fake = 4096                                    # non-null and aligned; nothing dereferences it on these paths
    big = 1 << 40

    def call(points=fake, B=2, N=100, verts=fake, V=8, per_mesh=0, faces=fake, F=12, chunks=0, dist2=fake, face=fake,
             closest=None, bary=None, ws=fake, ws_bytes=big):
        return lib.fpsg_point_mesh_distance(points, B, N, verts, V, per_mesh, faces, F, chunks, dist2, face, closest, bary,
                                            ws, ws_bytes, None)

    for name in ("points", "verts", "faces", "dist2", "face", "ws"):
        assert call(**{name: None}) == -1 and name.encode() in lib.fpsg_last_error(), name
    for name in ("B", "N", "V", "F"):
        for bad in (0, -3):
            assert call(**{name: bad}) == -2, (name, bad)
            assert call(**{name: bad, "points": None}) == -2                 # shapes in front of the pointers
    assert call(per_mesh=2) == -2 and b"verts_per_mesh" in lib.fpsg_last_error()
    assert call(per_mesh=-1) == -2
    assert call(N=meshes.POINT_MESH_MAX_POINTS + 1, B=1) == -4
    assert call(N=meshes.POINT_MESH_MAX_POINTS, B=65) == -4                   # B N beyond the total
    assert call(B=65536, N=1) == -4 and call(F=meshes.MESH_MAX_FACES + 1) == -4 and call(V=meshes.MESH_MAX_FACES + 1) == -4
    assert call(chunks=65) == -4 and call(chunks=65, points=None) == -4
    need = lib.fpsg_point_mesh_workspace_bytes(2, 100, 12, 3)
    assert need == 2 * 100 * 3 * 8
    assert call(chunks=3, ws_bytes=need - 1) == -2 and b"workspace" in lib.fpsg_last_error()
    assert call(chunks=3, ws_bytes=need, ws=None) == -1
    assert call(points=fake + 2) == -3 and call(ws=fake + 4) == -3 and call(closest=fake + 1) == -3
    # the library's choice: at least one slice, at most 64
    for B, N, F in ((1, 1, 1), (5, 2048, 7200), (1, 15000, 100000), (64, 1 << 20, 1 << 24)):
        c = lib.fpsg_point_mesh_workspace_bytes(B, N, F, 0) // (8 * B * N)
        assert 1 <= c <= 64 and lib.fpsg_point_mesh_workspace_bytes(B, N, F, 0) == c * 8 * B * N, (B, N, F)
    assert lib.fpsg_point_mesh_workspace_bytes(1, 1, 1, 0) == 8
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 65), (1, (1 << 20) + 1, 8, 1), (65536, 1, 8, 1),
                (65, 1 << 20, 8, 1), (1, 8, (1 << 24) + 1, 1), (-1, -1, -1, -1)):
        assert lib.fpsg_point_mesh_workspace_bytes(*bad) == 0, bad


def test_wrapper_refuses_bad_inputs_without_a_gpu():
    import torch

    from fpsg_amd import meshes
    from fpsg_amd._hip import FpsgHipError
    v, f, p = torch.from_numpy(UNIT), torch.from_numpy(ONE_FACE), torch.zeros(4, 3)
    with pytest.raises(FpsgHipError):
        meshes.point_mesh_distance(p, v, f)                                  # CPU tensors: no fallback
    with pytest.raises(FpsgHipError):
        meshes.mesh_accuracy(v, f, p)
    for bad in (torch.zeros(4, 2), torch.zeros(3), torch.zeros(0, 3), torch.zeros(4, 3, dtype=torch.float64), "x"):
        with pytest.raises(ValueError, match="points"):
            meshes.point_mesh_distance(bad, v, f)
    for bad in (torch.zeros(3, 2), torch.zeros(2, 2, 3, 3), UNIT, v.double()):
        with pytest.raises(ValueError, match="vert"):
            meshes.point_mesh_distance(p, bad, f)
    for bad in (f.float(), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(0, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="faces"):
            meshes.point_mesh_distance(p, v, bad)
    for bad in (0, 65, 1.5, True):
        with pytest.raises(ValueError, match="chunks"):
            meshes.point_mesh_distance(p, v, f, chunks=bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="n_samples"):
            meshes.mesh_accuracy(v, f, p, n_samples=bad)
    with pytest.raises(ValueError, match="cloud"):
        meshes.mesh_accuracy(v, f, torch.zeros(2, 4, 3))


# ---- the tool ----------------------------------------------------------------------------------------------------------------

def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "generate_meshes.py"), *args], capture_output=True, text=True,
                          cwd=ROOT, timeout=120)


def test_generate_meshes_lists_and_checks_the_metrics_options():
    out = _tool("--help")
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--metrics " in out.stdout.replace("\n", " ") and "--metrics_samples" in out.stdout
    out = _tool("--synthetic", "--metrics", "--metrics_samples", "0")
    assert out.returncode != 0 and "--metrics_samples" in out.stderr and "Traceback" not in out.stderr
    out = _tool("--synthetic", "--metrics_samples", "8")
    assert out.returncode != 0 and "--metrics_samples" in out.stderr and "--metrics" in out.stderr
    assert "Traceback" not in out.stderr
