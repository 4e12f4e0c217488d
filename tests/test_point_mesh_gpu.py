"""K32 on the GPU: the nearest triangle of every point.  ``dist2``, ``face``, ``closest`` and ``bary`` are compared bit for
bit with the float32 restatement of the header (``_point_mesh_ref.py``) and, against its float64 evaluation, with the
bound derived there from the header's operations.  The kernel streams the faces in tiles of 256 and keeps 512 points per
workgroup; the shapes below stand on both sides of each."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import _mesh_ref as mref
import _point_mesh_ref as ref
import test_point_mesh_cpu as host
import test_surface_gpu as k31                    # its untrained model
from fpsg_amd import _hip, meshes, metrics, surface

pytestmark = pytest.mark.gpu

EPS = ref.EPS
TILE = 256
KEYS = ("dist2", "face", "closest", "bary")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _run(gpu, points, verts, faces, **kw):
    out = meshes.point_mesh_distance(torch.from_numpy(points).to(gpu), torch.from_numpy(verts).to(gpu),
                                     torch.from_numpy(faces).to(gpu), closest=True, bary=True, **kw)
    return {k: out[k].cpu().numpy() for k in KEYS}


def bent_grid(n_patches=16, g=6, seed=0):
    """``surface``'s g x g grid mesh, every patch bent by a smooth map of its own -> (verts [n g g, 3], faces)."""
    uv = surface.regular_grid(g).astype(np.float64)                        # [2, g g]
    rng = np.random.default_rng(seed)
    patches = []
    for _ in range(n_patches):
        c, k = rng.uniform(-0.6, 0.6, 3), rng.uniform(1, 3, 2)
        x, y = uv[0] - 0.5, uv[1] - 0.5
        patches.append(np.stack([c[0] + 0.4 * x, c[1] + 0.4 * y, c[2] + 0.1 * np.sin(k[0] * x) * np.cos(k[1] * y)], axis=1))
    return np.concatenate(patches).astype(np.float32), surface.patch_faces(g, n_patches)


def _cloud(n, seed, B=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, 3) if B is None else (B, n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (points [B,N,3], verts [V,3] or [B,V,3], faces, well_shaped)."""
    cube_v, cube_f = mref.cube()
    grid_v, grid_f = bent_grid()
    if name == "cube":                                # 12 faces, 3 x 1000 points: two point blocks, the second part full
        return _cloud(1000, 1, B=3), cube_v, cube_f, True
    if name == "grid":                                # the tool's 800 faces, a mesh per cloud
        v = np.stack([bent_grid(seed=s)[0] for s in range(3)])
        return _cloud(257, 2, B=3), v, grid_f, True
    if name == "grid-shared":
        return _cloud(63, 3, B=1), grid_v, grid_f, True
    F, N, B, per_mesh = {"random-1": (1, 1, 1, False), "random-255": (TILE - 1, 63, 3, True),
                         "random-257": (TILE + 1, 257, 1, False), "random-800": (800, 1000, 3, False),
                         "random-800-own": (800, 1, 3, True)}[name]
    _, v, f = host.random_triangles(0.3, F=F, N=1, seed=F)
    if per_mesh:
        v = np.stack([host.random_triangles(0.3, F=F, N=1, seed=F + b)[1] for b in range(B)])
    return _cloud(N, F, B=B), v, f, False


CASES = ("cube", "grid", "grid-shared", "random-1", "random-255", "random-257", "random-800", "random-800-own")


@pytest.mark.parametrize("name", CASES)
def test_bit_for_bit_the_restatement_and_within_the_bound_of_float64(gpu, name):
    """All four outputs equal the float32 restatement; ``dist2`` is within ``_point_mesh_ref.dist2_bound`` of the float64
    one (its docstring holds the derivation), at every point of the well-shaped meshes with a finite bound.  Random
    triangles may be slivers, whose interior candidate has no bound; where the bound is finite it holds there too."""
    points, verts, faces, well_shaped = case(name)
    got = _run(gpu, points, verts, faces)
    B, N = points.shape[:2]
    assert got["dist2"].shape == (B, N) and got["face"].dtype == np.int64 and got["closest"].shape == (B, N, 3)
    want = ref.point_mesh_batch(points, verts, faces, np.float32)
    for k, w in zip(KEYS, want):
        assert _same(got[k], w), k
    assert (got["face"] >= 0).all()
    for b in range(min(B, 2)):
        v = verts if verts.ndim == 2 else verts[b]
        d64 = ref.point_mesh(points[b], v, faces, np.float64)[0]
        bound = ref.dist2_bound(points[b], v, faces)
        err = np.abs(got["dist2"][b].astype(np.float64) - d64)
        print(f"{name}[{b}]: largest |dist2 - float64| = {err.max() / EPS:.2f} eps, bound up to "
              f"{bound[np.isfinite(bound)].max() / EPS:.1f} eps, largest error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
        if well_shaped:
            assert np.isfinite(bound).all() and bound.max() < 1e-3 * max(d64.max(), 1e-3)
    # without the optional outputs, int64 faces, one cloud without the batch axis: the same bits
    plain = meshes.point_mesh_distance(torch.from_numpy(points[0]).to(gpu), torch.from_numpy(verts).to(gpu)[
        (0,) if verts.ndim == 3 else ()], torch.from_numpy(faces).long().to(gpu))
    assert sorted(plain) == ["dist2", "face"] and plain["dist2"].shape == (1, N)
    assert _same(plain["dist2"].cpu().numpy()[0], want[0][0]) and _same(plain["face"].cpu().numpy()[0], want[1][0])


def test_the_chunk_split_and_the_run_do_not_change_a_bit(gpu):
    _, v, f = host.random_triangles(0.3, F=700, N=1, seed=5)
    points = _cloud(600, 6, B=2)
    base = _run(gpu, points, v, f, chunks=1)
    want = ref.point_mesh_batch(points, v, f, np.float32)
    for k, w in zip(KEYS, want):
        assert _same(base[k], w), k
    for chunks in (3, 7, 64, None, 1):
        other = _run(gpu, points, v, f, chunks=chunks)
        for k in KEYS:
            assert _same(other[k], base[k]), (chunks, k)


def test_ties_go_to_the_lower_face_and_points_of_the_surface_have_distance_zero(gpu):
    v, f = mref.cube()
    twice = np.repeat(f, 2, axis=0)                                       # face 2 k + 1 repeats face 2 k
    on = np.array([[.5, .5, .5], [-.5, .5, -.5], [.5, .5, 0], [0, -.5, -.5], [.5, .25, .125], [-.25, .375, -.5],
                   [0, 0, .5]], np.float32)                               # vertices, edge midpoints, inside faces
    points = np.concatenate([on, _cloud(300, 7)])[None]
    got = _run(gpu, points, v, twice)
    single = _run(gpu, points, v, f)
    assert (got["face"] % 2 == 0).all() and np.array_equal(got["face"], 2 * single["face"])
    for k in ("dist2", "closest", "bary"):
        assert _same(got[k], single[k]), k
    assert np.array_equal(got["dist2"][0, :len(on)], np.zeros(len(on), np.float32))
    assert np.array_equal(got["closest"][0, :len(on)], on)
    want = ref.point_mesh_batch(points, v, twice, np.float32)
    for k, w in zip(KEYS, want):
        assert _same(got[k], w), k


def _entry(gpu, points, verts, faces, chunks=0):
    """The C entry on device copies of the arrays, ``faces`` as they are -> (rc, dist2, face, closest, bary)."""
    lib = _hip.load()
    B, N = points.shape[:2]
    V, F = verts.shape[-2], len(faces)
    d_p, d_v = torch.from_numpy(points).to(gpu), torch.from_numpy(verts).to(gpu)
    d_f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(gpu)
    dist2 = torch.empty((B, N), dtype=torch.float32, device=gpu)
    face = torch.empty((B, N), dtype=torch.int32, device=gpu)
    closest, bary = torch.empty((B, N, 3), device=gpu), torch.empty((B, N, 3), device=gpu)
    ws_bytes = lib.fpsg_point_mesh_workspace_bytes(B, N, F, chunks)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=gpu)
    rc = lib.fpsg_point_mesh_distance(d_p.data_ptr(), B, N, d_v.data_ptr(), V, int(verts.ndim == 3), d_f.data_ptr(), F,
                                      chunks, dist2.data_ptr(), face.data_ptr(), closest.data_ptr(), bary.data_ptr(),
                                      ws.data_ptr(), ws_bytes, torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    return rc, dist2.cpu().numpy(), face.cpu().numpy(), closest.cpu().numpy(), bary.cpu().numpy()


def test_faces_out_of_range_are_skipped_and_never_read_through(gpu):
    """Through the C ABI (the wrapper refuses such faces): rows holding -1, V and 2^31 - 1 give the result of the mesh
    without those rows; a mesh of only such rows gives +inf / -1 and NaN."""
    v, f = bent_grid(4)
    V = len(v)
    rng = np.random.default_rng(11)
    bad = np.array([[-1, 0, 1], [0, V, 1], [0, 1, 2 ** 31 - 1], [-2 ** 31, -1, V], [V, V, V], [2 ** 31 - 1, 0, 0]], np.int32)
    where = np.sort(rng.choice(len(f) + 60, 60, replace=False))
    mixed = np.zeros((len(f) + 60, 3), np.int32)
    is_bad = np.zeros(len(mixed), bool)
    is_bad[where] = True
    mixed[is_bad] = bad[rng.integers(0, len(bad), 60)]
    mixed[~is_bad] = f
    new_id = np.nonzero(~is_bad)[0]
    points = _cloud(300, 12, B=2)
    rc, d2, face, closest, bary = _entry(gpu, points, v, mixed)
    assert rc == 0
    rc, d2_0, face_0, closest_0, bary_0 = _entry(gpu, points, v, f)
    assert rc == 0 and _same(d2, d2_0) and np.array_equal(face, new_id[face_0])
    assert _same(closest, closest_0) and _same(bary, bary_0)
    want = ref.point_mesh_batch(points, v, mixed, np.float32)
    assert _same(d2, want[0]) and np.array_equal(face, want[1])
    rc, d2, face, closest, bary = _entry(gpu, points, v, mixed[is_bad], chunks=3)
    assert rc == 0 and np.isposinf(d2).all() and (face == -1).all() and np.isnan(closest).all() and np.isnan(bary).all()


def test_non_finite_points_and_faces_without_area(gpu):
    v, f = bent_grid(4)
    points = _cloud(520, 13, B=1)
    clean = _run(gpu, points, v, f)
    spoilt = points.copy()
    spoilt[0, [3, 255, 256, 519], [0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan]
    got = _run(gpu, spoilt, v, f)
    hit = np.zeros(520, bool)
    hit[[3, 255, 256, 519]] = True
    assert np.isposinf(got["dist2"][0, hit]).all() and (got["face"][0, hit] == -1).all()
    assert np.isnan(got["closest"][0, hit]).all() and np.isnan(got["bary"][0, hit]).all()
    for k in KEYS:
        assert _same(got[k][0, ~hit], clean[k][0, ~hit]), k
    # faces without area behind the mesh's own: a point (a, a, a) and an edge (a, b, a) of every tenth face.  They are
    # parts of the surface, so they change nothing unless one is nearer, by the rounding of another order of operations
    flat = np.concatenate([f, f[::10][:, [0, 0, 0]], f[::10][:, [0, 1, 0]]])
    got = _run(gpu, points, v, flat)
    for k, w in zip(KEYS, ref.point_mesh_batch(points, v, flat, np.float32)):
        assert _same(got[k], w), k
    kept = got["face"][0] < len(f)
    for k in KEYS:
        assert _same(got[k][0, kept], clean[k][0, kept]), k
    assert (got["dist2"][0, ~kept] < clean["dist2"][0, ~kept]).all() and kept.mean() > 0.9
    bound = ref.dist2_bound(points[0], v, f) + ref.dist2_bound(points[0], v, flat)    # the two float64 values agree
    assert (clean["dist2"][0].astype(np.float64) - got["dist2"][0] <= bound + 1e-15).all()
    # in front of it and nearer: a far point becomes the nearest face of the points around it
    far = np.concatenate([v, [[5, 5, 5]]]).astype(np.float32)
    near_far = np.array([[5, 5, 4], [4.5, 5, 5]], np.float32)
    got = _run(gpu, np.concatenate([near_far, points[0]])[None], far, np.concatenate([[[len(v)] * 3], f]).astype(np.int32))
    assert np.array_equal(got["face"][0, :2], [0, 0]) and np.array_equal(got["dist2"][0, :2], np.array([1, .25], np.float32))
    assert np.array_equal(got["face"][0, 2:], clean["face"][0] + 1) and _same(got["dist2"][0, 2:], clean["dist2"][0])
    assert _same(got["closest"][0, :2], np.array([[5, 5, 5]] * 2, np.float32))


def test_a_sliver_mesh_stays_between_the_surface_and_its_vertices(gpu):
    """Aspect 1e4: det cancels and the interior candidate has no bound, so only the two sides that need none are checked
    (``_point_mesh_ref.one_sided_slacks``): never nearer than the surface, never farther than the nearest vertex."""
    rng = np.random.default_rng(17)
    F = 300
    a = rng.uniform(-0.8, 0.8, (F, 3))
    along = rng.normal(size=(F, 3))
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    across = np.cross(along, rng.normal(size=(F, 3)))
    across /= np.linalg.norm(across, axis=1, keepdims=True)
    L = 0.4
    tri = np.stack([a, a + L * along, a + 0.5 * L * along + 1e-4 * L * across], axis=1).astype(np.float32)
    v, f = tri.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    points = _cloud(500, 18)
    got = _run(gpu, points[None], v, f)
    want = ref.point_mesh(points, v, f, np.float32)
    for k, w in zip(KEYS, want):
        assert _same(got[k][0], w), k
    d64 = ref.point_mesh(points, v, f, np.float64)[0]
    below, above, T = ref.one_sided_slacks(points, v, f, d64)
    d2 = got["dist2"][0].astype(np.float64)
    print(f"sliver: dist2 - float64 from {((d2 - d64) / EPS).min():.2f} to {((d2 - d64) / EPS).max():.2f} eps; slack below "
          f"up to {below.max() / EPS:.1f} eps, above up to {above.max() / EPS:.1f} eps")
    assert np.isfinite(d2).all() and (d2 >= d64 - below).all() and (d2 <= T + above).all()


@pytest.mark.parametrize("name", ["cube", "grid"])
def test_surface_samples_lie_on_the_surface(gpu, name):
    """K26's samples against the geometry.  A sample p = (w0 a + w1 b) + w2 c has weights that sum to 1 within 3 u (1 - s,
    a difference and two products) and carries 3 u per coordinate from its own products and sums, so it lies within
    sigma = (3 + 3 sqrt(3)) u Q of its face, Q the largest |vertex|: the float64 distance is at most sigma, and K32's
    within its bound of that."""
    v, f = mref.cube() if name == "cube" else bent_grid()
    d_v, d_f = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    u = torch.rand((700, 3), generator=torch.Generator().manual_seed(3))
    samples, fidx = meshes.sample_surface(d_v, d_f, 700, u=u)
    out = meshes.point_mesh_distance(samples, d_v, d_f)
    p = samples.cpu().numpy()
    d64 = ref.point_mesh(p, v, f, np.float64)[0]
    bound = ref.dist2_bound(p, v, f)
    sigma = (3 + 3 * np.sqrt(3)) * EPS * np.linalg.norm(v, axis=1).max()
    d2 = out["dist2"][0].cpu().numpy().astype(np.float64)
    print(f"{name}: largest float64 distance {np.sqrt(d64.max()) / EPS:.2f} eps (sigma {sigma / EPS:.2f}), largest K32 dist2 "
          f"{d2.max():.3e}, largest bound {bound.max():.3e}")
    assert (np.sqrt(d64) <= sigma).all() and np.isfinite(bound).all()
    assert (d2 <= sigma ** 2 + bound).all() and (np.abs(d2 - d64) <= bound).all()


def test_the_surface_is_no_farther_than_its_vertices(gpu):
    """``dist2`` against K1's nearest vertex (``metrics.nearest_rows``): the surface contains its vertices.  K1 rounds two
    differences and three fused terms, 5 u relative, so T <= K1 (1 + 6 u); K32's side is ``one_sided_slacks``' ``above``."""
    v, f = bent_grid()
    points = _cloud(1000, 21)
    d_p, d_v = torch.from_numpy(points).to(gpu), torch.from_numpy(v).to(gpu)
    d2 = meshes.point_mesh_distance(d_p, d_v, torch.from_numpy(f).to(gpu))["dist2"][0].cpu().numpy().astype(np.float64)
    k1 = metrics.nearest_rows(d_p.unsqueeze(0), d_v.unsqueeze(0))[0][0].cpu().numpy().astype(np.float64)
    d64 = ref.point_mesh(points, v, f, np.float64)[0]
    _, above, T = ref.one_sided_slacks(points, v, f, d64)
    assert (np.abs(k1 - T) <= 5 * EPS * T).all()
    assert (d2 <= k1 * (1 + 6 * EPS) + above).all() and (d2 < k1).mean() > 0.5


def _completeness_tolerance(d32, d64, bound):
    """|sqrt(x) - sqrt(y)| <= |x - y| / (sqrt(x) + sqrt(y)) and <= sqrt(|x - y|); the mean of the smaller over the points."""
    with np.errstate(all="ignore"):
        root = np.sqrt(d32) + np.sqrt(d64)
        return np.minimum(np.where(root > 0, bound / np.where(root > 0, root, 1), np.inf), np.sqrt(bound)).mean() + 1e-15


def test_mesh_accuracy(gpu):
    v, f = mref.cube()
    d_v, d_f = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    gen = torch.Generator().manual_seed(5)
    cloud, _ = meshes.sample_surface(d_v, d_f, 600, u=torch.rand((600, 3), generator=gen))
    u = torch.rand((400, 3), generator=gen)
    # the mesh's own samples: completeness zero within the samples' distance (sigma, above) and K32's bound
    own = meshes.mesh_accuracy(d_v, d_f, cloud, n_samples=400, u=u)
    assert sorted(own) == ["accuracy", "chamfer", "completeness", "hausdorff"] and all(type(x) is float for x in own.values())
    p = cloud.cpu().numpy()
    sigma = (3 + 3 * np.sqrt(3)) * EPS * np.linalg.norm(v, axis=1).max()
    assert 0 <= own["completeness"] <= np.sqrt(sigma ** 2 + ref.dist2_bound(p, v, f)).mean()
    assert 0 < own["accuracy"] < 0.1 and own["hausdorff"] >= own["accuracy"] and 0 < own["chamfer"] < 0.01
    # the same cube moved by 0.25 along x, against float64
    moved = cloud + torch.tensor([0.25, 0.0, 0.0], device=gpu)
    q = moved.cpu().numpy()
    got = meshes.mesh_accuracy(d_v, d_f, moved, n_samples=400, u=u)
    d32 = meshes.point_mesh_distance(moved, d_v, d_f)["dist2"][0].cpu().numpy().astype(np.float64)
    d64 = ref.point_mesh(q, v, f, np.float64)[0]
    bound = ref.dist2_bound(q, v, f)
    tol = _completeness_tolerance(d32, d64, bound)
    want = np.sqrt(d64).mean()
    print(f"completeness {got['completeness']:.9f}, float64 {want:.9f}, tolerance {tol:.3e}")
    # (most of the tolerance is sqrt(bound) at the points that stay in a face's plane, where the root has no slope)
    assert abs(got["completeness"] - want) <= tol and 0.05 < want < 0.25 and tol < 1e-4
    samples, _ = meshes.sample_surface(d_v, d_f, 400, u=u)
    s = samples.cpu().numpy().astype(np.float64)
    to_cloud = ((s[:, None, :] - q.astype(np.float64)[None]) ** 2).sum(-1).min(axis=1)
    assert abs(got["accuracy"] - np.sqrt(to_cloud).mean()) <= 1e-6
    assert abs(got["chamfer"] - (d64.mean() + to_cloud.mean())) <= 1e-6
    assert abs(got["hausdorff"] - np.sqrt(max(d64.max(), to_cloud.max()))) <= 1e-6
    assert meshes.mesh_accuracy(d_v, d_f, moved, n_samples=400, u=u) == got                 # the same numbers again
    assert meshes.mesh_accuracy(d_v, d_f, moved)["completeness"] == got["completeness"]       # S defaults to the cloud's size


def test_generate_meshes_with_metrics(gpu, tmp_path):
    model, _, _ = k31._model_and_sample()
    state = {k: t.clone() for k, t in model.state_dict().items()}         # the widened weights of K31's end-to-end test
    for key, t in state.items():
        if key.endswith("deformer.conv1.weight"):
            t *= 10
        elif ".node_pool." in key and key.endswith("conv1.weight"):
            t[:, -3:] *= 400
    os.makedirs(tmp_path / "ckpt" / "0")
    torch.save(state, tmp_path / "ckpt" / "0" / "model.pt")

    def run(tag, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "generate_meshes.py"), "--synthetic", "--n_shot", "2", "--n_query", "2",
               "--grid", "6", "--max_items", "2", "--model_path", str(tmp_path / "ckpt"), "--name", "0", "--eval_model",
               "model.pt", "--output", str(tmp_path / tag), *extra]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        files = {os.path.relpath(os.path.join(d, n), tmp_path / tag): open(os.path.join(d, n), "rb").read()
                 for d, _, names in os.walk(tmp_path / tag) for n in names}
        return out.stdout.replace(str(tmp_path / tag), ""), files

    stdout, files = run("a", "--metrics")
    classes = sorted({os.path.dirname(n) for n in files if n.endswith(".obj")})
    lines = [ln for ln in stdout.split("\n") if ln.startswith("Class: ")]
    print("\n".join(lines))
    assert [ln.split(" -- ")[0] for ln in lines] == [f"Class: {c}" for c in classes]
    report = json.loads(files["metrics.json"])
    assert report["grid"] == 6 and report["faces"] == 800 and report["samples"] >= 1
    assert sorted(report["classes"]) == classes and sum(c["items"] for c in report["classes"].values()) == 2
    for ln, name in zip(lines, classes):
        row = report["classes"][name]
        labels = [part.split(": ")[0] for part in ln.split(" -- ")[1].split("; ")]
        values = [float(part.split(": ")[1]) for part in ln.split(" -- ")[1].split("; ")]
        assert labels == ["P2S", "S2P", "Mesh CD", "Mesh HD"]
        assert values == [row[k] for k in ("completeness", "accuracy", "chamfer", "hausdorff")]
        assert all(np.isfinite(x) and x >= 0 for x in values) and row["hausdorff"] >= max(row["completeness"], row["accuracy"])
    assert "distances K32 + K26 + K1" in stdout.strip().split("\n")[-1]
    again, files_b = run("b", "--metrics")
    assert again == stdout and files_b == files                            # byte for byte, metrics.json included
    plain, files_c = run("c")
    assert "Class: " not in plain and "K32" not in plain
    assert files_c == {n: data for n, data in files.items() if n != "metrics.json"}
