"""K33 on the GPU (``include/fpsg_hip.h``): the neighbour lists bit for bit against the numpy restatement, the normals
against float64 PCA on the same neighbour sets within the derived bound, the sign rules, the degenerate clouds, the
spanning forest of K33b against its restatement, the host functions and the two tools."""
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
import _point_mesh_ref as pmref
import _point_normals_ref as ref
import test_surface_gpu as k31                    # its untrained model
from fpsg_amd import meshes, metrics, normals

pytestmark = pytest.mark.gpu

U = ref.U


def _estimate(gpu, x, k, mode=0, viewpoint=None):
    """K33a on numpy clouds ``[B,N,3]`` -> numpy ``(normals, variation, idx)``."""
    pts = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(gpu)
    r = None if viewpoint is None else torch.from_numpy(np.ascontiguousarray(viewpoint, np.float32)).to(gpu)
    n, v, i = normals.point_normals(pts, k, mode, r, variation=True, neighbors=True)
    torch.cuda.synchronize()
    return n.cpu().numpy(), v.cpu().numpy(), i.cpu().numpy()


def _orient(gpu, x, n, idx, axis=2):
    out, par = normals.orient_normals(torch.from_numpy(x).to(gpu), torch.from_numpy(n).to(gpu),
                                      torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(gpu), axis, parents=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), par.cpu().numpy()


def _random_clouds(B, N, seed):
    return np.random.default_rng(seed).standard_normal((B, N, 3)).astype(np.float32)


# ---- (a) neighbour lists --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k", [(1, 4, 3), (3, 63, 8), (3, 64, 16), (2, 65, 32), (2, 257, 16), (1, 33, 32),
                                     (2, 70, 9), (2, 70, 17)])       # the first k of pn_select_kernel<16> and <32>
def test_lists_equal_the_restatement(gpu, B, N, k):
    x = _random_clouds(B, N, 100 + N)
    _, _, idx = _estimate(gpu, x, k)
    assert idx.dtype == np.int32 and idx.shape == (B, N, k)
    for b in range(B):
        assert np.array_equal(idx[b], ref.neighbour_lists(x[b], k)), (b, N, k)


def test_lists_on_ties_and_duplicates(gpu):
    grid = ref.planar_grid(5)
    for k in (5, 8, 24):
        n, var, idx = _estimate(gpu, grid[None], k)
        assert np.array_equal(idx[0], ref.neighbour_lists(grid, k)), k
        assert np.array_equal(np.abs(n[0]), np.tile(np.float32([0, 0, 1]), (25, 1))) and (n[0][:, 2] == 1).all()
        assert np.abs(var).max() <= (2 * (k + 4) + 32) * U
    assert idx[0, 0, :5].tolist() == [1, 5, 6, 2, 10]
    p = _random_clouds(1, 40, 7)[0]
    x = np.concatenate([p, p])
    _, _, idx = _estimate(gpu, x[None], 9)
    assert np.array_equal(idx[0], ref.neighbour_lists(x, 9))
    assert idx[0, :40, 0].tolist() == list(range(40, 80)) and idx[0, 40:, 0].tolist() == list(range(40))


@pytest.mark.parametrize("N", [9, 65, 1030])         # the smallest cloud for k = 8; past K33a's 64 threads; past one tile
def test_lists_are_the_repulsion_lists(gpu, N):
    """One definition: K33a and K21 keep the lexicographic (d2, j) top-8 over the same sq_dist (csrc/self_knn.h)."""
    x = torch.from_numpy(_random_clouds(2, N, 33)).to(gpu)
    idx = normals.point_normals(x, 8, neighbors=True)[-1]
    rep = metrics.repulsion_loss(x, k=8, return_info=True)[1]["idx"]
    assert idx.shape == rep.shape == (2, N, 8)
    assert torch.equal(idx, rep)


# ---- (b) normals against float64 -------------------------------------------------------------------------------------
SHAPES = {
    "sphere": lambda n: ref.sphere(n, 1)[0],
    "small-offset-sphere": lambda n: ref.sphere(n, 1, 0.05, (10.0, -7.0, 3.0))[0],
    "cube": lambda n: ref.cube_surface(n, 2),
    "torus": lambda n: ref.torus(n, 3)[0],
    "blob": lambda n: ref.blob(n, 4),
}


@functools.lru_cache(maxsize=None)
def _reference(name, N, k):
    x = SHAPES[name](N)
    idx = ref.neighbour_lists(x, k)
    n64, lam, _ = ref.pca64(x, idx)
    return x, idx, n64, lam


@pytest.mark.parametrize("N,k", [(300, 8), (512, 16), (700, 32)])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_normals_within_the_bound_of_float64_pca_on_the_same_neighbours(gpu, name, N, k):
    """Largest observed sin / bound over the fifteen cases on the MI355X: 0.024."""
    x, idx, n64, lam = _reference(name, N, k)
    n, var, got_idx = _estimate(gpu, x[None], k)
    assert np.array_equal(got_idx[0], idx)
    trace = lam.sum(axis=1)
    ok = (lam[:, 1] - lam[:, 0]) / trace >= 1e-3
    assert (~ok).mean() <= 0.02
    ratio = ref.sin_angle(n[0], n64)[ok] / ref.angle_bound(k, lam)[ok]
    norm = np.abs((n[0].astype(np.float64) ** 2).sum(axis=1) - 1)
    dvar = np.abs(var[0] - lam[:, 0] / trace)
    print(f"{name} N={N} k={k}: excluded {(~ok).mean():.3f}, largest sin/bound {ratio.max():.4f}, "
          f"| |n|^2 - 1 | {norm.max() / U:.2f} u, variation {dvar.max() / U:.2f} u of {(2 * (k + 4) + 32)} u")
    assert ratio.max() <= 1.0
    assert norm.max() <= 8 * U
    assert dvar.max() <= (2 * (k + 4) + 32) * U and (var >= 0).all() and (var <= np.float32(1) / np.float32(3)).all()
    assert ref.canonical_sign_ok(n[0]).all()


# ---- (c) sign modes --------------------------------------------------------------------------------------------------
def _toward32(n, x, r):
    """The header's fp32 expression e = (nx (rx - px) + ny (ry - py)) + nz (rz - pz)."""
    d = np.float32(r)[None, :] - x
    return (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]


def test_sign_modes(gpu):
    x = np.stack([ref.sphere(300, 11, 0.5, (0.2, 0.1, -0.3))[0], ref.torus(300, 12)[0]])
    view = np.float32([[3.0, 2.0, 1.0], [0.0, 0.0, 0.0]])
    n0, _, _ = _estimate(gpu, x, 8, 0)
    n1, _, _ = _estimate(gpu, x, 8, 1, view)
    n2, _, _ = _estimate(gpu, x, 8, 2, view)
    for b in range(2):
        assert ref.canonical_sign_ok(n0[b]).all()
        e = _toward32(n0[b], x[b], view[b])
        assert np.array_equal(n1[b], np.where((e < 0)[:, None], -n0[b], n0[b]))      # bitwise, up to the negation
        assert np.array_equal(n2[b], np.where((e > 0)[:, None], -n0[b], n0[b]))
        assert (_toward32(n1[b], x[b], view[b]) >= 0).all() and (_toward32(n2[b], x[b], view[b]) <= 0).all()
        assert (e < 0).sum() >= 10 and (e > 0).sum() >= 10                              # both branches are taken
    # away from the centre of a sphere is its outward normal
    outward = ref.sphere(300, 11)[1]
    centre = np.float32([[0.2, 0.1, -0.3], [0.0, 0.0, 0.0]])
    away, _, _ = _estimate(gpu, x, 8, 2, centre)
    assert ((away[0].astype(np.float64) * outward).sum(axis=1) > 0).all()


# ---- (d) degenerates -------------------------------------------------------------------------------------------------
def test_degenerate_clouds(gpu):
    same = np.tile(np.float32([[0.3, -1.5, 2.0]]), (20, 1))
    n, var, idx = _estimate(gpu, same[None], 5)
    assert not n.any() and not var.any() and np.array_equal(idx[0], ref.neighbour_lists(same, 5))
    t = np.arange(40, dtype=np.float64)[:, None]
    line = (t * np.array([1.0, 2.0, -2.0]) + np.array([5.0, 0.0, -3.0])).astype(np.float32)     # integers: exactly collinear
    k = 6
    n, var, idx = _estimate(gpu, line[None], k)
    assert np.array_equal(idx[0], ref.neighbour_lists(line, k))
    _, lam, _ = ref.pca64(line, idx[0])
    along = np.abs(n[0].astype(np.float64) @ (np.array([1.0, 2.0, -2.0]) / 3))
    print(f"collinear: largest |n . dir| {along.max():.3e}, bound {ref.angle_bound(k, lam, lam[:, 2]).min():.3e}")
    assert (along <= ref.angle_bound(k, lam, lam[:, 2])).all()
    assert np.abs((n[0].astype(np.float64) ** 2).sum(axis=1) - 1).max() <= 8 * U
    assert np.abs(var).max() <= (2 * (k + 4) + 32) * U


def test_a_nan_coordinate_spoils_its_own_cloud_only(gpu):
    x = _random_clouds(3, 70, 21)
    clean = [_estimate(gpu, x[b:b + 1], 8) for b in (0, 2)]
    x[1, 13, 1] = np.nan
    n, var, idx = _estimate(gpu, x, 8)
    for (cn, cv, ci), b in zip(clean, (0, 2)):
        assert np.array_equal(n[b].view(np.uint32), cn[0].view(np.uint32)) and np.array_equal(idx[b], ci[0])
        assert np.array_equal(var[b].view(np.uint32), cv[0].view(np.uint32))
    assert idx.min() >= 0 and idx.max() < 70
    out, par = _orient(gpu, x, n, idx)
    assert par.min() >= -1 and par.max() < 70
    for b in (0, 2):
        alone, alone_par = _orient(gpu, x[b:b + 1], n[b:b + 1], idx[b:b + 1])
        assert np.array_equal(out[b].view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(par[b], alone_par[0])
    # a whole cloud of NaN, too few finite points for the lists: still every index in range, and the call returns
    x[1] = np.nan
    n, var, idx = _estimate(gpu, x, 8)
    assert idx.min() >= 0 and idx.max() < 70 and np.array_equal(idx[1], np.tile(np.arange(70)[:, None], (1, 8)))
    out, par = _orient(gpu, x, n, idx)
    assert (par[1] == -1).all()                                    # rows that hold only themselves: no edges, N roots


# ---- (e) determinism and batch independence ----------------------------------------------------------------------------
def test_two_runs_and_any_batch_give_the_same_bits(gpu):
    x = _random_clouds(4, 300, 31)
    first = _estimate(gpu, x, 12)
    again = _estimate(gpu, x, 12)
    alone = _estimate(gpu, x[2:3], 12)
    for a, b, c in zip(first, again, alone):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a[2].view(np.uint32), c[0].view(np.uint32))
    o1, o2, o3 = (_orient(gpu, x, first[0], first[2]), _orient(gpu, x, first[0], first[2]),
                  _orient(gpu, x[2:3], first[0][2:3], first[2][2:3]))
    assert np.array_equal(o1[0].view(np.uint32), o2[0].view(np.uint32)) and np.array_equal(o1[1], o2[1])
    assert np.array_equal(o1[0][2].view(np.uint32), o3[0][0].view(np.uint32)) and np.array_equal(o1[1][2], o3[1][0])


# ---- (f) orientation ---------------------------------------------------------------------------------------------------
def _two_spheres():
    a, na = ref.sphere(400, 41, 0.5)
    b, nb = ref.sphere(400, 42, 0.5, (4.0, 0.0, 0.25))
    return np.concatenate([a, b]), np.concatenate([na, nb])


ORIENT_CASES = {
    "sphere": (lambda: ref.sphere(600, 40), 12, 1),
    "torus": (lambda: ref.torus(1200, 43, 1.0, 0.4), 10, 1),
    "two-spheres": (_two_spheres, 8, 2),
}


@pytest.mark.parametrize("name", sorted(ORIENT_CASES))
def test_orientation_along_the_spanning_forest(gpu, name):
    make, k, n_roots = ORIENT_CASES[name]
    x, outward = make()
    N = len(x)
    n, _, idx = _estimate(gpu, x[None], k)
    out, par = _orient(gpu, x[None], n, idx)
    out, par, n, idx = out[0], par[0], n[0], idx[0]
    adj = ref.adjacency(idx, N)
    roots = np.flatnonzero(par < 0)
    assert len(roots) == n_roots and (out[roots, 2] >= 0).all()
    kids = np.flatnonzero(par >= 0)
    assert all(par[v] in adj[v] for v in kids)
    hops, at = 0, par.copy()                                       # following parents ends at a root within N steps
    while (at >= 0).any():
        at = np.where(at >= 0, par[np.maximum(at, 0)], -1)
        hops += 1
        assert hops <= N
    assert ((out[kids].astype(np.float64) * out[par[kids]].astype(np.float64)).sum(axis=1) >= 0).all()
    assert np.array_equal(np.abs(out).view(np.uint32), np.abs(n).view(np.uint32))
    # the restatement on the kernel's own normals and lists: the multiset of edge weights, and (the rules being
    # deterministic) the forest itself
    want_out, want_par, want_key, _ = ref.forest(x, n, idx, 2)
    got_w = ref.weight32(n[kids], n[par[kids]])
    assert np.array_equal(np.sort(got_w).view(np.uint32), np.sort(want_key[want_par >= 0]).view(np.uint32))
    assert np.array_equal(par, want_par) and np.array_equal(out.view(np.uint32), want_out.view(np.uint32))
    # the signs that come in do not matter
    flips = np.where(np.random.default_rng(5).random(N) < 0.5, np.float32(-1), np.float32(1))[:, None]
    out2, par2 = _orient(gpu, x[None], (n * flips)[None], idx[None])
    assert np.array_equal(out2[0].view(np.uint32), out.view(np.uint32)) and np.array_equal(par2[0], par)
    # every normal looks outward (unoriented, about half do)
    dots = (out.astype(np.float64) * outward).sum(axis=1)
    raw = (n.astype(np.float64) * outward).sum(axis=1)
    print(f"{name}: {len(roots)} roots, wrong {(dots <= 0).sum()} of {N} (unoriented {(raw <= 0).sum()}), "
          f"smallest dot {dots.min():.3f}")
    assert (dots > 0).all() and 0.25 < (raw <= 0).mean() < 0.75


def test_orientation_takes_any_table_and_any_axis(gpu):
    """Entries outside [0, N) or equal to their own row are no edges; y as the up axis."""
    x, outward = ref.sphere(200, 44)
    n, _, idx = _estimate(gpu, x[None], 8)
    table = idx[0].copy()
    table[:, -1] = np.where(np.arange(200) % 3 == 0, -7, np.where(np.arange(200) % 3 == 1, 200, np.arange(200)))
    table[:, 0] = table[:, 1]                                      # a repeated entry
    out, par = _orient(gpu, x[None], n, table[None], axis=1)
    want_out, want_par, _, _ = ref.forest(x, n[0], table, 1)
    assert np.array_equal(par[0], want_par) and np.array_equal(out[0].view(np.uint32), want_out.view(np.uint32))
    root = np.flatnonzero(par[0] < 0)
    assert root.tolist() == [int(np.argmax(x[:, 1]))] and out[0][root[0], 1] >= 0
    assert ((out[0].astype(np.float64) * outward).sum(axis=1) > 0).all()


def test_sizes_that_take_the_other_paths(gpu):
    """More than one LDS tile of candidates (N > 1024) in the selection; the 1024-thread workgroup (N > 4096) and more
    than 64 KB of LDS (N > 8160) in the forest, on a made-up connected table (a ring with chords)."""
    x = _random_clouds(1, 1030, 80)
    _, _, idx = _estimate(gpu, x, 8)
    assert np.array_equal(idx[0], ref.neighbour_lists(x[0], 8))
    N = 8200
    rng = np.random.default_rng(81)
    x = rng.standard_normal((N, 3)).astype(np.float32)
    n = rng.standard_normal((N, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    table = ((np.arange(N)[:, None] + np.array([1, 2, N - 1, N // 2])) % N).astype(np.int32)
    out, par = _orient(gpu, x[None], n[None], table[None])
    want_out, want_par, _, _ = ref.forest(x, n, table, 2)
    assert (want_par < 0).sum() == 1
    assert np.array_equal(par[0], want_par) and np.array_equal(out[0].view(np.uint32), want_out.view(np.uint32))


# ---- (g) host functions ------------------------------------------------------------------------------------------------
def test_estimate_normals_in_each_mode(gpu):
    x, outward = ref.sphere(500, 50)
    pts = torch.from_numpy(x).to(gpu)
    low = _estimate(gpu, x[None], 16)
    none, var, idx = normals.estimate_normals(pts, orient="none", return_variation=True, return_neighbors=True)
    assert none.shape == (500, 3) and var.shape == (500,) and idx.shape == (500, 16) and idx.dtype == torch.int64
    assert np.array_equal(none.cpu().numpy(), low[0][0]) and np.array_equal(var.cpu().numpy(), low[1][0])
    assert np.array_equal(idx.cpu().numpy(), low[2][0])
    mst = normals.estimate_normals(pts)                            # k = 16, orient "mst", up z
    want, _ = _orient(gpu, x[None], low[0], low[2])
    assert np.array_equal(mst.cpu().numpy(), want[0])
    for got in (mst, normals.estimate_normals(pts, orient="outward"), normals.estimate_normals(pts, 8, orient="mst", up="y"),
                normals.estimate_normals(pts, 8, orient="mst", up="x")):
        assert ((got.cpu().numpy().astype(np.float64) * outward).sum(axis=1) > 0).all()
    seen = normals.estimate_normals(pts, orient=torch.tensor([0.0, 0.0, 5.0]))           # a viewpoint on the CPU is fine
    assert (_toward32(seen.cpu().numpy(), x, [0.0, 0.0, 5.0]) >= 0).all()
    batch = torch.from_numpy(np.stack([x, ref.torus(500, 51)[0]])).to(gpu)
    both, bvar = normals.estimate_normals(batch.requires_grad_(), 16, return_variation=True)
    assert both.shape == (2, 500, 3) and bvar.shape == (2, 500) and not both.requires_grad
    assert torch.equal(both[0], mst)
    views = normals.estimate_normals(batch, 16, orient=torch.tensor([[0.0, 0.0, 5.0], [9.0, 0.0, 0.0]], device=gpu))
    assert torch.equal(views[0], seen)


def test_normal_consistency_of_two_clouds(gpu):
    x, nrm = ref.sphere(400, 60)
    p, n = torch.from_numpy(x).to(gpu), torch.from_numpy(nrm.astype(np.float32)).to(gpu)
    own = normals.normal_consistency(p, n, p, -n)
    assert sorted(own) == ["backward", "forward", "normal_consistency"] and all(type(v) is float for v in own.values())
    n64 = n.cpu().numpy().astype(np.float64)
    unit = (n64 * n64).sum(axis=1).mean()
    assert all(abs(v - unit) <= 1e-6 for v in own.values()) and abs(unit - 1) <= 1e-6
    theta = 0.4
    rot = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
    turned = (nrm @ rot.T).astype(np.float32)
    got = normals.normal_consistency(p, n, p, torch.from_numpy(turned).to(gpu))
    want = np.abs((n64 * turned.astype(np.float64)).sum(axis=1)).mean()
    assert all(abs(v - want) <= 1e-6 for v in got.values()) and 0.8 < want < 0.999
    # two different clouds, against brute force in float64
    y, nrm_y = ref.sphere(300, 61)
    q, m = torch.from_numpy(y).to(gpu), torch.from_numpy(nrm_y.astype(np.float32)).to(gpu)
    got = normals.normal_consistency(p, n, q, m)
    d = ((x.astype(np.float64)[:, None] - y.astype(np.float64)[None]) ** 2).sum(-1)
    m64 = nrm_y.astype(np.float32).astype(np.float64)
    fwd = np.abs((n64 * m64[d.argmin(axis=1)]).sum(axis=1)).mean()
    bwd = np.abs((m64 * n64[d.argmin(axis=0)]).sum(axis=1)).mean()
    assert abs(got["forward"] - fwd) <= 1e-6 and abs(got["backward"] - bwd) <= 1e-6
    assert abs(got["normal_consistency"] - 0.5 * (fwd + bwd)) <= 1e-6 and fwd > 0.95
    batched = normals.normal_consistency(p[None], n[None], q[None], m[None])
    assert batched == got


def test_mesh_normal_consistency(gpu):
    v, f = mref.cube()
    d_v, d_f = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    gen = torch.Generator().manual_seed(5)
    cloud, _ = meshes.sample_surface(d_v, d_f, 2000, u=torch.rand((2000, 3), generator=gen))
    u = torch.rand((500, 3), generator=gen)
    got = meshes.mesh_normal_consistency(d_v, d_f, cloud, n_samples=500, u=u)
    assert sorted(got) == ["normal_consistency", "to_cloud", "to_surface"] and all(type(x) is float for x in got.values())
    print(got)
    assert all(0.9 <= x <= 1 + 1e-9 for x in got.values())
    assert meshes.mesh_normal_consistency(d_v, d_f, cloud, n_samples=500, u=u) == got
    # float64 restatement on the same normals, faces by the float64 definition of K32, neighbours by brute force
    p = cloud.cpu().numpy()
    cn = normals.estimate_normals(cloud, 16, orient="none").cpu().numpy().astype(np.float64)
    v64 = v.astype(np.float64)
    g = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    face = pmref.point_mesh(p, v, f, np.float64)[1]
    to_surface = np.abs((cn * g[face]).sum(axis=1)).mean()
    samples, sample_face = meshes.sample_surface(d_v, d_f, 500, u=u)
    s = samples.cpu().numpy().astype(np.float64)
    near = ((s[:, None] - p.astype(np.float64)[None]) ** 2).sum(-1).argmin(axis=1)
    to_cloud = np.abs((g[sample_face.cpu().numpy()] * cn[near]).sum(axis=1)).mean()
    assert abs(got["to_surface"] - to_surface) <= 1e-6 and abs(got["to_cloud"] - to_cloud) <= 1e-6
    assert abs(got["normal_consistency"] - 0.5 * (to_surface + to_cloud)) <= 1e-6
    # the samples at least a quarter of the side away from every edge: planar neighbourhoods, the faces' own normals
    inner = np.sort(np.abs(p), axis=1)[:, 1] <= 0.25               # the two in-face coordinates (the third is 0.5)
    flat = cloud[torch.from_numpy(inner).to(gpu)].contiguous()
    assert 300 < len(flat) < 1000
    away = meshes.mesh_normal_consistency(d_v, d_f, flat, n_samples=500, u=u)
    print(away)
    assert abs(away["to_surface"] - 1) <= 1e-3
    # given normals are used as they are
    given = meshes.mesh_normal_consistency(d_v, d_f, cloud, n_samples=500, u=u, cloud_normals=torch.from_numpy(cn).float().to(gpu))
    assert given == got
    assert sorted(meshes.mesh_accuracy(d_v, d_f, cloud, n_samples=500, u=u)) == ["accuracy", "chamfer", "completeness", "hausdorff"]


# ---- (h) tools -----------------------------------------------------------------------------------------------------------
def test_generate_meshes_with_normal_consistency(gpu, tmp_path):
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
               "--grid", "6", "--max_items", "2", "--model_path", str(tmp_path / "ckpt"), "--name", "0",
               "--eval_model", "model.pt", "--output", str(tmp_path / tag), *extra]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        files = {os.path.relpath(os.path.join(d, n), tmp_path / tag): open(os.path.join(d, n), "rb").read()
                 for d, _, names in os.walk(tmp_path / tag) for n in names}
        return out.stdout.replace(str(tmp_path / tag), ""), files

    stdout, files = run("a", "--metrics", "--normal_consistency", "--normals_k", "12")
    lines = [ln for ln in stdout.split("\n") if ln.startswith("Class: ")]
    print("\n".join(lines))
    report = json.loads(files["metrics.json"])
    assert report["normals_k"] == 12 and len(lines) == len(report["classes"]) >= 1
    for ln in lines:
        row = report["classes"][ln.split(" -- ")[0][len("Class: "):]]
        parts = ln.split(" -- ")[1].split("; ")
        assert [part.split(": ")[0] for part in parts] == ["P2S", "S2P", "Mesh CD", "Mesh HD", "NC"]
        value = float(parts[-1].split(": ")[1])
        assert 0 <= value <= 1 and value == row["normal_consistency"]
        assert sorted(row) == ["accuracy", "chamfer", "completeness", "hausdorff", "items", "normal_consistency"]
    assert stdout.strip().split("\n")[-1].endswith("distances K32 + K26 + K1, normals K33)")
    again, files_b = run("b", "--metrics", "--normal_consistency", "--normals_k", "12")
    assert again == stdout and files_b == files                            # byte for byte, metrics.json included


def test_estimate_normals_tool(gpu, tmp_path):
    x = np.stack([ref.sphere(200, 70)[0], ref.torus(200, 71)[0]])
    np.save(tmp_path / "pair.npy", x)
    np.save(tmp_path / "one.npy", x[0])
    cmd = [sys.executable, os.path.join(ROOT, "estimate_normals.py"), "--input", str(tmp_path / "pair.npy"),
           str(tmp_path / "one.npy"), "--output", str(tmp_path / "out"), "--k", "10"]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("3 clouds, 600 points with normals (k = 10, orient mst, K33)")
    assert sorted(os.listdir(tmp_path / "out")) == ["one.ply", "pair_0.ply", "pair_1.ply"]
    from fpsg_amd.datasets import ply_reader
    for name, cloud in (("pair_0.ply", x[0]), ("pair_1.ply", x[1]), ("one.ply", x[0])):
        rows = np.asarray(ply_reader(str(tmp_path / "out" / name)), np.float32)
        assert rows.shape == (200, 6) and np.array_equal(rows[:, :3].view(np.uint32), cloud.view(np.uint32))
        assert np.abs((rows[:, 3:].astype(np.float64) ** 2).sum(axis=1) - 1).max() <= 8 * U
    want = normals.estimate_normals(torch.from_numpy(x[0]).to(gpu), 10).cpu().numpy()
    assert np.array_equal(np.asarray(ply_reader(str(tmp_path / "out" / "one.ply")), np.float32)[:, 3:], want)
