"""K33 without a GPU: the numpy restatement (tests/_point_normals_ref.py) on hand-made cases, the argument checks of the
entries and the host functions, the PLY with normals, and the tools' options."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import _point_normals_ref as ref


def test_the_emulated_fma_rounds_once():
    """(1 + 2^-12)^2 + 2^-60 lies just above the midpoint of two fp32 numbers: a float64 sum loses the 2^-60 and then
    rounds the tie to even (down); one rounding of the exact value goes up."""
    a = np.array([1 + 2.0 ** -12], np.float32)
    c = np.array([2.0 ** -60], np.float32)
    assert ref.fma32(a, a, c)[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert np.float32(a.astype(np.float64)[0] ** 2 + 2.0 ** -60) == np.float32(1 + 2.0 ** -11)      # the naive route
    assert ref.fma32(a, a, -c)[0] == np.float32(1 + 2.0 ** -11)
    rng = np.random.default_rng(0)
    x, y, z = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    exact = x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)
    assert np.abs(ref.fma32(x, y, z).astype(np.float64) - exact).max() <= ref.U * np.abs(exact).max()


def test_planar_grid_ties_follow_the_index_and_the_normal_is_z():
    x = ref.planar_grid(5)
    idx = ref.neighbour_lists(x, 5)
    # corner 0 at (0, 0): (0, 1/4) is index 1 and (1/4, 0) index 5, both at d2 = 1/16; the diagonal 6; then 2 and 10
    assert idx[0].tolist() == [1, 5, 6, 2, 10]
    # the centre 12: its four edge neighbours in index order, then the first diagonal
    assert idx[12].tolist() == [7, 11, 13, 17, 6]
    # every list is the full lexicographic sort on exact distances
    d2 = ((x[None].astype(np.float64) - x[:, None].astype(np.float64)) ** 2).sum(-1)
    for i in range(25):
        order = sorted((j for j in range(25) if j != i), key=lambda j: (d2[i, j], j))
        assert idx[i].tolist() == order[:5]
    n, lam, _ = ref.pca64(x, idx)
    assert np.allclose(np.abs(n), [0, 0, 1]) and np.allclose(lam[:, 0], 0) and (lam[:, 1] > 0.01).all()


def test_duplicates_are_neighbours_at_distance_zero_and_the_lower_index_wins():
    p = np.random.default_rng(1).standard_normal((6, 3)).astype(np.float32)
    x = np.concatenate([p, p])
    idx = ref.neighbour_lists(x, 3)
    assert idx[:6, 0].tolist() == list(range(6, 12)) and idx[6:, 0].tolist() == list(range(6))
    d2 = ref.sq_dist32(x)
    assert d2.dtype == np.float32 and np.array_equal(d2, d2.T) and (np.diag(d2) == 0).all()
    for i in range(12):                                            # a point and its copy tie: the lower index first
        row = idx[i, 1:].tolist()
        if row[0] % 6 == row[1] % 6:
            assert row[0] < row[1]


def test_a_line_of_points_is_rank_one():
    t = np.arange(12, dtype=np.float64)[:, None]
    x = (t * np.array([1.0, 2.0, -2.0])).astype(np.float32)         # integers: exactly collinear
    idx = ref.neighbour_lists(x, 4)
    assert idx[0].tolist() == [1, 2, 3, 4] and idx[5].tolist() == [4, 6, 3, 7]
    n, lam, vec = ref.pca64(x, idx)
    assert np.abs(lam[:, :2]).max() <= 1e-12 * lam[:, 2].min() and (lam[:, 2] > 1).all()
    assert np.allclose(np.abs(vec[:, :, 2] @ (np.array([1.0, 2.0, -2.0]) / 3)), 1)
    assert np.abs(n @ np.array([1.0, 2.0, -2.0])).max() <= 1e-9


def test_two_far_clusters_give_two_roots_at_their_topmost_points():
    a, na = ref.sphere(40, 2)
    b, nb = ref.sphere(30, 3, offset=(10.0, 0.0, 0.5))
    x = np.concatenate([a, b])
    idx = ref.neighbour_lists(x, 4)
    flips = np.where(np.random.default_rng(4).random(70) < 0.5, -1.0, 1.0)[:, None]
    normals = (np.concatenate([na, nb]) * flips).astype(np.float32)
    out, par, key, order = ref.forest(x, normals, idx, 2)
    roots = np.flatnonzero(par < 0)
    assert len(roots) == 2 and sorted(order.tolist()) == list(range(70))
    top_b, top_a = 40 + int(np.argmax(b[:, 2])), int(np.argmax(a[:, 2]))
    assert order[0] == top_b and set(roots) == {top_a, top_b}      # the higher cluster first
    assert (out[roots, 2] >= 0).all() and np.isnan(key[roots]).all()
    adj = ref.adjacency(idx, 70)
    for v in range(70):
        if par[v] >= 0:
            assert par[v] in adj[v] and (par[v] < 40) == (v < 40)
            assert key[v] == ref.weight32(normals[v], normals[par[v]])
            assert float(out[v].astype(np.float64) @ out[par[v]].astype(np.float64)) >= 0
    assert np.array_equal(np.abs(out), np.abs(normals))
    # the input's signs do not matter
    out2, par2, key2, _ = ref.forest(x, -normals, idx, 2)
    assert np.array_equal(out2, out) and np.array_equal(par2, par) and np.array_equal(key2, key, equal_nan=True)
    # entries out of range or equal to their own row are no edges
    bad = idx.copy()
    bad[:, -1] = np.where(np.arange(70) % 3 == 0, -1, np.where(np.arange(70) % 3 == 1, 70, np.arange(70)))
    adj = ref.adjacency(bad, 70)
    assert all(((a >= 0) & (a < 70)).all() and v not in a for v, a in enumerate(adj))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "fpsg_amd", "libfpsg_hip.so")):
        g.build()
    from fpsg_amd import _hip
    return _hip.load()


def test_entries_refuse_bad_arguments_before_any_hip_call(lib):
    from fpsg_amd import _hip
    for name in ("fpsg_point_normals", "fpsg_point_normals_orient"):
        assert name in _hip.SIGNATURES and name + "_workspace_bytes" in _hip.SIGNATURES
        assert getattr(lib, name + "_workspace_bytes").restype is ctypes.c_size_t
    assert lib.fpsg_point_normals_workspace_bytes(2, 100, 16) == 2 * 100 * 16 * 4
    assert lib.fpsg_point_normals_orient_workspace_bytes(2, 100, 16) == 2 * 100 * 18 * 4
    for bad in ((0, 100, 16), (1, 100, 2), (1, 100, 33), (1, 16, 16), (1, 16385, 16), (65536, 100, 16)):
        assert lib.fpsg_point_normals_workspace_bytes(*bad) == 0 and lib.fpsg_point_normals_orient_workspace_bytes(*bad) == 0
    fake = ctypes.c_void_p(4096)                                   # never dereferenced: every call stops on the host
    odd = ctypes.c_void_p(4098)

    def estimate(B=1, N=100, k=16, mode=0, xyz=fake, ref_=None, normals=fake, var=None, idx=None, ws=fake, ws_bytes=1 << 20):
        return lib.fpsg_point_normals(xyz, B, N, k, mode, ref_, normals, var, idx, ws, ws_bytes, None)

    def orient(B=1, N=100, k=16, axis=2, xyz=fake, nin=fake, idx=fake, out=fake, parent=None, ws=fake, ws_bytes=1 << 20):
        return lib.fpsg_point_normals_orient(xyz, nin, idx, B, N, k, axis, out, parent, ws, ws_bytes, None)

    for call in (estimate, orient):
        for kw, text in ((dict(B=0), b"B must be positive"), (dict(k=2), b"k must be in 3..32"), (dict(k=33), b"3..32"),
                         (dict(N=16), b"at least k + 1"), (dict(ws_bytes=100), b"workspace")):
            assert call(**kw) == -2 and text in lib.fpsg_last_error(), (call.__name__, kw, lib.fpsg_last_error())
        assert call(N=16385) == -4 and b"16384" in lib.fpsg_last_error()
        assert call(N=16385, xyz=None) == -4                        # shape and limit checks come first
        assert call(k=2, xyz=None) == -2
        assert call(xyz=None) == -1 and call(ws=None) == -1 and b"null pointer" in lib.fpsg_last_error()
        assert call(xyz=odd) == -3 and call(ws=odd) == -3
    assert estimate(mode=3) == -2 and estimate(mode=-1) == -2 and b"sign_mode" in lib.fpsg_last_error()
    assert estimate(mode=1) == -1 and estimate(mode=2) == -1 and estimate(normals=None) == -1
    assert estimate(var=odd) == -3 and estimate(idx=odd) == -3 and estimate(mode=1, ref_=odd) == -3
    assert orient(axis=3) == -2 and orient(axis=-1) == -2 and b"axis" in lib.fpsg_last_error()
    assert orient(nin=None) == -1 and orient(idx=None) == -1 and orient(out=None) == -1 and orient(parent=odd) == -3
    assert lib.fpsg_version() == 1


def test_host_functions_refuse_bad_inputs_without_a_gpu():
    import torch

    from fpsg_amd import meshes, normals
    from fpsg_amd._hip import FpsgHipError
    cloud = torch.rand(40, 3)
    for kw, text in ((dict(k=2), "3 to 32"), (dict(k=33), "3 to 32"), (dict(k=3.5), "3 to 32"), (dict(k=True), "3 to 32"),
                     (dict(orient="poisson"), "mst, outward, none"), (dict(up="w"), "x, y, z"),
                     (dict(orient=torch.zeros(2, 3)), "(3,) or (1, 3)")):
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
            normals.estimate_normals(cloud, **kw)
    with pytest.raises(ValueError, match="k \\+ 1 = 17 to 16384"):
        normals.estimate_normals(torch.rand(16, 3))
    with pytest.raises(ValueError, match="to 16384 points"):
        normals.estimate_normals(torch.rand(1, 16385, 3), 8)
    with pytest.raises(ValueError, match=r"\[N,3\] or \[B,N,3\]"):
        normals.estimate_normals(torch.rand(40, 2))
    with pytest.raises(ValueError, match="float32"):
        normals.estimate_normals(cloud.double())
    for orient in ("mst", "outward", "none", torch.zeros(3)):       # nothing wrong but the device: no CPU fallback
        with pytest.raises(FpsgHipError, match="no CPU fallback"):
            normals.estimate_normals(cloud, 8, orient=orient)
    with pytest.raises(ValueError, match="points' shape"):
        normals.normal_consistency(cloud, cloud[:10], cloud, cloud)
    with pytest.raises(ValueError, match="float32"):
        normals.normal_consistency(cloud, cloud, cloud.double(), cloud.double())
    with pytest.raises(FpsgHipError):
        normals.normal_consistency(cloud, cloud, cloud, cloud)
    verts, faces = torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]])
    with pytest.raises(ValueError, match=r"\[N,3\] cloud"):
        meshes.mesh_normal_consistency(verts, faces, torch.rand(2, 40, 3))
    with pytest.raises(ValueError, match="n_samples"):
        meshes.mesh_normal_consistency(verts, faces, cloud, n_samples=0)
    with pytest.raises(ValueError, match="cloud's shape"):
        meshes.mesh_normal_consistency(verts, faces, cloud, cloud_normals=cloud[:5])
    with pytest.raises(ValueError, match="3 to 32"):
        meshes.mesh_normal_consistency(verts, faces, cloud, k=40)
    assert sorted(meshes.mesh_accuracy.__kwdefaults__) == ["generator", "n_samples", "u"]     # untouched


def test_ply_with_normals_reads_back_and_the_plain_file_keeps_its_bytes(tmp_path):
    from fpsg_amd import meshes
    from fpsg_amd.datasets import ply_reader
    sys.path.insert(0, ROOT)
    from render_clouds import read_clouds
    rng = np.random.default_rng(5)
    p = rng.standard_normal((7, 3)).astype(np.float32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    meshes.write_ply_points(str(tmp_path / "plain.ply"), p)
    want = ("ply\nformat ascii 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\nend_header\n" +
            "".join("%.9g %.9g %.9g\n" % tuple(r) for r in p.tolist()))
    assert open(tmp_path / "plain.ply").read() == want
    meshes.write_ply_points(str(tmp_path / "with.ply"), p, n)
    text = open(tmp_path / "with.ply").read()
    assert "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n" in text
    rows = np.asarray(ply_reader(str(tmp_path / "with.ply")), np.float32)
    assert rows.shape == (7, 6) and np.array_equal(rows[:, :3], p) and np.array_equal(rows[:, 3:], n)
    assert np.array_equal(read_clouds(str(tmp_path / "with.ply")), p[None])                  # the first three columns
    with pytest.raises(ValueError, match="normals"):
        meshes.write_ply_points(str(tmp_path / "bad.ply"), p, n[:3])


def _tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, name), *args], capture_output=True, text=True, cwd=ROOT,
                          timeout=120)


def test_generate_meshes_lists_and_checks_the_normal_options():
    out = _tool("generate_meshes.py", "--help")
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stdout.replace("\n", " ")
    assert "--normal_consistency" in text and "--normals_k K" in text and "[default: 16]" in text
    assert text.index("meshes:") < text.index("--normal_consistency ", text.index("meshes:"))                      # the tool's own group
    for args, words in ((("--normal_consistency",), ("--normal_consistency", "--metrics")),
                        (("--metrics", "--normals_k", "8"), ("--normals_k", "--normal_consistency")),
                        (("--normals_k", "8"), ("--normals_k", "--metrics")),
                        (("--metrics", "--normal_consistency", "--normals_k", "2"), ("--normals_k", "3 to 32")),
                        (("--metrics", "--normal_consistency", "--normals_k", "33"), ("--normals_k", "3 to 32"))):
        out = _tool("generate_meshes.py", "--synthetic", *args)
        assert out.returncode != 0 and all(w in out.stderr for w in words) and "Traceback" not in out.stderr, (args, out.stderr)


def test_estimate_normals_tool_lists_and_checks_its_options(tmp_path):
    out = _tool("estimate_normals.py", "--help")
    assert out.returncode == 0, out.stderr[-2000:]
    for word in ("--input", "--output", "--k", "--orient", "{mst,outward,none}", "--up", "{z,y}"):
        assert word in out.stdout, word
    np.save(tmp_path / "few.npy", np.zeros((5, 3), np.float32))
    for args, word in ((("--k", "2"), "--k"), (("--k", "33"), "--k"), (("--k", "8"), "too few")):
        out = _tool("estimate_normals.py", "--input", str(tmp_path / "few.npy"), "--output", str(tmp_path / "o"), *args)
        assert out.returncode != 0 and word in out.stderr and "Traceback" not in out.stderr, (args, out.stderr)
    out = _tool("estimate_normals.py", "--input", str(tmp_path / "none.txt"), "--output", str(tmp_path / "o"))
    assert out.returncode != 0 and "Traceback" not in out.stderr and ".npy or .ply" in out.stderr
    assert not os.path.exists(tmp_path / "o")
