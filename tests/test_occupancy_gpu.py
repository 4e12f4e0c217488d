"""K15 on the GPU: the occupancy grid equals its numpy restatement integer for integer (through the C ABI and through
the Python mirror), its nodes are the nearest retained ones in float64, it is deterministic and additive, and the
Jensen-Shannon divergence built on it behaves as defined, up to ``evaluate_Network.py --jsd``."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _occupancy_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _c_abi(dev, x: np.ndarray, r, E, sph):
    """One call of fpsg_occupancy_grid on zeroed outputs: cells, counts, clouds_hit, outside as numpy."""
    from fpsg_amd import _hip
    lib = _hip.load()
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    S, N, _ = t.shape
    counts = torch.zeros(r ** 3, dtype=torch.int32, device=dev)
    hit = torch.zeros(r ** 3, dtype=torch.int32, device=dev)
    outside = torch.zeros(3, dtype=torch.int32, device=dev)
    cells = torch.full((S, N), -7, dtype=torch.int32, device=dev)
    assert lib.fpsg_occupancy_grid_workspace_bytes(S, N, r) == 0
    with torch.cuda.device(dev):
        rc = lib.fpsg_occupancy_grid(t.data_ptr(), S, N, r, float(E), int(sph), counts.data_ptr(), hit.data_ptr(),
                                     outside.data_ptr(), cells.data_ptr(), None, 0, _hip.stream_of(t))
    _hip.check(rc, "fpsg_occupancy_grid")
    torch.cuda.synchronize(dev)
    return cells.cpu().numpy(), counts.cpu().numpy(), hit.cpu().numpy(), outside.cpu().numpy()


def _check_case(dev, x, r, E=1.0, sph=True, what=""):
    from fpsg_amd.metrics import occupancy_grid
    want = ref.grid(x, r, E, sph)
    cells, counts, hit, outside = _c_abi(dev, x, r, E, sph)
    tag = f"{what} r={r} E={E} in_sphere={sph} shape={x.shape}"
    bad = np.nonzero(cells != want["cells"])
    assert bad[0].size == 0, (tag, "cells differ at", bad[0][:5], bad[1][:5], cells[bad][:5], want["cells"][bad][:5],
                              x[bad][:5])
    assert np.array_equal(counts, want["counts"]), tag
    assert np.array_equal(hit, want["clouds_hit"]), tag
    assert np.array_equal(outside, want["outside"]), (tag, outside, want["outside"])
    g = occupancy_grid(torch.from_numpy(x).to(dev), r, E, sph, return_cells=True)       # the mirror, same integers
    assert g["counts"].dtype == torch.int32 and tuple(g["counts"].shape) == (r, r, r) and g["counts"].device.type == "cuda"
    assert np.array_equal(g["cells"].cpu().numpy(), want["cells"]), tag
    assert np.array_equal(g["counts"].cpu().numpy().ravel(), want["counts"]), tag
    assert np.array_equal(g["clouds_hit"].cpu().numpy().ravel(), want["clouds_hit"]), tag
    assert g["outside"].tolist() == want["outside"].tolist(), tag
    assert g["n_clouds"] == x.shape[0] and g["n_points"] == x.shape[0] * x.shape[1]
    return want


# ---- 7. integer for integer --------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,N", [(1, 1), (1, 5000), (37, 2048), (300, 100), (37, 100)])
def test_ball_and_tanh_clouds_equal_the_restatement(gpu, S, N):
    rng = np.random.default_rng(1000 * S + N)
    w = _check_case(gpu, ref.ball_clouds(rng, S, N), 28, what="ball")
    assert w["counts"].sum() == S * N
    _check_case(gpu, ref.tanh_clouds(rng, S, N), 28, what="tanh")
    _check_case(gpu, ref.ball_clouds(rng, S, N) * np.float32(1.5), 28, what="1.5 E")


@pytest.mark.parametrize("r", [3, 5, 27, 28, 29, 64])
@pytest.mark.parametrize("sph", [True, False])
def test_every_resolution_with_and_without_the_sphere(gpu, r, sph):
    rng = np.random.default_rng(r + 100 * sph)
    S, N = (3, 400) if r == 64 else (5, 600)
    for E in (1.0, 0.5, 2.0):
        x = np.concatenate([ref.ball_clouds(rng, S, N), ref.tanh_clouds(rng, S, N),
                            ref.ball_clouds(rng, S, N) * np.float32(1.5)]) * np.float32(E)
        w = _check_case(gpu, x, r, E, sph, what="mixed")
        if E == 1.0 and sph:
            assert w["outside"][0] > 0 and w["outside"][1] > w["outside"][0]
    x = np.tile(ref.tanh_clouds(rng, 1, 1), (2, 2048, 1))           # clouds of one repeated point
    w = _check_case(gpu, x, r, 1.0, sph, what="repeated point")
    assert w["counts"].max() == 2 * 2048 and w["clouds_hit"].max() == 2 and (w["counts"] > 0).sum() == 1


def _lattice(r):
    """Points whose index coordinates are exact: with E = (r-1)/2 the scale is 1 and t = p + (r-1)/2.  Every
    combination over the three axes of nodes and half-way values next to the grid's ends, its centre and the
    sphere's surface on an axis line: half-way on one, two and three axes, both sides of retained / dropped node
    pairs, and +-E."""
    E = (r - 1) / 2.0
    m = (r - 1) // 2
    vals = sorted({v for v in [0, 0.5, 1, 1.5, 2, 2.5, m - 0.5, m, m + 0.5, m + 1, m + 1.5, r - 3.5, r - 3, r - 2.5,
                               r - 2, r - 1.5, r - 1] if 0 <= v <= r - 1})
    t = np.array([(a, b, c) for a in vals for b in vals for c in vals], dtype=np.float64)
    p = (t - E).astype(np.float32)
    assert np.array_equal(ref.index_coords(p, r, E).astype(np.float64), t)     # exact: no rounding anywhere
    return p[None], E, t


@pytest.mark.parametrize("r", [3, 5, 27, 28, 29, 64])
def test_half_way_points_round_half_to_even(gpu, r):
    x, E, t = _lattice(r)
    half = (t % 1 == 0.5).sum(axis=1)
    assert {1, 2, 3} <= set(half.tolist()) and (np.abs(x) == np.float32(E)).any()
    w = _check_case(gpu, x, r, E, True, what="lattice")
    keep = ref.retained(r)
    n0 = np.clip(np.rint(t), 0, r - 1).astype(int)
    dropped = ~keep[n0[:, 0], n0[:, 1], n0[:, 2]]
    assert dropped.any() and (~dropped).any()                      # both sides of the sphere's surface
    direct = (n0[:, 0] * r + n0[:, 1]) * r + n0[:, 2]
    assert np.array_equal(w["cells"][0][~dropped], direct[~dropped])            # half to even where retained
    _check_case(gpu, x, r, E, False, what="lattice")
    # the same lattice pushed slightly off the ties, both ways
    for eps in (np.float32(1e-4), np.float32(-1e-4)):
        _check_case(gpu, x + eps, r, E, True, what="lattice off the ties")


def test_non_finite_and_far_points(gpu):
    rng = np.random.default_rng(3)
    x = ref.ball_clouds(rng, 4, 300)
    x[0, 5, 1] = np.nan
    x[1, 7] = (np.inf, 0.0, 0.0)
    x[1, 8] = (0.1, -np.inf, np.nan)
    x[2, 0] = (30.0, -30.0, 30.0)                                  # beyond the windowed search: every node is scanned
    x[2, 1] = (1e30, 0.0, 0.0)
    x[2, 2] = (3e38, 3e38, -3e38)                                  # t overflows: every d is infinite, the lowest index
    x[3, 3] = (-19.0, 0.01, 0.02)
    x[3, 4] = (18.9, 18.9, 18.9)
    for r in (28, 5):
        w = _check_case(gpu, x, r, 1.0, True, what="odd points")
        assert w["outside"][2] == 3 and (w["cells"] == -1).sum() == 3
        assert w["counts"].sum() + w["outside"][2] == 4 * 300
        _check_case(gpu, x, r, 1.0, False, what="odd points")


# ---- 8. nearest in float64 ---------------------------------------------------------------------------------------

def _min_dist64(t64, nodes):
    try:
        from scipy.spatial import cKDTree
        return cKDTree(nodes).query(t64, k=1)[0]
    except ImportError:
        out = np.empty(len(t64))
        for k in range(0, len(t64), 256):
            out[k:k + 256] = np.sqrt(((t64[k:k + 256, None, :] - nodes[None]) ** 2).sum(-1).min(axis=1))
        return out


@pytest.mark.parametrize("kind", ["ball", "tanh"])
def test_cells_are_the_nearest_retained_nodes_in_float64(gpu, kind):
    """Independent of the fp32 rounding rules: the float64 distance (index units, from the float64 image of the point)
    to the kernel's node exceeds the float64 minimum over the retained nodes by at most 2 delta (|dx| + |dy| + |dz|) +
    1e-6 d, delta = 2^-18 (two fp32 half-ulp roundings of a t below 64, and the fp32 sum), dx.. and d the offsets and
    the distance to the kernel's node.  Every point is checked."""
    r, E = 28, 1.0
    rng = np.random.default_rng(8)
    x = (ref.ball_clouds if kind == "ball" else ref.tanh_clouds)(rng, 16, 2048)
    cells = _c_abi(gpu, x, r, E, True)[0].reshape(-1)
    assert (cells >= 0).all()
    node = np.stack([cells // (r * r), (cells // r) % r, cells % r], axis=1).astype(np.float64)
    keep = ref.retained(r)
    assert keep[tuple(node.astype(int).T)].all()
    t64 = x.reshape(-1, 3).astype(np.float64) * ((r - 1) / (2 * E)) + (r - 1) / 2
    off = np.abs(t64 - node)
    dist = np.sqrt((off ** 2).sum(axis=1))
    best = _min_dist64(t64, np.argwhere(keep).astype(np.float64))
    excess = dist - best
    bound = 2 * 2.0 ** -18 * off.sum(axis=1) + 1e-6 * dist
    print(f"{kind}: max excess {excess.max():.3e}, points not at the float64 minimum {(excess > 1e-12).sum()} of "
          f"{len(dist)}, max excess / bound {np.max(excess / np.maximum(bound, 1e-300)):.3f}")
    assert (excess >= -1e-9).all()
    assert (excess <= bound).all(), (excess.max(), int((excess > bound).sum()))


# ---- 9. determinism and additivity -------------------------------------------------------------------------------

def test_deterministic_additive_and_scale_invariant(gpu):
    from fpsg_amd.metrics import occupancy_grid
    from fpsg_amd.set_metrics import retained_nodes
    rng = np.random.default_rng(9)
    S, N = 37, 2048
    x = torch.from_numpy(np.concatenate([ref.ball_clouds(rng, 20, N), ref.tanh_clouds(rng, 17, N)])).to(gpu)
    x[3, 11, 0] = float("nan")
    a = occupancy_grid(x, return_cells=True)
    b = occupancy_grid(x, return_cells=True)
    for k in ("counts", "clouds_hit", "outside", "cells"):
        assert torch.equal(a[k], b[k]), k
    for cuts in ((0, 1, 37), (0, 10, 20, 37), (0, 36, 37), tuple(range(38))):
        acc = None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            acc = occupancy_grid(x[lo:hi].contiguous(), out=acc)
        assert acc["n_clouds"] == S and acc["n_points"] == S * N and "cells" not in acc
        for k in ("counts", "clouds_hit", "outside"):
            assert torch.equal(acc[k], a[k]), (k, cuts)
    h = occupancy_grid((x * 0.5).contiguous(), half_extent=0.5, return_cells=True)      # scaling by 0.5 is exact
    for k in ("counts", "clouds_hit", "outside", "cells"):
        assert torch.equal(h[k], a[k]), k
    counts, hit = a["counts"].long(), a["clouds_hit"].long()
    assert int(counts.sum()) + int(a["outside"][2]) == S * N and int(a["outside"][2]) == 1
    assert bool((hit <= torch.minimum(counts, torch.full_like(counts, S))).all())
    assert torch.equal(hit > 0, counts > 0)
    keep = retained_nodes(28).to(gpu)
    assert int(counts[~keep].sum()) == 0 and int(hit[~keep].sum()) == 0
    with pytest.raises(ValueError):
        occupancy_grid(x, resolution=27, out=a)


# ---- 10. the divergence ------------------------------------------------------------------------------------------

def test_jsd_of_sets(gpu):
    from fpsg_amd.set_metrics import jsd, jsd_from_counts
    rng = np.random.default_rng(10)
    r, E = 28, 1.0
    gen, rf = ref.tanh_clouds(rng, 12, 1024) * np.float32(0.8), ref.ball_clouds(rng, 20, 2048)
    got = jsd(torch.from_numpy(gen).to(gpu), torch.from_numpy(rf).to(gpu))
    wg, wr = ref.grid(gen, r, E), ref.grid(rf, r, E)
    want = jsd_from_counts(torch.from_numpy(wg["counts"]), torch.from_numpy(wr["counts"]))
    assert abs(got["jsd"] - want) <= 1e-12 and abs(got["jsd"] - ref.jsd(wg["counts"], wr["counts"])) <= 1e-12
    assert 0.0 < got["jsd"] < 1.0
    assert got["outside_gen"] == wg["outside"].tolist() and got["outside_ref"] == wr["outside"].tolist()
    keep = ref.retained(r).ravel()
    for key, w, n in (("entropy_gen", wg, 12), ("entropy_ref", wr, 20)):
        p = w["clouds_hit"][keep] / n
        hb = -(np.where(p > 0, p * np.log2(np.maximum(p, 1e-300)), 0) +
               np.where(p < 1, (1 - p) * np.log2(np.maximum(1 - p, 1e-300)), 0))
        assert abs(got[key] - hb.mean()) <= 1e-12, key
    x = torch.from_numpy(rf).to(gpu)
    assert jsd(x, x)["jsd"] == 0.0
    # opposite half-spaces, each at least one cell width from the dividing plane: disjoint supports
    cell = 2 * E / (r - 1)
    left, right = rf.copy(), rf.copy()
    left[..., 0] = -np.abs(left[..., 0]) * np.float32(0.8) - np.float32(1.01 * cell)
    right[..., 0] = np.abs(right[..., 0]) * np.float32(0.8) + np.float32(1.01 * cell)
    assert left[..., 0].max() <= -cell and right[..., 0].min() >= cell
    v = jsd(torch.from_numpy(left).to(gpu), torch.from_numpy(right).to(gpu))["jsd"]
    assert abs(v - 1.0) <= 1e-12, v
    # a shift of the whole set is seen; a small jitter much less
    shifted = rf + np.array([0.2 * E, 0, 0], dtype=np.float32)
    jitter = rf + (rng.standard_normal(rf.shape) * 0.01 * E).astype(np.float32)
    v_shift = jsd(x, torch.from_numpy(shifted).to(gpu))["jsd"]
    v_jit = jsd(x, torch.from_numpy(jitter).to(gpu))["jsd"]
    assert v_shift > v_jit >= 0.0, (v_shift, v_jit)


# ---- 11. the entry point -----------------------------------------------------------------------------------------

def _evaluate(tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "evaluate_Network.py", "--synthetic", "--n_shot", "2", "--n_query", "1",
                        "--sequential_eval", "--model_path", str(tmp_path), "--name", "x"] + extra,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("Class: ")]


def test_entry_point_flag(gpu, tmp_path):
    lines = _evaluate(tmp_path, ["--jsd"])
    plain = _evaluate(tmp_path, [])
    assert lines and len(lines) == len(plain)
    for ln, pl in zip(lines, plain):
        head, sep, v = ln.rpartition("; JSD: ")
        assert sep and 0.0 <= float(v) <= 1.0 and math.isfinite(float(v)), ln
        assert "JSD" not in pl and "JSD" not in head
        assert head.split(" -- ")[0] == pl.split(" -- ")[0]
        assert [f.split(": ")[0] for f in head.split("; ")] == [f.split(": ")[0] for f in pl.split("; ")]
        for f in pl.split(" -- ")[1].split("; "):                   # today's line: the two reference metrics, no more
            assert f.split(": ")[0] in ("Rec CD", "Rec EMD") and math.isfinite(float(f.split(": ")[1])), pl
    both = _evaluate(tmp_path, ["--set_metrics", "--jsd"])
    assert len(both) == len(plain)
    for ln in both:                                                # (the weights are drawn anew in every run)
        head, sep, v = ln.rpartition("; JSD: ")
        assert sep and "; MMD-CD: " in head and "; COV-CD: " in head and "; 1-NNA-CD: " in head, ln
        assert 0.0 <= float(v) <= 1.0


def test_entry_point_value_is_the_jsd_of_the_returned_clouds(gpu, tmp_path, monkeypatch):
    import evaluate_Network
    from fpsg_amd import cli
    from fpsg_amd.engine import EvalItem
    from fpsg_amd.set_metrics import jsd
    seen = {}
    inner = EvalItem.__call__

    def spy(self, sample):
        out = inner(self, sample)
        assert self.return_clouds
        seen.setdefault(sample["class"][0], []).append((out["syn_pc"].clone(), out["ref_pc_q"].clone()))
        return out

    monkeypatch.setattr(EvalItem, "__call__", spy)
    argv = ["--synthetic", "--n_shot", "2", "--n_query", "2", "--sequential_eval", "--model_path", str(tmp_path),
            "--name", "x"]
    parser = cli.few_shot_parser(evaluation=True)
    torch.manual_seed(0)
    res = evaluate_Network.main(parser.parse_args(argv + ["--jsd"]))
    assert len(res) == 3 and set(res[2]) == set(res[0]) == set(seen)
    for name, m in res[2].items():
        gen = torch.cat([g for g, _ in seen[name]]).contiguous()
        rf = torch.cat([q for _, q in seen[name]]).contiguous()
        assert m == jsd(gen, rf), name
        assert 0.0 <= m["jsd"] <= 1.0
    monkeypatch.setattr(EvalItem, "__call__", inner)
    torch.manual_seed(0)
    assert len(evaluate_Network.main(parser.parse_args(argv))) == 2   # without the flag: today's return value
