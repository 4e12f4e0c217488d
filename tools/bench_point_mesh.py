"""K32 (the nearest triangle of every point) alone, by device events, at two shapes:
  the tool's: B = 5 meshes of F = 7200 faces (16 patches, 16 x 16 grid) with N = 2048 points each;
  a dataset-sized mesh: B = 1, N = 15000 points against F = 100000 faces;
each with chunks = 1 and with the library's choice, alternating over --rounds rounds.  Reports microseconds per call,
pairs per second and the share of the fp32 VALU rate by counted operations (112 per pair: the definition's differences,
products, sums, clamps, comparisons and selects, none of them fused).  With --tool also the wall time of one
generate_meshes.py run with and without --metrics.  Appends its figures to profiles/k32/notes.md.

    python tools/bench_point_mesh.py [--rounds 5] [--iters 50] [--chunks 1 0 16 64] [--tool]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from fpsg_amd import _hip, cli, surface

NOTES = os.path.join(ROOT, "profiles", "k32", "notes.md")
OPS_PER_PAIR = 112
VALU_RATE = 157.3e12 / 2        # fp32 operations per second without fma: half the MI355X's vector peak (spec)


def bumpy_sphere(B, g=16, n_patches=16, seed=0):
    """B meshes on the decoder's topology: a sphere of radius 0.7 tiled by the patches, jittered per mesh."""
    rng = np.random.default_rng(seed)
    uv = surface.regular_grid(g).astype(np.float64)
    rows = []
    for k in range(n_patches):
        lon = (k % 4 + uv[0]) * (np.pi / 2)
        lat = ((k // 4 + uv[1]) / 4 - 0.5) * np.pi * 0.98
        r = 0.7 + 0.03 * np.sin(5 * lon) * np.cos(4 * lat)
        rows.append(np.stack([r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat)], axis=1))
    v = np.concatenate(rows)
    v = v[None] + rng.normal(scale=0.002, size=(B,) + v.shape)
    return v.astype(np.float32), surface.patch_faces(g, n_patches)


def random_mesh(F, seed=1):
    """F small triangles scattered over the unit ball's shell: a dataset mesh's face count without its file."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(F, 3))
    c = 0.5 * c / np.linalg.norm(c, axis=1, keepdims=True)
    tri = c[:, None, :] + rng.normal(scale=0.01, size=(F, 3, 3))
    return tri.reshape(-1, 3).astype(np.float32), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def kernel(a, out):
    dev = torch.device("cuda:0")
    lib = _hip.load()
    g = torch.Generator().manual_seed(0)
    tool_v, tool_f = bumpy_sphere(5)
    data_v, data_f = random_mesh(100000)
    shapes = {"tool: B = 5, N = 2048, F = 7200": (torch.rand((5, 2048, 3), generator=g) * 1.6 - 0.8, tool_v, tool_f),
              "dataset: B = 1, N = 15000, F = 100000": (torch.rand((1, 15000, 3), generator=g) - 0.5, data_v[None], data_f)}
    out.append("| shape | chunks | median | min | max | pairs / s | of the fp32 VALU rate |")
    out.append("|---|---|---|---|---|---|---|")
    for name, (points, verts, faces) in shapes.items():
        B, N = points.shape[:2]
        V, F = verts.shape[-2], len(faces)
        d_p, d_v, d_f = points.to(dev), torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
        dist2 = torch.empty((B, N), dtype=torch.float32, device=dev)
        face = torch.empty((B, N), dtype=torch.int32, device=dev)
        stream = _hip.stream_of(d_p)
        forms, results = {}, {}
        for chunks in a.chunks:
            ws_bytes = lib.fpsg_point_mesh_workspace_bytes(B, N, F, chunks)
            ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)

            def entry(chunks=chunks, ws=ws, ws_bytes=ws_bytes):   # the entry itself: the wrapper's allocations would pace it
                _hip.check(lib.fpsg_point_mesh_distance(d_p.data_ptr(), B, N, d_v.data_ptr(), V, 1, d_f.data_ptr(), F, chunks,
                                                        dist2.data_ptr(), face.data_ptr(), None, None, ws.data_ptr(),
                                                        ws_bytes, stream), "fpsg_point_mesh_distance")

            label = str(chunks) if chunks > 0 else f"library ({ws_bytes // (8 * B * N)})"
            forms[label] = entry
            entry()
            torch.cuda.synchronize()
            results[label] = (dist2.clone(), face.clone())
        first = next(iter(results.values()))
        assert all(torch.equal(r[0], first[0]) and torch.equal(r[1], first[1]) for r in results.values())
        times = {label: [] for label in forms}
        for _ in range(a.rounds):
            for label, fn in forms.items():
                times[label].append(timed(fn, a.iters))
        pairs = B * N * F
        for label, ts in times.items():
            med = sorted(ts)[len(ts) // 2]
            rate = pairs / (med * 1e-6)
            out.append(f"| {name} | {label} | {med:.1f} us | {min(ts):.1f} us | {max(ts):.1f} us | {rate:.3e} | "
                       f"{100 * rate * OPS_PER_PAIR / VALU_RATE:.1f} % |")
    out.append("")
    out.append(f"Device events around {a.iters} back-to-back calls of the C entry (both kernels), {a.rounds} alternating rounds, "
               f"medians over the rounds; {OPS_PER_PAIR} counted operations per pair against {VALU_RATE / 1e12:.2f} T "
               f"unfused fp32 operations per second (half the 157.3 TFLOPS vector peak).")


def tool(out):
    from fpsg_amd.engine import build_model, default_options
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "ckpt", "0"))
        torch.manual_seed(0)
        torch.save(build_model(default_options(device="cuda", n_shot=1, n_query=5)).state_dict(),
                   os.path.join(tmp, "ckpt", "0", "model.pt"))
        base = [sys.executable, os.path.join(ROOT, "generate_meshes.py"), "--synthetic", "--n_shot", "1", "--n_query", "5",
                "--sequential_eval", "--grid", "16", "--max_items", "8", "--model_path", os.path.join(tmp, "ckpt"), "--name",
                "0", "--eval_model", "model.pt"]
        rows = {}
        for label, extra in (("without --metrics", []), ("with --metrics", ["--metrics"])) * 2:
            t0 = time.perf_counter()
            run = subprocess.run(base + ["--output", os.path.join(tmp, label.replace(" ", "_"))] + extra, capture_output=True,
                                 text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
            assert run.returncode == 0, run.stderr[-2000:]
            rows.setdefault(label, []).append(time.perf_counter() - t0)
        out.append("")
        out.append("One `generate_meshes.py` run (the process's wall time, start-up and model build included; 8 items x 5 "
                   "queries, grid 16, sheets written; two runs each, alternating, untrained weights):")
        out.append("")
        for label, ts in rows.items():
            out.append(f"- {label}: " + ", ".join(f"{t:.2f} s" for t in ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 0], help="0: the library's choice")
    ap.add_argument("--tool", action="store_true")
    a = ap.parse_args()
    cli.limit_host_threads()
    out = [f"## tools/bench_point_mesh.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}", ""]
    kernel(a, out)
    if a.tool:
        tool(out)
    print("\n".join(out))
    os.makedirs(os.path.dirname(NOTES), exist_ok=True)
    with open(NOTES, "a") as f:
        f.write("\n".join(out) + "\n\n")


if __name__ == "__main__":
    main()
