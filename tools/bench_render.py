"""One call of each render entry, by device events, at the shape of profiles/k31/notes.md: a mesh of V = 4096 vertices
and F = 7200 faces (the decoder's 16 patches on a 16 x 16 grid) with 16 `Kd` materials, 3 views, 192 px at ssaa 2, the
image the only output; fpsg_points_render on 5 clouds of 2048 coloured points with the same views and size.  Buffers
are allocated once and the ctypes entries are called on torch's current stream.  One line per entry: median, min and max
over --rounds rounds (the entries alternate inside a round) and the CRC-32 of the image, so that two builds of the
library can be told to draw the same.  Against another build on the same GPU:

    tools/ab_lib.sh <the other libfpsg_hip.so> render python tools/bench_render.py [--rounds 7] [--iters 200]
"""
import argparse
import ctypes
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bench_point_mesh import bumpy_sphere, timed
from fpsg_amd import _hip, cli, meshes

SIZE, SSAA, CLOUDS, POINTS, POINT_RADIUS, ORTHO = 192, 2, 5, 2048, 0.02, 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    cli.limit_host_threads()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    rng = np.random.default_rng(0)
    verts, faces = bumpy_sphere(1)
    V, F, M, R = verts.shape[1], len(faces), 16, SIZE * SSAA
    d_verts, d_faces = torch.from_numpy(verts[0]).to(dev), torch.from_numpy(faces).to(dev)
    d_normals = meshes.vertex_normals(d_verts, d_faces)[d_faces.long()].contiguous()
    d_face_material = torch.from_numpy((np.arange(F) // (F // M)).astype(np.int32)).to(dev)
    materials = np.concatenate([rng.random((M, 3)), np.full((M, 1), -1.0)], axis=1).astype(np.float32)
    c_materials = materials.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    views = meshes.camera_views(60.0, (0, 120, 240))
    NV = len(views)
    d_views = torch.from_numpy(views).to(dev)
    cloud = rng.normal(size=(CLOUDS, POINTS, 3))
    d_points = torch.from_numpy((0.7 * cloud / np.linalg.norm(cloud, axis=2, keepdims=True)).astype(np.float32)).to(dev)
    d_colors = torch.from_numpy(rng.integers(0, 256, (CLOUDS, POINTS, 3), dtype=np.uint8)).to(dev)
    material = meshes.PhongMaterial()
    log2s = material.log2_shininess()
    params = (ctypes.c_float * 17)(*material.params().tolist(), material.ambient, material.diffuse)
    ws_bytes = max(lib.fpsg_mesh_render_materials_workspace_bytes(V, F, NV, R, R, M, 0),
                   lib.fpsg_points_render_workspace_bytes(CLOUDS, POINTS, NV, R, R))
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes // 16 + 1, 2), dtype=torch.int64, device=dev)
    image = torch.zeros((CLOUDS, NV, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)   # a mesh fills image[0]
    stream = _hip.stream_of(d_verts)
    mesh = (d_verts.data_ptr(), V, d_faces.data_ptr(), F)
    tables = (c_materials, M, None, 0, None, 0)
    tail = (d_views.data_ptr(), NV, R, R, SSAA, ORTHO)
    outputs = (params, log2s, None, image.data_ptr(), None, None, None, ws.data_ptr(), ws.numel() * 8, stream)
    calls = {
        "fpsg_mesh_render": (*mesh, *tail, *outputs),
        "fpsg_mesh_render_materials": (*mesh, d_face_material.data_ptr(), None, *tables, *tail, *outputs),
        "fpsg_mesh_render_smooth": (*mesh, d_face_material.data_ptr(), None, d_normals.data_ptr(), *tables, *tail, *outputs),
        "fpsg_points_render": (d_points.data_ptr(), d_colors.data_ptr(), CLOUDS, POINTS, *tail, POINT_RADIUS, *outputs),
    }
    entries, crc = {}, {}
    for name, args in calls.items():
        entries[name] = lambda name=name, args=args: _hip.check(getattr(lib, name)(*args), name)
        entries[name]()
        torch.cuda.synchronize()
        crc[name] = zlib.crc32((image if name == "fpsg_points_render" else image[0]).cpu().numpy().tobytes())
    times = {name: [] for name in entries}
    for _ in range(a.rounds):
        for name, fn in entries.items():
            times[name].append(timed(fn, a.iters))
    for name, ts in times.items():
        print(f"{name}: median {sorted(ts)[len(ts) // 2]:.2f} us, min {min(ts):.2f} us, max {max(ts):.2f} us over {a.rounds} "
              f"rounds of {a.iters} calls; image crc32 {crc[name]:08x}")


if __name__ == "__main__":
    main()
