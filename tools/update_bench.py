#!/usr/bin/env python3
"""tools/update_bench.py — rtg_scene_update beside the scene creations it replaces, on icosphere_field.

Per subdivision level (default 5 and 7: 102 k and 1.6 M triangles), each step in its own process under its own time
limit, best of three after a warm-up:
  create_gpu / create_sah  wall time of rtg_scene_create (RTG_BVH_GPU / RTG_BVH_SAH) of the deformed mesh
  update                   rtg_update_stats.kernel_ms of a whole-mesh device-pointer update (torch tensor) to the
                           deformed mesh, its two parts, and the bytes it moves against the peak HBM bandwidth
  trace_refit / trace_sah  closest-hit Grays/s of the camera's primary rays on the refitted SAH tree and on a fresh
                           SAH tree of the deformed mesh
The deformation: every icosphere scaled by 1.5 about its centre, every vertex displaced by a low-frequency sine of
a tenth of the sphere radius. Prints one JSON line per step and a summary line per level.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-practice_amd", "python"))
STEPS = ["create_gpu", "create_sah", "update", "trace_refit", "trace_sah"]
HBM_GBPS = 8000.0  # the MI355X's peak HBM bandwidth (8 TB/s): the floor is the update's bytes, reads and writes, over it


def _mesh(s):
    """(n, 12) float32 update rows of the scene's primitives and their deformed twins (triangles only move)."""
    import numpy as np

    import rtgpu

    n = s.desc.num_prims
    raw = np.ctypeslib.as_array(C.cast(s.desc.prims, C.POINTER(C.c_char)), (n * C.sizeof(rtgpu.rtg_primitive),))
    prims = raw.view(np.dtype([("kind", "<i4"), ("material", "<i4"), ("p0", "<f8", 3), ("p1", "<f8", 3), ("p2", "<f8", 3),
                               ("radius", "<f8")]))
    assert prims.dtype.itemsize == C.sizeof(rtgpu.rtg_primitive) and np.all(prims["kind"] == rtgpu.RTG_PRIM_TRIANGLE)
    a = np.zeros((n, 12), np.float32)
    a[:, 0:3], a[:, 4:7], a[:, 8:11] = prims["p0"], prims["p1"], prims["p2"]
    b = a.copy()
    per = (n - 2) // 5  # two ground triangles, then five icospheres
    for k in range(5):
        blk = slice(2 + k * per, 2 + (k + 1) * per)
        v = np.stack([a[blk, 0:3], a[blk, 0:3] + a[blk, 4:7], a[blk, 0:3] + a[blk, 8:11]]).astype(np.float64)
        c = v.reshape(-1, 3).mean(axis=0)
        r = np.linalg.norm(v[0] - c, axis=1).mean()
        w = c + 1.5 * (v - c)
        w += 0.1 * r * np.sin(w[..., [1, 2, 0]] * (1.0 / r))
        b[blk, 0:3], b[blk, 4:7], b[blk, 8:11] = w[0], w[1] - w[0], w[2] - w[0]
    return a, b


def _desc_of(s, rows):
    """The scene's descriptor with the primitives' coordinates replaced (kept alive by the returned array)."""
    import numpy as np

    import rtgpu

    P = (rtgpu.rtg_primitive * len(rows))()
    C.memmove(P, s.desc.prims, C.sizeof(P))
    v = np.frombuffer(P, dtype=np.dtype([("kind", "<i4"), ("material", "<i4"), ("p0", "<f8", 3), ("p1", "<f8", 3),
                                         ("p2", "<f8", 3), ("radius", "<f8")]))
    v["p0"], v["p1"], v["p2"] = rows[:, 0:3], rows[:, 4:7], rows[:, 8:11]
    d = rtgpu.rtg_scene_desc.from_buffer_copy(s.desc)
    d.prims = C.cast(P, C.POINTER(rtgpu.rtg_primitive))
    d._keep = P
    return d


def step(name, a):
    import numpy as np

    import rtgpu

    lib = rtgpu.Library()
    s = rtgpu.SceneLibrary().build("icosphere_field", grid=a.level, rand_seed=1)
    base, moved = _mesh(s)
    out = {"step": name, "level": a.level, "prims": len(base)}
    if name.startswith("create"):
        d = _desc_of(s, moved)
        d.bvh_mode = rtgpu.RTG_BVH_GPU if name == "create_gpu" else rtgpu.RTG_BVH_SAH
        ms = []
        for _ in range(4):  # the first is the warm-up
            t0 = time.perf_counter()
            ds = lib.scene_create(d)
            ms.append((time.perf_counter() - t0) * 1e3)
            out["nodes"] = int(ds.info().num_nodes)
            ds.close()
        out["wall_ms"] = min(ms[1:])
    elif name == "update":
        import torch

        s.desc.bvh_mode = rtgpu.RTG_BVH_SAH | rtgpu.RTG_BVH_REFIT
        ds = lib.scene_create(s.desc)
        dev = [torch.from_numpy(x).cuda() for x in (moved, base)]
        torch.cuda.synchronize()
        best = None
        for k in range(4):
            st = ds.update_device(0, dev[k % 2].data_ptr(), len(base))
            if k and (best is None or st.kernel_ms < best[0]):
                best = (st.kernel_ms, st.reserved_[0] * 1e-6)
        nodes = int(ds.info().num_nodes)
        ds.close()
        # bytes: updates read (48), records (48) and vertex boxes (24) written; boxes (24) and references (4) read by
        # the refit; per node the code row read twice, the plane rows written and (inner slots) read back, two table words
        moved_bytes = len(base) * (48 + 48 + 24 + 24 + 4) + nodes * (112 + 16 + 96 + 8)
        out.update(kernel_ms=best[0], records_ms=best[1], refit_ms=best[0] - best[1], nodes=nodes, bytes=moved_bytes,
                   floor_ms=moved_bytes / HBM_GBPS * 1e-6, launch=f"records {(len(base) + 255) // 256} x 256, "
                   f"parents and refit {(nodes * 4 + 255) // 256} x 256 each")
        out["floor_share"] = out["floor_ms"] / out["kernel_ms"]
    else:
        cam = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
        cam.image_width, cam.aspect_ratio = 1920, 1920 / 1080
        p = lib.camera_resolve(cam)
        c, p00, du, dv = (np.array(x[:]) for x in (p.center, p.pixel00_loc, p.pixel_delta_u, p.pixel_delta_v))
        jj, ii = np.mgrid[0:p.image_height, 0:p.image_width]
        rays = np.zeros(ii.size, dtype=np.dtype(rtgpu.RAY_DTYPE))
        rays["origin"] = c
        rays["dir"] = p00 + ii.reshape(-1, 1) * du + jj.reshape(-1, 1) * dv - c
        rays["tmin"], rays["tmax"] = 1e-3, np.inf
        if name == "trace_refit":
            s.desc.bvh_mode = rtgpu.RTG_BVH_SAH | rtgpu.RTG_BVH_REFIT
            ds = lib.scene_create(s.desc)
            ds.update(None, moved)
        else:
            ds = lib.scene_create(_desc_of(s, moved))
        ms = []
        for _ in range(4):
            hits, st = ds.intersect(rays)
            ms.append(st.kernel_ms)
        ds.close()
        out.update(kernel_ms=min(ms[1:]), rays=int(st.rays), hits=int(st.hits), schedule=int(st.reserved_[0]),
                   grays_per_s=st.rays / min(ms[1:]) * 1e-6, checksum=int(hits["prim"].astype(np.int64).sum()))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="5,7")
    ap.add_argument("--level", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--step", choices=STEPS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    for level in (int(x) for x in a.levels.split(",")):
        res = {}
        for name in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, f"--level={level}"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.exit(f"step {name} (level {level}) failed ({r.returncode}):\n{r.stderr[-2000:]}")
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[name] = json.loads(line)
        u = res["update"]
        print(json.dumps({"summary": level, "update_ms": round(u["kernel_ms"], 4),
                          "gpu_build_over_update": round(res["create_gpu"]["wall_ms"] / u["kernel_ms"], 1),
                          "sah_build_over_update": round(res["create_sah"]["wall_ms"] / u["kernel_ms"], 1),
                          "floor_share": round(u["floor_share"], 3),
                          "refit_over_fresh_trace": round(res["trace_refit"]["grays_per_s"] / res["trace_sah"]["grays_per_s"], 3),
                          "same_answers": res["trace_refit"]["checksum"] == res["trace_sah"]["checksum"]}), flush=True)


if __name__ == "__main__":
    main()
