#!/usr/bin/env python3
"""rtg_closest_point throughput (DESIGN.md §8 "Proximity queries"): Mpoints/s on icosphere_field for points uniform
in the scene box and points just off the surfaces, schedules 3 and 4 where they run, device-resident batches; a
torch brute-force line (all pairs against the triangles' vertices) at a size where that fits, for scale.
--k 1,4,16: rtg_closest_points instead, one line per k, and torch.topk over the same all-pairs matrix for scale."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-practice_amd", "python"))
import rtgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=3, help="icosphere_field level")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--brute", type=int, default=4096, help="points of the torch brute-force line")
    ap.add_argument("--k", default=None, help="comma-separated list sizes: time rtg_closest_points for each")
    a = ap.parse_args()
    import torch

    lib = rtgpu.Library()
    s = rtgpu.SceneLibrary().build("icosphere_field", grid=a.grid, rand_seed=1, bvh_mode=rtgpu.RTG_BVH_SAH | rtgpu.RTG_BVH_NEAREST)
    ds = lib.scene_create(s.desc)
    prims = np.array([[*p.p0, *p.p1, *p.p2] for p in s.desc.prims[:s.desc.num_prims]])
    verts = np.vstack([prims[:, 0:3], prims[:, 0:3] + prims[:, 3:6], prims[:, 0:3] + prims[:, 6:9]])
    rng = np.random.default_rng(1)
    k = rng.integers(0, len(prims), a.points)
    ab = rng.uniform(0, 0.5, (a.points, 2))
    surf = prims[k, 0:3] + ab[:, :1] * prims[k, 3:6] + ab[:, 1:] * prims[k, 6:9]
    sets = {"uniform": rng.uniform(verts.min(0), verts.max(0), (a.points, 3)), "near": surf + rng.normal(0, 0.01, surf.shape)}
    ks = [int(x) for x in a.k.split(",")] if a.k else [None]
    out = torch.zeros(a.points * max(k or 1 for k in ks), 8, dtype=torch.float32, device="cuda")
    counts = torch.zeros(a.points, dtype=torch.int32, device="cuda")
    for name, p in sets.items():
        pts = np.zeros(a.points, dtype=np.dtype(rtgpu.POINT_DTYPE))
        pts["p"], pts["max_dist"] = p, np.inf
        d_pts = torch.from_numpy(pts.view(np.float32).reshape(-1, 4)).cuda()
        torch.cuda.synchronize()
        for sched, k in [(sched, k) for sched in (3, 4) for k in ks]:
            def run():
                if k is None:
                    return ds.closest_point_device(d_pts.data_ptr(), a.points, out.data_ptr(), schedule=sched)
                return ds.closest_points_device(d_pts.data_ptr(), a.points, k, out.data_ptr(), counts.data_ptr(), schedule=sched)
            try:
                ms = [run().kernel_ms for _ in range(a.steps + 1)][1:]
            except rtgpu.RtgError as e:
                print(json.dumps({"points": name, "schedule": sched, "k": k, "error": str(e)}))
                continue
            print(json.dumps({"points": name, "schedule": sched, "k": k, "n": a.points, "prims": len(prims), "ms_best": min(ms),
                              "ms_median": float(np.median(ms)), "mpoints_per_s": a.points / min(ms) / 1e3}), flush=True)
    # for scale: all-pairs distance to the vertices (cheaper than the triangle test it stands in for)
    q, v = torch.from_numpy(sets["uniform"][:a.brute]).float().cuda(), torch.from_numpy(verts).float().cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cdist(q, v).min(dim=1)
    ev[0].record()
    torch.cdist(q, v).min(dim=1)
    ev[1].record()
    torch.cuda.synchronize()
    print(json.dumps({"torch_brute_force_vertices": a.brute, "ms": ev[0].elapsed_time(ev[1]),
                      "mpoints_per_s": a.brute / ev[0].elapsed_time(ev[1]) / 1e3}))
    for k in [k for k in ks if k is not None]:  # the k smallest of the same matrix
        torch.cdist(q, v).topk(k, dim=1, largest=False)
        ev[0].record()
        torch.cdist(q, v).topk(k, dim=1, largest=False)
        ev[1].record()
        torch.cuda.synchronize()
        print(json.dumps({"torch_topk_brute_force_vertices": a.brute, "k": k, "ms": ev[0].elapsed_time(ev[1]),
                          "mpoints_per_s": a.brute / ev[0].elapsed_time(ev[1]) / 1e3}))
    ds.close()


if __name__ == "__main__":
    main()
