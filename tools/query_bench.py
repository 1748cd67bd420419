#!/usr/bin/env python3
"""tools/query_bench.py — rtg_intersect throughput beside the render's, on the config-2 scene and camera.

The primary rays of the 1920x1080 camera (pixel centres, from the lens centre, time 0), once in pixel order and
once under a fixed-seed shuffle, as closest-hit and as any-hit queries; times are rtg_query_stats.kernel_ms,
best of three after a warm-up. The render line is the same scene at --spp samples: segments / kernel_ms. Every
GPU step runs in a child process under its own time limit, and the tool stops at the first step that fails.
Prints one JSON line per step and a summary line with the ratios.

`bounce` is the workload RTG_QUERY_SORT is for: the second segments of the primary rays that hit, from o + t d in
the direction normal + a fixed-seed random unit vector, in pixel order of their parents (closest hit). --sort adds
a `_sorted` twin of every query step (the same batch with RTG_QUERY_SORT; `sort_us` is the sort kernels' share of
kernel_ms); --grid picks the scene's size (500: the 1M-sphere scene of bench.py config 5, treelet schedule);
--steps runs a subset (the render of a large scene takes long).
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-practice_amd", "python"))
STEPS = ["render", "closest_ordered", "closest_shuffled", "any_ordered", "any_shuffled", "bounce"]
SORTED = [n + "_sorted" for n in STEPS[1:]]


def step(name, a):
    import numpy as np

    import rtgpu

    lib = rtgpu.Library()
    s = rtgpu.SceneLibrary().build("bouncing_spheres", grid=a.grid, rand_seed=1)
    cam = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    cam.image_width, cam.aspect_ratio, cam.samples_per_pixel, cam.max_depth = a.width, a.width / a.height, a.spp, 50
    ds = lib.scene_create(s.desc)
    if name == "render":
        ms, segs = [], 0
        for _ in range(4):  # the first is the warm-up
            _, st = ds.render_host(cam)
            ms.append(st.kernel_ms)
            segs = st.segments
        plan = ds.plan(cam)
        out = {"step": name, "kernel_ms": min(ms[1:]), "rays": int(segs), "schedule": plan.schedule,
               "workgroups": plan.workgroups, "waves_per_workgroup": plan.waves_per_workgroup, "lds_bytes": plan.lds_bytes}
    else:
        p = lib.camera_resolve(cam)
        c, p00, du, dv = (np.array(x[:]) for x in (p.center, p.pixel00_loc, p.pixel_delta_u, p.pixel_delta_v))
        jj, ii = np.mgrid[0:p.image_height, 0:p.image_width]
        rays = np.zeros(ii.size, dtype=np.dtype(rtgpu.RAY_DTYPE))
        rays["origin"] = c
        rays["dir"] = p00 + ii.reshape(-1, 1) * du + jj.reshape(-1, 1) * dv - c
        rays["tmin"], rays["tmax"] = 1e-3, np.inf
        sort = name.endswith("_sorted")
        if "shuffled" in name:
            rays = rays[np.random.default_rng(7).permutation(len(rays))]
        if name.startswith("bounce"):
            h, _ = ds.intersect(rays, max_workgroups=a.max_workgroups)
            hit = h["prim"] >= 0
            rays, h = rays[hit], h[hit]
            rng = np.random.default_rng(7)
            v = rng.standard_normal((len(rays), 3), dtype=np.float32)
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            rays["origin"] += h["t"][:, None] * rays["dir"]
            rays["dir"] = h["normal"] + v
            del h, v, hit
        ms, sort_us = [], []
        for _ in range(4):
            _, st = ds.intersect(rays, any_hit=name.startswith("any"), max_workgroups=a.max_workgroups, sort=sort)
            ms.append(st.kernel_ms)
            sort_us.append(int(st.reserved_[4]))
        best = 1 + int(np.argmin(ms[1:]))
        out = {"step": name, "kernel_ms": ms[best], "sort_us": sort_us[best], "rays": int(st.rays), "hits": int(st.hits),
               "schedule": int(st.reserved_[0]), "workgroups": int(st.reserved_[1]),
               "waves_per_workgroup": int(st.reserved_[2]), "lds_bytes": int(st.reserved_[3])}
    ds.close()
    out["grays_per_s"] = out["rays"] / out["kernel_ms"] * 1e-6
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16, help="samples per pixel of the render line")
    ap.add_argument("--max-workgroups", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per GPU step")
    ap.add_argument("--grid", type=int, default=11, help="bouncing_spheres grid half-width (500: 1M spheres)")
    ap.add_argument("--sort", action="store_true", help="also run every query step with RTG_QUERY_SORT")
    ap.add_argument("--steps", help="comma-separated subset of " + ",".join(STEPS))
    ap.add_argument("--step", choices=STEPS + SORTED)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    res = {}
    names = a.steps.split(",") if a.steps else STEPS
    if any(n not in STEPS for n in names):
        ap.error("--steps takes names out of " + ",".join(STEPS))
    for name in [m for n in names for m in ([n, n + "_sorted"] if a.sort and n != "render" else [n])]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [
            f"--{k.replace('_', '-')}={getattr(a, k)}" for k in ("width", "height", "spp", "max_workgroups", "grid")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.exit(f"step {name} failed ({r.returncode}):\n{r.stderr[-2000:]}")
        line = r.stdout.strip().splitlines()[-1]
        print(line)
        res[name] = json.loads(line)
    g = {k: v["grays_per_s"] for k, v in res.items()}
    summary = {"summary": {k: round(v, 3) for k, v in g.items()}}
    for key, num, den in [("closest_to_render", "closest_ordered", "render"),
                          ("shuffled_to_ordered_closest", "closest_shuffled", "closest_ordered"),
                          ("shuffled_to_ordered_any", "any_shuffled", "any_ordered")] + [
                              ("sorted_to_unsorted_" + n, n + "_sorted", n) for n in STEPS[1:]]:
        if num in g and den in g:
            summary[key] = round(g[num] / g[den], 3)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
