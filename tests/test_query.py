"""rtg_intersect (DESIGN.md §3 "ray queries", §4 "query semantics"): batched closest-hit / any-hit queries against
the fp32 oracle (equality) and a float64 brute force (triangles, intervals, u / v / normal, any-hit)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtgpu
from test_gpu import _desc
from test_triangles import SKEW, SPHERE, TRI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)
GRID = [(rtgpu.RTG_BVH_MEDIAN, 0), (rtgpu.RTG_BVH_MEDIAN, 4), (rtgpu.RTG_BVH_SAH, 0), (rtgpu.RTG_BVH_SAH, 4),
        (rtgpu.RTG_BVH_SAH, 5), (rtgpu.RTG_BVH_GPU, 0), (rtgpu.RTG_BVH_GPU, 4), (rtgpu.RTG_BVH_GPU, 5)]


def _rays(o, d, tmin=1e-3, tmax=INF):
    r = np.zeros(len(o), dtype=np.dtype(rtgpu.RAY_DTYPE))
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, d, tmin, tmax
    return r


_ORACLE = {}


def _oracle_rays(lib, scenes, oracle, name):
    """2048 camera-like segments and 1024 second-bounce segments from the first hits' o + t d, with the fp32
    oracle's winner and t; computed once per scene."""
    if name not in _ORACLE:
        s = scenes.build(name, rand_seed=1)
        p = lib.camera_resolve(rtgpu.rtg_camera_desc.from_buffer_copy(s.camera))
        c, p00, du, dv = (np.array(x[:]) for x in (p.center, p.pixel00_loc, p.pixel_delta_u, p.pixel_delta_v))
        rng = np.random.default_rng(11)
        i, j = rng.uniform(0, p.image_width, (2048, 1)), rng.uniform(0, p.image_height, (2048, 1))
        o = np.broadcast_to(c, (2048, 3)).astype(np.float32)
        d = (p00 + i * du + j * dv - c).astype(np.float32)
        tm = rng.uniform(0, 1, 3072).astype(np.float32)
        prim, t = oracle.closest_hit32(s.desc, o, d, tm[:2048])
        hit = np.flatnonzero(prim >= 0)[:1024]
        assert len(hit) == 1024
        o2 = (o[hit] + t[hit, None] * d[hit]).astype(np.float32)  # on the surfaces
        d2 = rng.normal(size=(1024, 3)).astype(np.float32)
        o, d, tm = np.vstack([o, o2]), np.vstack([d, d2]), np.concatenate([tm[:2048], tm[hit]])
        _ORACLE[name] = (_rays(o, d), tm) + oracle.closest_hit32(s.desc, o, d, tm)
    return _ORACLE[name]


@pytest.mark.gpu
@pytest.mark.parametrize("bvh,sched", GRID)
@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_box"])
def test_closest_hit_equals_the_fp32_oracle(gpu_lib, scenes, oracle, name, bvh, sched):
    """prim and the bits of t of every ray equal cpu_ref32's: the project's frames are bit-identical to the oracle
    on these scenes and every segment of those frames is such a query (occluder, moving spheres, bvh_node ties)."""
    rays, tm, prim, t = _oracle_rays(gpu_lib, scenes, oracle, name)
    s = scenes.build(name, rand_seed=1, bvh_mode=bvh)  # (kept alive: the descriptor points into it)
    ds = gpu_lib.scene_create(s.desc)
    try:
        hits, st = ds.intersect(rays, tm, schedule=sched)
    except rtgpu.RtgError as e:
        if e.status == rtgpu.RTG_E_UNSUPPORTED:
            pytest.skip(str(e))
        raise
    finally:
        ds.close()
    bad = (hits["prim"] != prim) | (hits["t"].view(np.uint32) != t.view(np.uint32))
    print(f"{name} bvh {bvh} schedule {sched} -> {st.reserved_[0]}: {int(bad.sum())} of {len(rays)} rays differ")
    assert not bad.any(), (np.flatnonzero(bad)[:8], hits["prim"][bad][:8], prim[bad][:8], hits["t"][bad][:8], t[bad][:8])
    assert st.rays == len(rays) and st.hits == int((prim >= 0).sum())


# ---- float64 reference: triangles, intervals, u / v / normal / front_face, any-hit ----
# Bounds: four times the largest error of the first MI355X run (DESIGN.md §4 "query semantics": t 2.95e-5 relative,
# u 1.82e-6, v 1.92e-6, normal 1.52e-6), t's capped at 1e-4: an error above that at these coordinates is a bug.
T_REL, UV_ABS, N_ABS = 1e-4, 7.7e-6, 6.1e-6


def _reference(prims, o, d, tmin, tmax):
    """Per primitive k and ray: the root in the interval (inf: none), u, v, the outward normal; and the rays the
    reference cannot decide (a candidate within 1e-3 of an edge, barycentric, or of grazing, disc / (a r^2))."""
    n = len(o)
    T, U, V, N = np.full((len(prims), n), np.inf), np.zeros((len(prims), n)), np.zeros((len(prims), n)), np.zeros((len(prims), n, 3))
    unsure = np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, (kind, Q, e1, e2, r) in enumerate(prims):
            Q, e1, e2 = (np.asarray(x, dtype=np.float64) for x in (Q, e1, e2))
            if kind == SPHERE:
                oc = o - Q
                a, hb, c = np.sum(d * d, axis=1), np.sum(d * oc, axis=1), np.sum(oc * oc, axis=1) - r * r
                disc = hb * hb - a * c
                sq = np.sqrt(np.maximum(disc, 0))
                t0, t1 = (-hb - sq) / a, (-hb + sq) / a
                ok0, ok1 = (disc > 0) & (tmin < t0) & (t0 < tmax), (disc > 0) & (tmin < t1) & (t1 < tmax)
                t = np.where(ok0, t0, np.where(ok1, t1, np.inf))
                unsure |= (np.abs(disc / (a * r * r)) < 1e-3) & (t1 > tmin)
                out = (o + np.where(np.isfinite(t), t, 0)[:, None] * d - Q) / r
                U[k] = (np.arctan2(-out[:, 2], out[:, 0]) + np.pi) / (2 * np.pi)
                V[k] = np.arccos(np.clip(-out[:, 1], -1, 1)) / np.pi
                N[k] = out
            else:  # Moeller-Trumbore: (alpha, beta) are the barycentrics of e1, e2
                pv = np.cross(d, e2)
                det = pv @ e1
                tv = o - Q
                al = np.sum(pv * tv, axis=1) / det
                qv = np.cross(tv, e1)
                be, t = np.sum(d * qv, axis=1) / det, (qv @ e2) / det
                edges = [al, be, 1 - al - be] if kind == TRI else [al, be, 1 - al, 1 - be]
                inside = np.all([e >= 0 for e in edges], axis=0) & (tmin <= t) & (t <= tmax)
                unsure |= (np.min(np.abs(edges), axis=0) < 1e-3) & (tmin <= t) & (t <= tmax) & (np.min(edges, axis=0) > -1e-3)
                t = np.where(inside, t, np.inf)
                U[k], V[k] = al, be
                N[k] = np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2))
            T[k] = t
    return T, U, V, N, unsure


def _skew_case(variant):
    prims = {"noquad": SKEW[:-1], "quad": SKEW, "quad_reversed": SKEW[::-1]}[variant]
    rng = np.random.default_rng(5)
    o = rng.uniform(-14, 14, (4096, 3))
    tgt = rng.uniform(-8, 8, (4096, 3))
    ln = rng.uniform(0.25, 4, (4096, 1))
    d = (tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True) * ln
    return prims, o.astype(np.float32), d.astype(np.float32), rng


def _float64_case(prims, o32, d32, clip, rng, tag):
    """The reference's answers for one ray set: tmax (inf, or per ray 0.5x / 2x the closest t), per-primitive roots and
    records, the kept rays, the winners. The conditions that keep a case from hiding a failure are asserted here,
    before the GPU is touched: every primitive (but the earlier of a coplanar pair, which the later one covers)
    wins at least 16 kept rays and 25 % of the rays hit; half of each where half the hits are clipped away."""
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    pair = [k for k, p in enumerate(prims) if p[1] == SKEW[0][1]]  # triangle 0 and its coplanar quad
    tmax = np.full(len(o), np.inf)
    if clip:
        t0 = _reference(prims, o, d, 1e-3, tmax)[0].min(axis=0)
        tmax = np.where(np.isfinite(t0), t0 * rng.choice([0.5, 2.0], len(o)), np.inf).astype(np.float32).astype(np.float64)
    T, U, V, N, unsure = _reference(prims, o, d, np.float64(np.float32(1e-3)), tmax)
    order = np.argsort(T, axis=0)
    best, t1, t2 = order[0], np.take_along_axis(T, order[:1], 0)[0], np.take_along_axis(T, order[1:2], 0)[0]
    with np.errstate(invalid="ignore"):
        close = np.isfinite(t1) & (t2 - t1 <= 1e-4 * t1)
    copl = close & np.isin(order[0], pair) & np.isin(order[1], pair) & (len(pair) == 2)
    best = np.where(copl, max(pair), best)  # the later list entry wins the coplanar pair
    keep = ~unsure & ~(close & ~copl)
    hit = np.isfinite(t1)
    best = np.where(hit, best, -1)
    wins = np.bincount(best[keep & hit], minlength=len(prims))
    print(f"{tag} clip {clip}: left out {1 - keep.mean():.4f}, hit {hit.mean():.3f}, wins {wins.tolist()}")
    counted = [k for k in range(len(prims)) if len(pair) < 2 or k != min(pair)]
    assert 1 - keep.mean() <= 0.02
    assert hit.mean() >= (0.125 if clip else 0.25) and wins[counted].min() >= (8 if clip else 16)
    return dict(o=o, d=d, tmax=tmax, T=T, U=U, V=V, N=N, keep=keep, hit=hit, best=best, t1=t1)


def _check_against_float64(gpu_lib, prims, o32, d32, ref, schedule=0):
    """Closest and any-hit queries of the scene `prims` against _float64_case's answers. Kept rays: prim and
    front_face equal, t / u / v / normal within the bounds above; any-hit: hit / miss equal and the returned
    primitive has a reference root at the returned t."""
    d, T, keep, hit, best, t1 = (ref[n] for n in ("d", "T", "keep", "hit", "best", "t1"))
    d_ = _desc([rtgpu.rtg_primitive(kind=kind, material=0, p0=rtgpu.D3(*Q), p1=rtgpu.D3(*u), p2=rtgpu.D3(*v), radius=r)
                for kind, Q, u, v, r in prims], [rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=0)],
               [rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(1, 1, 1))])
    ds = gpu_lib.scene_create(d_)
    rays = _rays(o32, d32, 1e-3, ref["tmax"].astype(np.float32))
    h, st = ds.intersect(rays, schedule=schedule)
    a, _ = ds.intersect(rays, any_hit=True, schedule=schedule)
    ds.close()
    assert st.reserved_[0] == (schedule or 3)
    k = keep & hit
    assert np.array_equal(h["prim"][keep], best[keep])
    rows = np.arange(len(d))
    bk = np.maximum(best, 0)
    n_ref = ref["N"][bk, rows]
    front = np.sum(d * n_ref, axis=1) < 0
    n_ref = np.where(front[:, None], n_ref, -n_ref)
    assert np.array_equal(h["front_face"][k], front[k].astype(np.int32))
    du = np.abs(h["u"] - ref["U"][bk, rows])
    du = np.where(np.array([p[0] for p in prims])[bk] == SPHERE, np.minimum(du, 1 - du), du)  # a sphere's u is periodic
    err = {"t": np.max(np.abs(h["t"][k] - t1[k]) / t1[k]), "u": du[k].max(), "v": np.abs(h["v"] - ref["V"][bk, rows])[k].max(),
           "normal": np.abs(h["normal"] - n_ref)[k].max()}
    print("largest errors", {n: float(e) for n, e in err.items()})
    assert err["t"] <= T_REL and err["u"] <= UV_ABS and err["v"] <= UV_ABS and err["normal"] <= N_ABS
    assert np.all(h["prim"][keep & ~hit] == -1) and np.all(h["t"][keep & ~hit] == -1)
    # any-hit: the same hit / miss; the returned primitive really has a root at the returned t
    assert np.array_equal(a["prim"][keep] >= 0, hit[keep])
    ta = T[np.maximum(a["prim"], 0), rows]
    assert np.all(np.abs(a["t"][k] - ta[k]) <= T_REL * ta[k])


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("variant", ["noquad", "quad", "quad_reversed"])
def test_skew_scene_matches_float64(gpu_lib, variant, clip):
    """The SKEW primitives of test_triangles.py (a mixed scene), tmax = inf or clipped."""
    prims, o32, d32, rng = _skew_case(variant)
    _check_against_float64(gpu_lib, prims, o32, d32, _float64_case(prims, o32, d32, clip, rng, variant))


# A sphere whose box spans the scene: the SAH build keeps it out of the tree (DevScene::occluder) and every
# query ray tests it first. It lies to the side (-x), so the rays see it away from get_sphere_uv's poles and seam.
GROUND = (SPHERE, (-50, 0, 0), (-50, 0, 0), (0, 0, 0), 40.0)


@pytest.mark.gpu
@pytest.mark.parametrize("sched", [0, 5])
@pytest.mark.parametrize("ground", [False, True])
def test_triangle_only_tree_matches_float64(gpu_lib, ground, sched):
    """The SKEW triangles alone: the triangle-only kernel class (whole scene in LDS, and the treelet's spilling
    stack form); with the scene-spanning sphere first in the list the tree is still triangles only, but the winner
    may be the sphere, so the mixed class answers and every input index moves by one."""
    _, o32, d32, rng = _skew_case("noquad")
    prims = ([GROUND] if ground else []) + SKEW[:7]
    _check_against_float64(gpu_lib, prims, o32, d32, _float64_case(prims, o32, d32, False, rng, f"ground {ground}"), sched)


# ---- shapes at which the kernel can go wrong (Cornell box against the oracle values above) ----
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_ray_counts_at_wave_edges(gpu_lib, scenes, oracle, n):
    rays, tm, prim, t = _oracle_rays(gpu_lib, scenes, oracle, "cornell_box")
    s = scenes.build("cornell_box", rand_seed=1)
    ds = gpu_lib.scene_create(s.desc)
    hits, st = ds.intersect(rays[:n], tm[:n])
    ds.close()
    assert st.rays == n and np.array_equal(hits["prim"], prim[:n]) and np.array_equal(hits["t"], t[:n])


@pytest.mark.gpu
def test_one_workgroup_refills_and_leaves_the_guard_row_alone(gpu_lib, scenes, oracle):
    """max_workgroups = 1 with 3000 rays: every lane refills many times; the device-pointer, stream, async path
    (through torch) gives the host path's bytes and writes nothing past num_rays."""
    import torch

    rays, tm, prim, t = _oracle_rays(gpu_lib, scenes, oracle, "cornell_box")
    rays, tm, n = rays[:3000], tm[:3000], 3000
    s = scenes.build("cornell_box", rand_seed=1)
    ds = gpu_lib.scene_create(s.desc)
    ref, _ = ds.intersect(rays, tm)
    one, st = ds.intersect(rays, tm, max_workgroups=1)
    assert st.reserved_[1] == 1 and one.tobytes() == ref.tobytes()
    assert np.array_equal(ref["prim"], prim[:n]) and np.array_equal(ref["t"], t[:n])
    d_rays = torch.from_numpy(rays.view(np.float32).copy()).cuda()
    d_tm = torch.from_numpy(tm.copy()).cuda()
    d_hits = torch.full(((n + 1) * 8,), 7.0, dtype=torch.float32, device="cuda")  # one guard row after the array
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ds.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_tm.data_ptr(), stream.cuda_stream,
                        max_workgroups=1, asynchronous=True)
    stream.synchronize()
    got = d_hits.cpu().numpy()
    ds.close()
    assert got[:n * 8].tobytes() == ref.tobytes() and np.all(got[n * 8:] == 7.0)


@pytest.mark.gpu
@pytest.mark.parametrize("sched", [0, 4])
def test_spill_stack_answers_as_the_default_stack(gpu_lib, scenes, oracle, monkeypatch, sched):
    rays, tm, prim, t = _oracle_rays(gpu_lib, scenes, oracle, "bouncing_spheres")
    monkeypatch.setenv("RTG_STACK_LDS_ENTRIES", "1")
    s = scenes.build("bouncing_spheres", rand_seed=1)
    ds = gpu_lib.scene_create(s.desc)  # knobs are read once per scene
    hits, _ = ds.intersect(rays, tm, schedule=sched)
    ds.close()
    assert np.array_equal(hits["prim"], prim) and np.array_equal(hits["t"], t)


# ---- host tests (no GPU) ----
def test_query_struct_sizes_match_the_header(tmp_path):
    names = ["rtg_ray", "rtg_hit", "rtg_query_desc", "rtg_query_stats"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rtgpu.h"\nint main(void) {\n' +
                   "".join(f'printf("%zu\\n", sizeof({n}));\n' for n in names) + "return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "sizes")], check=True)
    got = subprocess.run([str(tmp_path / "sizes")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(g) for g in got] == [C.sizeof(getattr(rtgpu, n)) for n in names]
    assert C.sizeof(rtgpu.rtg_ray) == 32 == np.dtype(rtgpu.RAY_DTYPE).itemsize
    assert C.sizeof(rtgpu.rtg_hit) == 32 == np.dtype(rtgpu.HIT_DTYPE).itemsize


@pytest.mark.parametrize("case", ["null_desc", "negative", "async_without_device"])
def test_intersect_rejects_bad_arguments(lib, case):
    """The descriptor is validated before the scene is looked at (rtgpu.h), so a NULL scene reaches these checks."""
    buf = (C.c_char * 64)()
    q = rtgpu.rtg_query_desc(C.addressof(buf), None, -1 if case == "negative" else 1, C.addressof(buf),
                             rtgpu.RTG_QUERY_ASYNC if case == "async_without_device" else 0, 0, None)
    st = lib.lib.rtg_intersect(None, None if case == "null_desc" else C.byref(q), None)
    want = {"null_desc": b"null", "negative": b"num_rays", "async_without_device": b"RTG_QUERY_ASYNC"}[case]
    assert st == rtgpu.RTG_E_INVALID and want in lib.lib.rtg_last_error()
