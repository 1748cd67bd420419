"""rtg_scene_update (DESIGN.md §3 "Scene updates"): a scene created with RTG_BVH_REFIT, moved on the device, answers
bit for bit as a freshly created scene of the moved primitives does, and agrees with a float64 brute force."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtgpu
from test_gpu import _desc
from test_query import GRID, N_ABS, T_REL, UV_ABS, _rays, _reference
from test_triangles import QUAD, SPHERE, TRI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFIT = rtgpu.RTG_BVH_REFIT
BIG = 768  # the scene-spanning sphere: the SAH and device builds keep it out of the tree (the occluder)


def _scene():
    """(kinds, A, B): 769 primitives as (n, 12) float32 rtg_prim_update rows, before (A) and after (B) the move. A
    16 x 16 grid of unit cells, two triangles and a sphere or a skew quad per cell, then the big sphere. The move:
    every primitive displaced by up to four cell widths and scaled by 1.25 (the big sphere: shifted and grown).
    The grid is centred on the origin and the small spheres have radius 0.6 (0.75 moved): see _ray_set."""
    rng = np.random.default_rng(3)
    cell = np.stack(np.meshgrid(np.arange(16.0) - 8, np.arange(16.0) - 8), -1).reshape(-1, 2)
    n = 3 * len(cell) + 1
    kinds, A = np.full(n, TRI), np.zeros((n, 12), np.float32)
    for c, (x, y) in enumerate(cell):
        j = rng.uniform(-0.05, 0.05, (3, 9))
        A[3 * c, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = np.array([x + 0.1, y + 0.1, 0.2, 0.7, 0.1, 0.2, 0.1, 0.7, -0.2]) + j[0]
        A[3 * c + 1, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = np.array([x + 0.9, y + 0.9, 0.8, -0.6, 0.1, 0.1, 0.1, -0.6, 0.3]) + j[1]
        if (int(x) + int(y)) % 2:
            kinds[3 * c + 2] = QUAD
            A[3 * c + 2, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = np.array([x + 0.2, y + 0.2, -0.7, 0.6, 0.1, 0.1, -0.1, 0.5, 0.2]) + j[2]
        else:
            kinds[3 * c + 2] = SPHERE
            A[3 * c + 2, [0, 1, 2]] = A[3 * c + 2, [4, 5, 6]] = np.array([x + 0.5, y + 0.5, -0.6], np.float32) + j[2, :3].astype(np.float32)
            A[3 * c + 2, 3] = 0.6
    kinds[BIG], A[BIG, :8] = SPHERE, [0, 0, -40, 30, 0, 0, -40, 0]
    k = np.arange(n)[:, None]
    disp = (4.0 * np.hstack([np.sin(0.7 * k), np.cos(1.3 * k), 0.5 * np.sin(2.1 * k)])).astype(np.float32)
    B = A.copy()
    B[:, 0:3] += disp
    B[:, [3, 4, 5, 6, 8, 9, 10]] *= np.float32(1.25)
    sph = kinds == SPHERE
    B[sph, 4:7] = B[sph, 0:3]
    B[BIG, :8] = [1, -2, -43, 31, 1, -2, -43, 0]
    return kinds, A, B


KINDS, A, B = _scene()
N = len(A)


def _fresh_desc(P, bvh=rtgpu.RTG_BVH_SAH):
    d = _desc([rtgpu.rtg_primitive(kind=int(k), material=0, p0=rtgpu.D3(*map(float, p[0:3])), p1=rtgpu.D3(*map(float, p[4:7])),
                                   p2=rtgpu.D3(*map(float, p[8:11])), radius=float(p[3])) for k, p in zip(KINDS, P)],
              [rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=0)],
              [rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(1, 1, 1))])
    d.bvh_mode = bvh
    return d


def _ray_set(P, seed=5, n=4096, near=False):
    """As test_query's _skew_case over the small primitives' extent, from above (misses meet the big sphere).
    near: origins just above the primitives and targets within 3 units sideways. A sphere's fp32 root loses
    about 2^-24 (distance / r)^2 relative to r to the discriminant's cancellation, and its normal is the hit point
    over r; test_query's N_ABS was measured at distance / r of about 8, which these rays keep below 10."""
    rng = np.random.default_rng(seed)
    lo, hi = P[:BIG, 0:3].min(axis=0) - 1, P[:BIG, 0:3].max(axis=0) + 2
    o = np.column_stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng.uniform(*((1.5, 3) if near else (6, 12)), n)])
    tgt = rng.uniform(lo, hi, (n, 3))
    if near:
        tgt[:, :2] = o[:, :2] + rng.uniform(-3, 3, (n, 2))
    d = (tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True) * rng.uniform(0.25, 4, (n, 1))
    return _rays(o.astype(np.float32), d.astype(np.float32), 1e-3)


_CACHE = {}


def _fresh(lib, key, P, rays):
    """Closest and any-hit answers of a freshly created scene of the primitives P; once per key."""
    key = (key, len(rays))
    if key not in _CACHE:
        ds = lib.scene_create(_fresh_desc(P))
        _CACHE[key] = (ds.intersect(rays)[0], ds.intersect(rays, any_hit=True)[0]["prim"] >= 0)
        ds.close()
    return _CACHE[key]


def _same(ds, rays, want, schedule=0):
    h, _ = ds.intersect(rays, schedule=schedule)
    a, _ = ds.intersect(rays, any_hit=True, schedule=schedule)
    bad = np.any(h.view(np.uint32).reshape(-1, 8) != want[0].view(np.uint32).reshape(-1, 8), axis=1)
    print(f"{int(bad.sum())} of {len(rays)} closest-hit records differ, hits {int((want[0]['prim'] >= 0).sum())}")
    assert not bad.any(), (np.flatnonzero(bad)[:8], h[bad][:4], want[0][bad][:4])
    assert np.array_equal(a["prim"] >= 0, want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("bvh,sched", GRID)
def test_updated_scene_equals_a_fresh_one(gpu_lib, bvh, sched):
    """Whole-mesh update (indices NULL): the raw 32-byte closest-hit records and the any-hit pattern equal the fresh
    scene's. A refit that does nothing or stops a level short loses hits: the move leaves most old boxes behind."""
    rays = _ray_set(B)
    want = _fresh(gpu_lib, "moved", B, rays)
    ds = gpu_lib.scene_create(_fresh_desc(A, bvh | REFIT))
    try:
        assert ds.info().bvh_mode == bvh | REFIT
        st = ds.update(None, B)
        assert st.updated == N and st.invalid == 0 and st.kernel_ms > 0
        _same(ds, rays, want, sched)
    finally:
        ds.close()


@pytest.mark.gpu
def test_updated_scene_matches_float64(gpu_lib):
    """The updated scene against test_query's float64 brute force and its bounds, on rays for which the reference
    alone (asserted before the GPU is touched) leaves out at most 2 %, hits at least 25 %, and whose closest hit
    lies outside the winner's old vertex box for most kept rays."""
    rays = _ray_set(B, near=True)
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    prims = [(int(k), p[0:3], p[4:7], p[8:11], float(p[3])) for k, p in zip(KINDS, B.astype(np.float64))]
    T, U, V, Nn, unsure = _reference(prims, o, d, np.float64(np.float32(1e-3)), np.full(len(o), np.inf))
    order = np.argsort(T, axis=0)
    best, rows = order[0], np.arange(len(o))
    t1, t2 = T[best, rows], T[order[1], rows]
    hit = np.isfinite(t1)
    with np.errstate(invalid="ignore"):
        keep = ~unsure & ~(hit & (t2 - t1 <= 1e-4 * t1))
    k = keep & hit
    small = k & (best != BIG)
    pt = o + t1[:, None] * d
    e1 = np.where((KINDS == SPHERE)[:, None], 0, A[:, 4:7])
    verts = np.stack([A[:, 0:3], A[:, 0:3] + e1, A[:, 0:3] + A[:, 8:11]]).astype(np.float64)
    old_lo, old_hi = verts.min(axis=0) - A[:, 3:4], verts.max(axis=0) + A[:, 3:4]  # (a sphere's: centre -+ radius)
    outside = np.any((pt < old_lo[best]) | (pt > old_hi[best]), axis=1)
    print(f"left out {1 - keep.mean():.4f}, hit {hit.mean():.3f}, small winners {int(small.sum())}, outside the old box "
          f"{outside[small].mean():.3f}")
    assert 1 - keep.mean() <= 0.02 and hit.mean() >= 0.25 and small.sum() >= 1000 and outside[small].mean() > 0.5
    ds = gpu_lib.scene_create(_fresh_desc(A, rtgpu.RTG_BVH_SAH | REFIT))
    ds.update(None, B)
    h, _ = ds.intersect(rays)
    a, _ = ds.intersect(rays, any_hit=True)
    ds.close()
    assert np.array_equal(h["prim"][keep], np.where(hit, best, -1)[keep])
    n_ref = Nn[best, rows]
    front = np.sum(d * n_ref, axis=1) < 0
    n_ref = np.where(front[:, None], n_ref, -n_ref)
    assert np.array_equal(h["front_face"][k], front[k].astype(np.int32))
    du = np.abs(h["u"] - U[best, rows])
    du = np.where(KINDS[best] == SPHERE, np.minimum(du, 1 - du), du)
    err = {"t": np.max(np.abs(h["t"][k] - t1[k]) / t1[k]), "u": du[k].max(), "v": np.abs(h["v"] - V[best, rows])[k].max(),
           "normal": np.abs(h["normal"] - n_ref)[k].max()}
    print("largest errors", {n: float(e) for n, e in err.items()})
    assert err["t"] <= T_REL and err["u"] <= UV_ABS and err["v"] <= UV_ABS and err["normal"] <= N_ABS
    assert np.array_equal(a["prim"][keep] >= 0, hit[keep])


def _partial(count):
    idx = np.random.default_rng(count).permutation(N)[:count].astype(np.int32)  # shuffled, distinct
    P = A.copy()
    P[idx] = B[idx]
    return idx, P


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, N - 1, "occluder"])
def test_partial_updates(gpu_lib, count, device):
    """Explicit shuffled indices at the wave edges, from host arrays and from torch tensors; the occluder alone."""
    idx, P = (np.array([BIG], np.int32), np.vstack([A[:BIG], B[BIG:]])) if count == "occluder" else _partial(count)
    rays = _ray_set(B)
    want = _fresh(gpu_lib, ("partial", count), P, rays)
    ds = gpu_lib.scene_create(_fresh_desc(A, rtgpu.RTG_BVH_SAH | REFIT))
    try:
        if device:
            import torch

            d_idx, d_p = torch.from_numpy(idx).cuda(), torch.from_numpy(np.ascontiguousarray(P[idx])).cuda()
            torch.cuda.synchronize()
            st = ds.update_device(d_idx.data_ptr(), d_p.data_ptr(), len(idx))
        else:
            st = ds.update(idx, P[idx])
        assert st.updated == len(idx) and st.invalid == 0
        _same(ds, rays, want)
    finally:
        ds.close()


@pytest.mark.gpu
def test_origin_bound_rises_and_stays(gpu_lib):
    """Five primitives out to 16x the scene's reach: M grows, rays aimed at them from outside the old extent equal
    the fresh scene's; moved back, M stays."""
    idx = np.array([5, 100, 301, 303, 600], np.int32)  # a quad and four triangles
    far = A.copy()
    far[idx, 0] += np.float32(16 * 70)
    rng = np.random.default_rng(9)
    tgt = np.repeat(far[idx, 0:3] + 0.3 * (far[idx, 4:7] + far[idx, 8:11]), 64, axis=0) + rng.uniform(-0.3, 0.3, (320, 3))
    o = tgt + rng.uniform(-1, 1, (320, 3)) + [0, 0, 9]
    rays = np.concatenate([_rays(o.astype(np.float32), (tgt - o).astype(np.float32), 1e-3), _ray_set(A, n=1024)])
    want = _fresh(gpu_lib, "far", far, rays)
    assert (want[0]["prim"][:320] >= 0).mean() > 0.5
    ds = gpu_lib.scene_create(_fresh_desc(A, rtgpu.RTG_BVH_SAH | REFIT))
    try:
        m0 = ds.update(idx, A[idx]).origin_bound
        m1 = ds.update(idx, far[idx]).origin_bound
        assert 69 < m0 < 72 and 1120 < m1 < 1140
        _same(ds, rays, want)
        assert ds.update(idx, A[idx]).origin_bound == m1
        _same(ds, rays, _fresh(gpu_lib, "base", A, rays))
    finally:
        ds.close()


CAM = dict(image_width=64, aspect_ratio=1.0, samples_per_pixel=4, max_depth=8, vfov=70.0, lookfrom=(0, 0, 14),
           lookat=(0, 0, 0), background=(0.7, 0.8, 1.0))


@pytest.mark.gpu
def test_update_after_prepare(gpu_lib):
    """rtg_scene_prepare on the treelet schedule renumbers the node array (hot treelet); the refit derives its
    parents from the array as it is."""
    rays = _ray_set(B)
    want = _fresh(gpu_lib, "moved", B, rays)
    ds = gpu_lib.scene_create(_fresh_desc(A, rtgpu.RTG_BVH_SAH | REFIT))
    try:
        cam = rtgpu.camera(**CAM)
        job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, rtgpu.RTG_RENDER_OUT_DEVICE | rtgpu.RTG_RENDER_SCHEDULE(5), None)
        gpu_lib.check("rtg_scene_prepare", gpu_lib.lib.rtg_scene_prepare(ds.handle, C.byref(cam), C.byref(job)))
        ds.update(None, B)
        _same(ds, rays, want, 5)
    finally:
        ds.close()


@pytest.mark.gpu
def test_render_sees_the_update(gpu_lib):
    cam = rtgpu.camera(**CAM)
    fresh = gpu_lib.scene_create(_fresh_desc(B))
    want, _ = fresh.render_host(cam)
    fresh.close()
    ds = gpu_lib.scene_create(_fresh_desc(A, rtgpu.RTG_BVH_SAH | REFIT))
    before, _ = ds.render_host(cam)
    ds.update(None, B)
    got, _ = ds.render_host(cam)
    ds.close()
    assert not np.array_equal(before, want) and np.array_equal(got, want)


@pytest.mark.gpu
def test_steady_state_updates_allocate_nothing(gpu_lib):
    idx, P = _partial(65)
    ds = gpu_lib.scene_create(_fresh_desc(A, rtgpu.RTG_BVH_SAH | REFIT))
    ds.update(idx, P[idx])
    ds.update(idx, P[idx])
    n0 = gpu_lib.allocation_count()
    ds.update(idx, P[idx])
    n1 = gpu_lib.allocation_count()
    ds.close()
    assert n0 == n1


@pytest.mark.gpu
def test_update_errors_on_a_scene(gpu_lib):
    """RTG_E_UNSUPPORTED without the bit; a degenerate triangle: host pointers change nothing, device pointers leave
    that primitive out, apply the rest and report it."""
    import torch

    frozen = gpu_lib.scene_create(_fresh_desc(A))
    with pytest.raises(rtgpu.RtgError) as e:
        frozen.update(None, B)
    frozen.close()
    assert e.value.status == rtgpu.RTG_E_UNSUPPORTED
    idx, P = _partial(64)
    tri = int(idx[np.flatnonzero(KINDS[idx] == TRI)[0]])
    bad = P.copy()
    bad[tri, 8:11] = 2 * bad[tri, 4:7]  # v = 2 u
    rays = _ray_set(B)
    ds = gpu_lib.scene_create(_fresh_desc(A, rtgpu.RTG_BVH_SAH | REFIT))
    try:
        with pytest.raises(rtgpu.RtgError) as e:
            ds.update(idx, bad[idx])
        assert e.value.status == rtgpu.RTG_E_INVALID and "degenerate" in str(e.value)
        _same(ds, rays, _fresh(gpu_lib, "base", A, rays))
        d_idx, d_p = torch.from_numpy(idx).cuda(), torch.from_numpy(np.ascontiguousarray(bad[idx])).cuda()
        torch.cuda.synchronize()
        u = rtgpu.rtg_update_desc(d_idx.data_ptr(), d_p.data_ptr(), len(idx), rtgpu.RTG_UPDATE_DEVICE, None)
        st = rtgpu.rtg_update_stats()
        assert gpu_lib.lib.rtg_scene_update(ds.handle, C.byref(u), C.byref(st)) == rtgpu.RTG_E_INVALID
        assert st.invalid == 1 and st.updated == 63
        P[tri] = A[tri]
        _same(ds, rays, _fresh(gpu_lib, "all but the degenerate one", P, rays))
    finally:
        ds.close()


# ---- host tests (no GPU) ----
def test_update_struct_sizes_match_the_header(tmp_path):
    names = ["rtg_prim_update", "rtg_update_desc", "rtg_update_stats"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rtgpu.h"\nint main(void) {\n' +
                   "".join(f'printf("%zu\\n", sizeof({n}));\n' for n in names) + "return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "sizes")], check=True)
    got = subprocess.run([str(tmp_path / "sizes")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(g) for g in got] == [C.sizeof(getattr(rtgpu, n)) for n in names]
    assert C.sizeof(rtgpu.rtg_prim_update) == 48 == np.dtype(rtgpu.UPDATE_DTYPE).itemsize


@pytest.mark.parametrize("case", ["null_desc", "negative", "flags", "null_prims"])
def test_update_rejects_bad_arguments(lib, case):
    """The descriptor is validated before the scene is looked at (rtgpu.h), so a NULL scene reaches these checks."""
    buf = (C.c_char * 64)()
    u = rtgpu.rtg_update_desc(None, None if case == "null_prims" else C.addressof(buf), -1 if case == "negative" else 1,
                              0x2 if case == "flags" else 0, None)
    st = lib.lib.rtg_scene_update(None, None if case == "null_desc" else C.byref(u), None)
    want = {"null_desc": b"null update", "negative": b"count", "flags": b"flags", "null_prims": b"null primitive"}[case]
    assert st == rtgpu.RTG_E_INVALID and want in lib.lib.rtg_last_error()


def test_build_host_ignores_the_refit_bit(lib):
    plain = lib.bvh_build_host(_fresh_desc(A[:64], rtgpu.RTG_BVH_SAH))
    d = _fresh_desc(A[:64], rtgpu.RTG_BVH_SAH | REFIT)
    nodes, refs, depth = lib.bvh_build_host(d)
    assert (len(nodes), list(refs), depth) == (len(plain[0]), list(plain[1]), plain[2])
    d.bvh_mode = rtgpu.RTG_BVH_SAH | 0x200
    assert lib.lib.rtg_bvh_build_host(C.byref(d), None, 0, None, 0, None, None, None) == rtgpu.RTG_E_INVALID
