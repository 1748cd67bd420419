"""rtg_closest_point (DESIGN.md §3 "Proximity queries", §4 "Proximity semantics"): batched nearest-surface queries
against a float64 brute force over all (point, primitive) pairs, across trees, schedules, stacks and updates."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtgpu
from test_gpu import _desc
from test_triangles import QUAD, SKEW, SPHERE, TRI
from test_update import A, B, BIG, KINDS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAREST, REFIT = rtgpu.RTG_BVH_NEAREST, rtgpu.RTG_BVH_REFIT
CONFIGS = [(rtgpu.RTG_BVH_MEDIAN, 0), (rtgpu.RTG_BVH_MEDIAN, 4), (rtgpu.RTG_BVH_SAH, 0), (rtgpu.RTG_BVH_SAH, 3),
           (rtgpu.RTG_BVH_SAH, 4), (rtgpu.RTG_BVH_GPU, 0), (rtgpu.RTG_BVH_GPU, 4)]
N_POINTS = 4096
# Bounds (relative to S, the largest |coordinate| among the case's points and vertices): four times the largest
# error of the first MI355X run against the float64 reference below, capped at 2e-6 S and 2e-5 S.
# Measured maxima (the same in all seven configurations; DESIGN.md §4 "Proximity semantics"): grid dist 9.83e-8 S,
# point 5.74e-8 S; skew dist 1.37e-7 S, point 1.98e-8 S.
DIST_REL = {"grid": min(4 * 9.83e-8, 2e-6), "skew": min(4 * 1.37e-7, 2e-6)}
POINT_REL = {"grid": min(4 * 5.74e-8, 2e-5), "skew": min(4 * 1.98e-8, 2e-5)}


def _skew_prims():
    """SKEW, eight 1:100 sliver triangles above it, then triangle 1 once more (exact ties): (n, 12) float32 rows."""
    rng = np.random.default_rng(11)
    rows = [(k, *Q, r, *u, 0, *v, 0) for k, Q, u, v, r in SKEW]
    for _ in range(8):
        base = rng.normal(size=3)
        base *= 10 / np.linalg.norm(base)
        perp = np.cross(base, rng.normal(size=3))
        perp *= 0.1 / np.linalg.norm(perp)  # height 0.1 over a base of 10
        rows.append((TRI, *rng.uniform(-8, 8, 2), rng.uniform(2, 8), 0, *base, 0, *(rng.uniform(0.2, 0.8) * base + perp), 0))
    rows.append(rows[1])
    rows = np.array(rows, np.float64)
    return rows[:, 0].astype(int), rows[:, 1:].astype(np.float32)


SKEW_KINDS, SKEW_P = _skew_prims()
SLIVERS, DUP = np.arange(len(SKEW), len(SKEW) + 8), len(SKEW) + 8
SCENES = {"grid": (KINDS, A), "skew": (SKEW_KINDS, SKEW_P)}


def _scene_desc(kinds, P, bvh):
    d = _desc([rtgpu.rtg_primitive(kind=int(k), material=0, p0=rtgpu.D3(*map(float, p[0:3])), p1=rtgpu.D3(*map(float, p[4:7])),
                                   p2=rtgpu.D3(*map(float, p[8:11])), radius=float(p[3])) for k, p in zip(kinds, P)],
              [rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=0)],
              [rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(1, 1, 1))])
    d.bvh_mode = bvh
    return d


# ---- the float64 reference: every (point, primitive) pair ----
def _closest(kind, row, p):
    """(distance, closest point, signed offset for `side`, (a, b)) of points p (n, 3) to one primitive, in float64."""
    Q, u, v, r = row[0:3], row[4:7], row[8:11], abs(row[3])
    if kind == SPHERE:
        d = p - Q
        ln = np.linalg.norm(d, axis=1)
        return np.abs(ln - r), Q + r * d / ln[:, None], ln - r, np.zeros((len(p), 2))
    hp = p - Q
    uu, uv, vv = u @ u, u @ v, v @ v
    a, b = np.linalg.solve([[uu, uv], [uv, vv]], [hp @ u, hp @ v])
    inside = (a >= 0) & (b >= 0) & ((a + b <= 1) if kind == TRI else ((a <= 1) & (b <= 1)))
    best = np.where(inside, 0.0, np.inf)  # of the in-plane part; the clamped edge projections compete outside
    ab = np.stack([a, b], 1)
    far = [((1, 0), (-1, 1))] if kind == TRI else [((0, 1), (1, 0)), ((1, 0), (0, 1))]
    for (a0, b0), (da, db) in [((0, 0), (1, 0)), ((0, 0), (0, 1))] + far:
        e = da * u + db * v
        t = np.clip(((hp - a0 * u - b0 * v) @ e) / (e @ e), 0, 1)
        cand = np.stack([a0 + t * da, b0 + t * db], 1)
        dist = np.linalg.norm(hp - cand[:, :1] * u - cand[:, 1:] * v, axis=1)
        take = ~inside & (dist < best)
        best, ab = np.where(take, dist, best), np.where(take[:, None], cand, ab)
    pt = Q + ab[:, :1] * u + ab[:, 1:] * v
    n = np.cross(u, v)
    return np.linalg.norm(p - pt, axis=1), pt, hp @ n / np.linalg.norm(n), ab


_CASES = {}


def _case(name):
    """(kinds, P64, points, D, S) of a scene: 4096 points of POINT_DTYPE from a fixed seed, the float64 distance of
    every pair (prims x points), and the conditions on the reference alone, before any GPU work."""
    if name in _CASES:
        return _CASES[name]
    kinds, P32 = SCENES[name]
    P = P32.astype(np.float64)
    rng = np.random.default_rng(29)
    q = N_POINTS // 4
    small = np.arange(len(P)) != (BIG if name == "grid" else -1)
    edge = np.where((kinds == SPHERE)[:, None], 0.0, P[:, 4:7])  # (a sphere's second point is its centre again)
    verts = np.vstack([P[small][:, 0:3], P[small][:, 0:3] + edge[small], P[small][:, 0:3] + P[small][:, 8:11]])
    lo, hi = verts.min(axis=0) - 3, verts.max(axis=0) + 3

    def surface(n):  # a random primitive's surface point
        k = rng.integers(0, len(P), n)
        a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        fold = (kinds[k] == TRI) & (a + b > 1)
        a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
        corner = rng.uniform(size=n) < 0.25  # exactly on a vertex
        a, b = np.where(corner, np.round(a), a), np.where(corner, np.round(b) * (1 - np.round(a) * (kinds[k] == TRI)), b)
        dirs = rng.normal(size=(n, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        flat = P[k, 0:3] + a[:, None] * P[k, 4:7] + b[:, None] * P[k, 8:11]
        return np.where((kinds[k] == SPHERE)[:, None], P[k, 0:3] + np.abs(P[k, 3:4]) * dirs, flat), dirs

    near, dirs = surface(q)
    pts = np.vstack([rng.uniform(lo, hi, (q, 3)), rng.uniform(-60, 60, (q, 3)),
                     near + dirs * rng.uniform(0.005, 0.05, (q, 1)), surface(q)[0]]).astype(np.float32)
    p = pts.astype(np.float64)
    D = np.stack([_closest(int(k), row, p)[0] for k, row in zip(kinds, P)])
    dmin = D.min(axis=0)
    # the radius: +inf, or 0.5x / 2x the true nearest distance for a random two thirds of the points off the
    # surfaces (half of all points): never within rounding of the answer. The on-surface quarter keeps +inf: at a
    # true distance of 0 or 1e-8 no factor separates the radius from the fp32 answer.
    finite = np.concatenate([rng.uniform(size=3 * q) < 2 / 3, np.zeros(q, bool)])
    radius = np.where(finite, dmin * rng.choice([0.5, 2.0], N_POINTS), np.inf).astype(np.float32)
    points = np.zeros(N_POINTS, dtype=np.dtype(rtgpu.POINT_DTYPE))
    points["p"], points["max_dist"] = pts, radius
    win = np.where(dmin <= radius, D.argmin(axis=0), -1)
    if name == "grid":
        assert all(np.sum((win >= 0) & (win != BIG) & (kinds[win] == k)) >= 64 for k in (SPHERE, QUAD, TRI))
        assert np.sum(win == BIG) >= 16
    else:
        assert np.isin(win, SLIVERS).sum() >= 32 and np.sum(win == 1) >= 16
    assert np.mean(win < 0) >= 0.2
    S = max(np.abs(pts).max(), np.abs(verts).max())
    _CASES[name] = (kinds, P, points, D, S)
    return _CASES[name]


_ANSWERS = {}


def _answers(lib, name, bvh, sched):
    """The records and stats of one configuration, once per session; None where a forced schedule cannot run."""
    key = (name, bvh, sched)
    if key not in _ANSWERS:
        kinds, _, points, _, _ = _case(name)
        ds = lib.scene_create(_scene_desc(kinds, SCENES[name][1], bvh | NEAREST))
        try:
            assert ds.info().bvh_mode == bvh | NEAREST
            _ANSWERS[key] = ds.closest_point(points, schedule=sched)
        except rtgpu.RtgError as e:
            if e.status != rtgpu.RTG_E_UNSUPPORTED or sched == 0:
                raise
            _ANSWERS[key] = None
        finally:
            ds.close()
    return _ANSWERS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("bvh,sched", CONFIGS)
@pytest.mark.parametrize("name", ["grid", "skew"])
def test_matches_float64(gpu_lib, name, bvh, sched):
    kinds, P, points, D, S = _case(name)
    got = _answers(gpu_lib, name, bvh, sched)
    if got is None:
        pytest.skip("the forced schedule cannot run this scene")
    out, st = got
    dist_abs, point_abs = DIST_REL[name] * S, POINT_REL[name] * S
    p, dmin = points["p"].astype(np.float64), D.min(axis=0)
    hit = dmin <= points["max_dist"]
    assert np.array_equal(out["prim"] >= 0, hit)
    assert st.points == N_POINTS and st.found == hit.sum() and st.reserved_[0] in (3, 4)
    miss = out[~hit]
    assert np.all(miss["dist"] == -1) and not miss["point"].any() and not miss["u"].any() and not miss["side"].any()
    rows = np.flatnonzero(hit)
    e_dist = np.abs(out["dist"][rows] - dmin[rows]).max()
    e_win = (D[out["prim"][rows], rows] - dmin[rows]).max()
    e_point = e_uv = 0.0
    for k in np.unique(out["prim"][rows]):
        r = rows[out["prim"][rows] == k]
        _, pt, signed, _ = _closest(int(kinds[k]), P[k], p[r])
        e_point = max(e_point, np.abs(out["point"][r] - pt).max())
        if kinds[k] != SPHERE:
            uvp = P[k, 0:3] + out["u"][r, None] * P[k, 4:7] + out["v"][r, None] * P[k, 8:11]
            e_uv = max(e_uv, np.abs(uvp - out["point"][r]).max())
        sure = np.abs(signed) > dist_abs
        assert np.array_equal(out["side"][r][sure], np.where(signed[sure] > 0, 1, -1))
    print(f"{name} bvh {bvh} schedule {sched} -> {st.reserved_[0]}: dist {e_dist / S:.3g} S, winner {e_win / S:.3g} S, "
          f"point {e_point / S:.3g} S, uv point {e_uv / S:.3g} S (S = {S:.3g}), {st.kernel_ms:.3f} ms")
    assert e_dist <= dist_abs and e_win <= dist_abs
    assert e_point <= point_abs and e_uv <= point_abs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid", "skew"])
def test_trees_and_schedules_agree(gpu_lib, name, monkeypatch):
    kinds, _, points, _, _ = _case(name)
    first = _answers(gpu_lib, name, *CONFIGS[0])[0]
    for cfg in CONFIGS[1:]:
        got = _answers(gpu_lib, name, *cfg)
        assert got is None or np.array_equal(got[0].view(np.uint32), first.view(np.uint32)), cfg
    if name == "skew":
        assert np.sum(first["prim"] == 1) >= 16 and not np.any(first["prim"] == DUP)
    monkeypatch.setenv("RTG_STACK_LDS_ENTRIES", "2")  # knobs are read once per scene: the spill path
    for bvh, sched in [(rtgpu.RTG_BVH_SAH, 0), (rtgpu.RTG_BVH_MEDIAN, 4)]:
        ds = gpu_lib.scene_create(_scene_desc(kinds, SCENES[name][1], bvh | NEAREST))
        out, _ = ds.closest_point(points, schedule=sched)
        ds.close()
        assert np.array_equal(out.view(np.uint32), first.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_point_counts_at_wave_edges(gpu_lib, n):
    kinds, _, points, _, _ = _case("grid")
    full = _answers(gpu_lib, "grid", rtgpu.RTG_BVH_SAH, 0)[0]
    pts, want = np.concatenate([points, points[:1]])[:n].copy(), np.concatenate([full, full[:1]])[:n].copy()
    if n == 65:  # one bad value each: all misses, the neighbours unaffected
        pts["p"][3, 1], pts["max_dist"][17], pts["max_dist"][40], pts["p"][64, 0] = np.nan, -1.0, np.nan, np.inf
        want[[3, 17, 40, 64]] = np.array((-1.0, -1, 0, 0, (0, 0, 0), 0), dtype=want.dtype)
    buf = np.zeros(n + 1, dtype=np.dtype(rtgpu.NEAREST_DTYPE))
    buf.view(np.uint32)[:] = 0x7b7b7b7b
    ds = gpu_lib.scene_create(_scene_desc(kinds, A, rtgpu.RTG_BVH_SAH | NEAREST))
    _, st = ds.closest_point(pts, max_workgroups=1, out=buf[:n])
    ds.close()
    assert st.points == n and (n == 0 or st.reserved_[1] == 1)
    assert np.array_equal(buf[:n].view(np.uint32), want.view(np.uint32))
    assert np.all(buf[n:].view(np.uint32) == 0x7b7b7b7b)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_updated_scene_answers_as_a_fresh_one(gpu_lib, device):
    points = _case("grid")[2]
    mode = rtgpu.RTG_BVH_SAH | REFIT | NEAREST
    fresh = gpu_lib.scene_create(_scene_desc(KINDS, B, mode))
    want, _ = fresh.closest_point(points)
    fresh.close()
    ds = gpu_lib.scene_create(_scene_desc(KINDS, A, mode))
    try:
        if device:
            import torch

            d_p = torch.from_numpy(B).cuda()
            torch.cuda.synchronize()
            ds.update_device(0, d_p.data_ptr(), len(B))
        else:
            ds.update(None, B)
        assert np.array_equal(ds.closest_point(points)[0].view(np.uint32), want.view(np.uint32))
        idx = np.arange(0, 64, dtype=np.int32)  # a partial update with one degenerate triangle: nothing changes
        bad = A[idx].copy()
        bad[3, 8:11] = 2 * bad[3, 4:7]
        with pytest.raises(rtgpu.RtgError) as e:
            ds.update(idx, bad)
        assert e.value.status == rtgpu.RTG_E_INVALID
        assert np.array_equal(ds.closest_point(points)[0].view(np.uint32), want.view(np.uint32))
    finally:
        ds.close()


@pytest.mark.gpu
def test_errors_and_allocations(gpu_lib):
    points = _case("grid")[2]
    plain = gpu_lib.scene_create(_scene_desc(KINDS, A, rtgpu.RTG_BVH_SAH))
    twin = gpu_lib.scene_create(_scene_desc(KINDS, A, rtgpu.RTG_BVH_SAH))
    with_bit = gpu_lib.scene_create(_scene_desc(KINDS, A, rtgpu.RTG_BVH_SAH | NEAREST))
    no_tris = KINDS != TRI
    flat = gpu_lib.scene_create(_scene_desc(KINDS[no_tris], A[no_tris], rtgpu.RTG_BVH_SAH))
    flat_bit = gpu_lib.scene_create(_scene_desc(KINDS[no_tris], A[no_tris], rtgpu.RTG_BVH_SAH | NEAREST))
    try:
        with pytest.raises(rtgpu.RtgError) as e:
            plain.closest_point(points)
        assert e.value.status == rtgpu.RTG_E_UNSUPPORTED and "RTG_BVH_NEAREST" in str(e.value)
        with pytest.raises(rtgpu.RtgError) as e:
            with_bit.closest_point(points, schedule=5)
        assert e.value.status == rtgpu.RTG_E_UNSUPPORTED
        assert plain.info().device_bytes == twin.info().device_bytes and plain.info().bvh_mode == rtgpu.RTG_BVH_SAH
        assert with_bit.info().device_bytes == plain.info().device_bytes + 48 * int(np.sum(KINDS == TRI))
        assert flat_bit.info().device_bytes == flat.info().device_bytes  # no triangles: nothing for the bit
        out, st = flat.closest_point(points)  # spheres and quads answer without the bit
        assert st.found > 0 and np.array_equal(out.view(np.uint32), flat_bit.closest_point(points)[0].view(np.uint32))
        with_bit.closest_point(points)
        n0 = gpu_lib.allocation_count()
        for _ in range(3):
            with_bit.closest_point(points)
        assert gpu_lib.allocation_count() == n0
    finally:
        for ds in (plain, twin, with_bit, flat, flat_bit):
            ds.close()


# ---- host tests (no GPU) ----
def test_struct_sizes_match_the_header(tmp_path):
    names = ["rtg_point", "rtg_nearest", "rtg_nearest_desc", "rtg_nearest_stats"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rtgpu.h"\nint main(void) {\n' +
                   "".join(f'printf("%zu\\n", sizeof({n}));\n' for n in names) + "return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "sizes")], check=True)
    got = subprocess.run([str(tmp_path / "sizes")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(g) for g in got] == [C.sizeof(getattr(rtgpu, n)) for n in names]
    assert C.sizeof(rtgpu.rtg_point) == 16 == np.dtype(rtgpu.POINT_DTYPE).itemsize
    assert C.sizeof(rtgpu.rtg_nearest) == 32 == np.dtype(rtgpu.NEAREST_DTYPE).itemsize


@pytest.mark.parametrize("case", ["null_desc", "negative", "unknown_flag", "null_arrays"])
def test_closest_point_rejects_bad_arguments(lib, case):
    """The descriptor is validated before the scene is looked at (rtgpu.h), so a NULL scene reaches these checks."""
    buf = (C.c_char * 64)()
    ptr = None if case == "null_arrays" else C.addressof(buf)
    q = rtgpu.rtg_nearest_desc(ptr, None, -1 if case == "negative" else 1, ptr, 0x1 if case == "unknown_flag" else 0, 0, None)
    st = lib.lib.rtg_closest_point(None, None if case == "null_desc" else C.byref(q), None)
    want = {"null_desc": b"null", "negative": b"num_points", "unknown_flag": b"flags", "null_arrays": b"null point"}[case]
    assert st == rtgpu.RTG_E_INVALID and want in lib.lib.rtg_last_error()
