"""RTG_QUERY_SORT (DESIGN.md §3 "Ray sorting"): the coherence key on the host, and sorted queries against the unsorted
ones (bytes), test_query.py's float64 reference (its bounds and its "unsure" rule) and the order the device left."""
import functools

import numpy as np
import pytest

import rtgpu
from test_gpu import _desc
from test_query import N_ABS, T_REL, UV_ABS, _float64_case, _rays, _skew_case
from test_triangles import SPHERE

CHUNK = rtgpu.RTG_QUERY_SORT_CHUNK
BIG = 3 * CHUNK + 17  # four sort workgroups, the last chunk partial
SENTINEL = 0x5A


# ---- the key on the host (no GPU) ----
def _bounce_batch():
    rng = np.random.default_rng(3)
    return _rays(rng.uniform(-10, 10, (4096, 3)).astype(np.float32), rng.normal(size=(4096, 3)).astype(np.float32))


@pytest.mark.parametrize("case", ["camera", "bounce", "invalid", "equal"])
def test_sort_keys_host(lib, case):
    if case == "camera":  # one origin, a 64 x 64 pixel grid: every bit to the direction axes
        jj, ii = np.mgrid[0:64, 0:64]
        d = np.stack([ii.ravel() / 64 - 0.5, jj.ravel() / 64 - 0.5, -np.ones(4096)], axis=1)
        keys, lay = lib.ray_sort_keys_host(_rays(np.broadcast_to(np.float32([13, 2, 3]), (4096, 3)), d.astype(np.float32)), 20.0)
        assert list(lay.bits[:3]) == [0, 0, 0] and sum(lay.bits[3:]) == lay.key_bits and not lay.empty
        assert len(np.unique(keys)) >= 256
    elif case == "bounce":
        # origins and directions all over: after the random rays (which fix the box), 256 rays per origin axis
        # that sweep that coordinate with everything else held; then the same with other directions of the batch
        rays = np.concatenate([_bounce_batch(), np.repeat(_rays(np.float32([[1, -2, 3]]), np.float32([[1, 2, -3]])), 768)])
        for a in range(3):
            rays["origin"][4096 + 256 * a:4352 + 256 * a, a] = np.linspace(-9, 9, 256, dtype=np.float32)
        keys, lay = lib.ray_sort_keys_host(rays, 20.0)
        nd = sum(lay.bits[3:])
        assert min(lay.bits) >= 1 and sum(lay.bits) == lay.key_bits
        for a in range(3):
            k = keys[4096 + 256 * a:4352 + 256 * a].astype(np.int64)
            assert np.all(np.diff(k) >= 0) and len(np.unique(k)) == 1 << lay.bits[a], (a, k)
        other = rays.copy()
        other["dir"][4096:] = rays["dir"][:768]
        keys2, _ = lib.ray_sort_keys_host(other, 20.0)
        assert np.array_equal(keys >> nd, keys2 >> nd) and not np.array_equal(keys, keys2)  # origin bits on top
    elif case == "invalid":
        rays = _bounce_batch()
        bad = np.array([0, 77, 2048, 4095])
        rays["origin"][0, 1], rays["origin"][77, 0], rays["dir"][2048], rays["dir"][4095, 2] = np.nan, 2e30, 0, np.inf
        keys, lay = lib.ray_sort_keys_host(rays, 20.0)
        good, lay_good = lib.ray_sort_keys_host(np.delete(rays, bad), 20.0)
        assert np.all(keys[bad] == (1 << lay.key_bits) - 1) and np.array_equal(np.delete(keys, bad), good)
        assert list(lay.lo) == list(lay_good.lo) and list(lay.hi) == list(lay_good.hi) and list(lay.bits) == list(lay_good.bits)
        keys, lay = lib.ray_sort_keys_host(rays[bad], 20.0)  # nothing to trace: the empty box
        assert lay.empty and np.all(keys == (1 << lay.key_bits) - 1)
    else:
        keys, lay = lib.ray_sort_keys_host(np.repeat(_bounce_batch()[:1], 1000), 20.0)
        assert sum(lay.bits) == 0 and np.all(keys == 0)


# ---- on the GPU: the SKEW scene of test_query.py and its float64 helper's rays, computed once ----
@functools.lru_cache(maxsize=None)
def _skew():
    prims, o32, d32, rng = _skew_case("quad")
    return prims, o32, d32, _float64_case(prims, o32, d32, False, rng, "quad (sorted queries)")


def _scene(gpu_lib, bvh=rtgpu.RTG_BVH_SAH):
    d = _desc([rtgpu.rtg_primitive(kind=kind, material=0, p0=rtgpu.D3(*Q), p1=rtgpu.D3(*u), p2=rtgpu.D3(*v), radius=r)
               for kind, Q, u, v, r in _skew()[0]], [rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=0)],
              [rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(1, 1, 1))])
    d.bvh_mode = bvh
    return gpu_lib.scene_create(d)


def _batch(n):
    """The first n rays of the helper's 4096, repeated as often as n needs; and their indices into the reference."""
    _, o32, d32, _ = _skew()
    idx = np.arange(n) % len(o32)
    return _rays(o32[idx], d32[idx]), idx


def _sentinel(n):
    return np.frombuffer(bytes([SENTINEL]) * (32 * n), dtype=np.dtype(rtgpu.HIT_DTYPE)).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, BIG])
@pytest.mark.parametrize("bvh,sched", [(rtgpu.RTG_BVH_SAH, 0), (rtgpu.RTG_BVH_SAH, 4), (rtgpu.RTG_BVH_SAH, 5),
                                       (rtgpu.RTG_BVH_MEDIAN, 4), (rtgpu.RTG_BVH_GPU, 5)])
def test_sorted_closest_hit(gpu_lib, bvh, sched, n):
    """Every byte of the sorted answer equals the unsorted one's, and it meets the float64 reference."""
    prims, _, _, ref = _skew()
    rays, idx = _batch(n)
    ds = _scene(gpu_lib, bvh)
    plain, st0 = ds.intersect(rays, schedule=sched, hits=_sentinel(n))
    h, st = ds.intersect(rays, schedule=sched, sort=True, hits=_sentinel(n))
    ds.close()
    assert h.tobytes() == plain.tobytes()
    assert (st.rays, st.hits) == (st0.rays, st0.hits) == (n, int((plain["prim"] >= 0).sum()))
    assert st0.reserved_[4] == 0 and st.reserved_[0] == st0.reserved_[0] == (sched or 3)
    assert 0 < st.reserved_[4] <= st.kernel_ms * 1000 + 1  # the sort's microseconds, a part of kernel_ms (rounded)
    keep, hit, best, t1, d = (ref[x][idx] for x in ("keep", "hit", "best", "t1", "d"))
    k, bk = keep & hit, np.maximum(best, 0)
    assert np.array_equal(h["prim"][keep], best[keep])
    assert np.all(h["prim"][keep & ~hit] == -1) and np.all(h["t"][keep & ~hit] == -1)
    n_ref = ref["N"][bk, idx]
    front = np.sum(d * n_ref, axis=1) < 0
    n_ref = np.where(front[:, None], n_ref, -n_ref)
    du = np.abs(h["u"] - ref["U"][bk, idx])
    du = np.where(np.array([p[0] for p in prims])[bk] == SPHERE, np.minimum(du, 1 - du), du)  # a sphere's u is periodic
    err = {"t": np.max(np.abs(h["t"][k] - t1[k]) / t1[k], initial=0), "u": du[k].max(initial=0),
           "v": np.abs(h["v"] - ref["V"][bk, idx])[k].max(initial=0), "normal": np.abs(h["normal"] - n_ref)[k].max(initial=0)}
    print("largest errors", {x: float(e) for x, e in err.items()})
    assert np.array_equal(h["front_face"][k], front[k].astype(np.int32))
    assert err["t"] <= T_REL and err["u"] <= UV_ABS and err["v"] <= UV_ABS and err["normal"] <= N_ABS


@pytest.mark.gpu
def test_the_order_is_a_sort(gpu_lib):
    """What the device left behind: a permutation, the host twin's keys, non-decreasing keys along the permutation
    (an identity "sort" would pass every other test here)."""
    rays, _ = _batch(BIG)
    ds = _scene(gpu_lib)
    assert len(ds.query_last_order()[0]) == 0
    ds.intersect(rays, sort=True)
    perm, keys, lay = ds.query_last_order()
    ds.close()
    host, host_lay = gpu_lib.ray_sort_keys_host(rays, lay.scene_extent)
    assert (lay.chunk, lay.workgroups) == (CHUNK, 4) and lay.scene_extent > 0
    assert list(lay.bits) == list(host_lay.bits) and list(lay.lo) == list(host_lay.lo) and list(lay.hi) == list(host_lay.hi)
    assert np.array_equal(np.sort(perm), np.arange(BIG))
    assert np.array_equal(keys, host)
    assert np.all(np.diff(keys[perm].astype(np.int64)) >= 0) and len(np.unique(keys)) >= 256


@pytest.mark.gpu
@pytest.mark.parametrize("sched", [0, 5])
def test_sorted_any_hit(gpu_lib, sched):
    ref = _skew()[3]
    rays, idx = _batch(BIG)
    ds = _scene(gpu_lib)
    plain, _ = ds.intersect(rays, any_hit=True, schedule=sched)
    a, st = ds.intersect(rays, any_hit=True, schedule=sched, sort=True, hits=_sentinel(BIG))
    ds.close()
    keep = ref["keep"][idx]
    assert np.array_equal(a["prim"] >= 0, plain["prim"] >= 0) and st.hits == int((a["prim"] >= 0).sum())
    assert np.array_equal(a["prim"][keep] >= 0, ref["hit"][idx][keep])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["none", "invalid_mixed", "invalid_only", "identical"])
def test_sorted_edge_batches(gpu_lib, case):
    rays, _ = _batch({"none": 0, "invalid_mixed": CHUNK + 900, "invalid_only": 100, "identical": 8192}[case])
    n = len(rays)
    bad = np.arange(n) if case == "invalid_only" else np.arange(0, n, 37) if case == "invalid_mixed" else np.arange(0)
    rays["origin"][bad[0::3], 0], rays["origin"][bad[1::3], 2], rays["dir"][bad[2::3]] = np.nan, np.inf, 0
    if case == "identical":
        rays[:] = rays[np.flatnonzero(_skew()[3]["hit"])[0]]
    times = np.random.default_rng(9).uniform(0, 1, n).astype(np.float32)
    ds = _scene(gpu_lib)
    if case == "none":  # an empty sorted batch after a sorted one: the last order is then empty too
        ds.intersect(_batch(65)[0], sort=True)
    plain, _ = ds.intersect(rays, times)
    h, st = ds.intersect(rays, times, sort=True, hits=_sentinel(n))
    perm, keys, lay = ds.query_last_order()
    ds.close()
    assert h.tobytes() == plain.tobytes() and st.rays == n and np.all(h["prim"][bad] == -1)
    assert np.array_equal(np.sort(perm), np.arange(n)) and np.all(np.diff(keys[perm].astype(np.int64)) >= 0)
    if case == "identical":
        assert np.all(h["prim"] >= 0) and len(np.unique(keys)) == 1
    if n:
        assert np.all(keys[bad] == (1 << lay.key_bits) - 1) and bool(lay.empty) == (case == "invalid_only")


@pytest.mark.gpu
def test_sorted_device_path_allocates_nothing_in_steady_state(gpu_lib):
    """RTG_QUERY_DEVICE with torch tensors (the box comes from the device pre-pass): the host path's bytes; an async
    sorted query followed by a plain one; the third sorted call of one size allocates nothing."""
    import torch

    rays, _ = _batch(BIG)
    ds = _scene(gpu_lib)
    ref, _ = ds.intersect(rays, sort=True)
    d_rays = torch.from_numpy(rays.view(np.float32).copy()).cuda()
    d_hits = [torch.full((BIG * 8,), 7.0, dtype=torch.float32, device="cuda") for _ in range(4)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ds.intersect_device(d_rays.data_ptr(), BIG, d_hits[0].data_ptr(), stream_ptr=stream.cuda_stream, sort=True)
    perm, keys, lay = ds.query_last_order()
    ds.intersect_device(d_rays.data_ptr(), BIG, d_hits[1].data_ptr(), stream_ptr=stream.cuda_stream, sort=True)
    before = gpu_lib.allocation_count()
    ds.intersect_device(d_rays.data_ptr(), BIG, d_hits[2].data_ptr(), stream_ptr=stream.cuda_stream, sort=True, asynchronous=True)
    ds.intersect_device(d_rays.data_ptr(), BIG, d_hits[3].data_ptr(), stream_ptr=stream.cuda_stream)
    assert gpu_lib.allocation_count() == before
    stream.synchronize()
    ds.close()
    host, host_lay = gpu_lib.ray_sort_keys_host(rays, lay.scene_extent)
    assert np.array_equal(keys, host) and list(lay.lo) == list(host_lay.lo) and list(lay.hi) == list(host_lay.hi)
    assert np.array_equal(np.sort(perm), np.arange(BIG)) and np.all(np.diff(keys[perm].astype(np.int64)) >= 0)
    for h in d_hits:
        assert h.cpu().numpy().tobytes() == ref.tobytes()
