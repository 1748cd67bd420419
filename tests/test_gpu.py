"""Device parity: the HIP kernels (through the C-ABI of librtgpu.so) against the fp32 oracle
(cpu_ref32) on the same seeds. Bar (BASELINE.json north_star): per-pixel RMSE < 1e-3 of the linear
mean framebuffer; in practice the GPU reproduces the oracle bit for bit (since round 3 also on the
textured scenes: the textures' sin / acos / atan2 are fixed fp32 sequences of the spec, not libm)."""
import math
import os
import subprocess

import numpy as np
import pytest

import rtgpu
from conftest import REPO

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-3  # north_star: per-pixel RMSE < 1e-3 with matched seeds


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def compare(gpu_lib, scenes, oracle, name, seed=rtgpu.DEFAULT_SEED, bvh=rtgpu.RTG_BVH_SAH, **cam):
    s = scenes.build(name, rand_seed=1, bvh_mode=bvh, grid=cam.pop("grid", 0))
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    for k, v in cam.items():
        setattr(c, k, v)
    ds = gpu_lib.scene_create(s.desc)
    g, st = ds.render_host(c, seed=seed)
    o, segs = oracle.render_f32(s.desc, c, seed=seed)
    ds.close()
    return g, o, st, segs


def assert_parity(g, o, st, segs, exact_frac=1.0):
    """RMSE < 1e-3 is the north star's bar. Beyond it the GPU implements the oracle's fp32 spec (DESIGN.md
    §4) bit for bit — since round 4 including exact-t ties (the spec's tie rule) — so by default every
    pixel and the segment count must be identical; exact_frac < 1 only where a test says why."""
    assert g.shape == o.shape
    assert np.all(np.isfinite(g))
    e = rmse(g, o)
    assert e < RMSE_TOL, e
    frac = float(np.mean(np.all(g == o, axis=-1)))
    assert frac >= exact_frac, (frac, e)
    if exact_frac >= 1.0:
        assert int(st.segments) == int(segs), (st.segments, segs)
    else:
        assert abs(int(st.segments) - int(segs)) <= max(2, 1e-4 * segs), (st.segments, segs)


def test_book1_config1(gpu_lib, scenes, oracle):
    # BASELINE config 1 geometry: 400x225, 10 spp, depth 10
    g, o, st, segs = compare(gpu_lib, scenes, oracle, "bouncing_spheres", image_width=400,
                             aspect_ratio=16.0 / 9.0, samples_per_pixel=10, max_depth=10)
    assert g.shape == (225, 400, 3)
    assert_parity(g, o, st, segs)
    assert st.samples == 400 * 225 * 10
    assert 2.0 < st.segments / st.samples < 3.2  # 2.55 segments/sample at depth 10


@pytest.mark.parametrize("grid", [13, 14])
def test_lds_scene_with_32bit_stack_codes(gpu_lib, scenes, oracle, grid):
    """Bouncing-sphere grids of half-width 13 and 14 still fit the LDS schedule but their 4-wide trees
    have more than 292 nodes, so node codes (LDS addresses) no longer fit a 16-bit stack entry: the
    schedule keeps 32-bit entries there (and no dual launch); the frame must still match the oracle."""
    g, o, st, segs = compare(gpu_lib, scenes, oracle, "bouncing_spheres", grid=grid, image_width=96,
                             aspect_ratio=16.0 / 9.0, samples_per_pixel=4, max_depth=20)
    assert_parity(g, o, st, segs)


@pytest.mark.parametrize("name,W,spp,depth,exact", [
    ("cornell_box", 96, 16, 50, 1.0),
    ("quads", 64, 8, 50, 1.0),
    ("checkered_spheres", 96, 8, 20, 1.0),
    ("simple_light", 96, 8, 50, 1.0),    # noise texture: the spec's sin (round 3), bit for bit
    ("perlin_sphere", 96, 8, 50, 1.0),
    ("earth", 96, 8, 50, 1.0),           # image texture: the spec's acos / atan2 (round 3)
    ("earth_perlin", 96, 8, 50, 1.0),
])
def test_reference_scenes(gpu_lib, scenes, oracle, name, W, spp, depth, exact):
    g, o, st, segs = compare(gpu_lib, scenes, oracle, name, image_width=W,
                             samples_per_pixel=spp, max_depth=depth)
    assert_parity(g, o, st, segs, exact_frac=exact)


@pytest.mark.parametrize("name,W,spp", [
    ("cornell_box", 64, 16),        # BASELINE config 4's scene at its own depth 100
    ("cornell_translate", 64, 16),  # translate (hittable.hpp:74-117), nested, on quads and a sphere
])
def test_depth100_scenes_match_oracle(gpu_lib, scenes, oracle, name, W, spp):
    g, o, st, segs = compare(gpu_lib, scenes, oracle, name, image_width=W, aspect_ratio=1.0,
                             samples_per_pixel=spp, max_depth=100)
    assert_parity(g, o, st, segs)
    assert st.segments / st.samples > 5.0  # long Cornell paths (6.6 segments/sample)


# G5: the HIP frame against the reference estimator's per-pixel mean
# (tests/golden/moments_*.npz, >= 2048 samples per pixel of the ref-hybrid render from glibc rand()
# streams). GPU samples per pixel: enough that 8x8-block means are gaussian.
G5_GPU = [("book1", 1024), ("cornell", 2048), ("cornell_translate", 2048), ("simple_light", 1024),
          ("perlin", 1024), ("book1_g500", 1024), ("earth_perlin", 1024), ("earth", 1024),
          ("checkered", 1024), ("quads", 1024)]


@pytest.mark.parametrize("scene,spp", G5_GPU)
def test_statistical_parity_vs_reference(gpu_lib, scenes, scene, spp):
    """The GPU's changes to the reference algorithm (fp32, counter RNG, direct sampling of the
    unit sphere / disk, SAH 4-wide BVH, chunked sums, origin rule) leave the expected image
    unchanged: |z| < 4 on >= 99.9 % of 8x8 blocks, chi-square of the block z-scores ~ 1, the
    global channel means within 3 sigma, and the mean path length within 1 %."""
    from golden_stats import MOMENT_SCENES, assert_statistical_parity, moments_camera

    name, grid = MOMENT_SCENES[scene]
    s = scenes.build(name, grid=grid, rand_seed=1)
    cam, m = moments_camera(scene, spp)
    ds = gpu_lib.scene_create(s.desc)
    g, st = ds.render_host(cam, seed=0xB0BA)
    ds.close()
    assert g.shape == m["mean"].shape
    rep = assert_statistical_parity(g, m, spp)
    H, W = g.shape[:2]
    ref_len = float(m["segments"]) / (int(m["n"]) * H * W)
    gpu_len = st.segments / st.samples
    assert abs(gpu_len - ref_len) / ref_len < 0.01, (gpu_len, ref_len, rep)


def test_bvh_mode_does_not_change_the_image(gpu_lib, scenes):
    imgs = []
    for mode in (rtgpu.RTG_BVH_MEDIAN, rtgpu.RTG_BVH_SAH):
        s = scenes.build("bouncing_spheres", rand_seed=1, bvh_mode=mode)
        c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
        c.image_width, c.samples_per_pixel, c.max_depth = 160, 4, 20
        ds = gpu_lib.scene_create(s.desc)
        imgs.append(ds.render_host(c)[0])
        ds.close()
    # the closest hit is order-free, exact-t ties included (the spec's tie rule)
    assert np.array_equal(imgs[0], imgs[1])


def test_schedules_give_identical_frames(gpu_lib, scenes):
    """All kernel schedules (persistent LDS-resident default, plain-grid ballot-batched, the
    treelet) differ only in when a lane's work runs, never in what it computes: identical frames
    and segment counts. The retired per-segment schedules 1 and 2 report RTG_E_UNSUPPORTED."""
    import ctypes as C

    frames, segs = [], []
    for mode, flag_set in (
            (rtgpu.RTG_BVH_MEDIAN, (0, rtgpu.RTG_RENDER_SCHEDULE(3), rtgpu.RTG_RENDER_SCHEDULE(4))),
            (2, (0, rtgpu.RTG_RENDER_SCHEDULE(4))),  # binary SAH
            (rtgpu.RTG_BVH_SAH, (0, rtgpu.RTG_RENDER_SCHEDULE(4), rtgpu.RTG_RENDER_LEAF_BATCH(1),
                                 rtgpu.RTG_RENDER_LEAF_BATCH(64), rtgpu.RTG_RENDER_SHADE_BATCH(1),
                                 rtgpu.RTG_RENDER_SHADE_BATCH(64),
                                 rtgpu.RTG_RENDER_SCHEDULE(4) | rtgpu.RTG_RENDER_SHADE_BATCH(40)))):
        s = scenes.build("bouncing_spheres", rand_seed=1, bvh_mode=mode)
        c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
        c.image_width, c.samples_per_pixel, c.max_depth = 160, 8, 50
        ds = gpu_lib.scene_create(s.desc)
        H = gpu_lib.camera_resolve(c).image_height
        for flags in flag_set:
            out = np.zeros((H, 160, 3), dtype=np.float32)
            job = rtgpu.rtg_render_desc(5, 0, 1, 0, flags, None)
            st = rtgpu.rtg_render_stats()
            gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                                out.ctypes.data, C.byref(st)))
            frames.append(out)
            segs.append(st.segments)
        ds.close()
    # every tree and schedule: bit-identical (the spec's tie rule makes the closest hit order-free)
    assert all(np.array_equal(f, frames[0]) for f in frames)
    assert max(segs) == min(segs)
    s = scenes.build("bouncing_spheres", rand_seed=1, bvh_mode=rtgpu.RTG_BVH_MEDIAN)
    ds = gpu_lib.scene_create(s.desc)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 32, 1, 5
    out = np.zeros((gpu_lib.camera_resolve(c).image_height, 32, 3), dtype=np.float32)
    for sched in (1, 2):
        job = rtgpu.rtg_render_desc(5, 0, 1, 0, rtgpu.RTG_RENDER_SCHEDULE(sched), None)
        assert gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job), out.ctypes.data, None) == \
            rtgpu.RTG_E_UNSUPPORTED
    ds.close()


@pytest.mark.parametrize("name,W,spp,depth", [("cornell_box", 96, 16, 100), ("earth_perlin", 128, 8, 50)])
def test_small_scene_workgroup_shapes(gpu_lib, scenes, oracle, name, W, spp, depth, monkeypatch):
    """Scenes small enough for five copies of scene + stacks per CU run five 4-wave persistent
    workgroups per CU (5 waves per SIMD) instead of one 16-wave one: the work units are the same,
    so the frame and the segment count are identical, and both match the oracle."""
    s = scenes.build(name, rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = W, spp, depth
    out = {}
    for waves in ("4", "16"):
        monkeypatch.setenv("RTG_LDS_WAVES", waves)
        ds = gpu_lib.scene_create(s.desc)
        out[waves] = ds.render_host(c)
        ds.close()
    (g4, st4), (g16, st16) = out["4"], out["16"]
    assert np.array_equal(g4, g16) and st4.segments == st16.segments
    o, segs = oracle.render_f32(s.desc, c)
    assert np.sqrt(np.mean((g4.astype(np.float64) - o) ** 2)) < 1e-3


def test_dual_launch_matches_single(gpu_lib, scenes, monkeypatch):
    """Book-1 is too large for five 4-wave workgroups per CU, so a second persistent launch (one
    4-wave workgroup per CU on an auxiliary stream, beside the 16-wave one) fills the fifth wave slot
    of each SIMD; both launches take units from one counter, so the frame and the segment count are
    those of the single launch (RTG_DUAL=0) and of the plain grid."""
    import ctypes as C

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 240, 24, 50  # 24 spp: two sample chunks
    out = {}
    for dual in ("1", "0"):
        monkeypatch.setenv("RTG_DUAL", dual)
        ds = gpu_lib.scene_create(s.desc)
        out[dual] = ds.render_host(c)
        ds.close()
    monkeypatch.delenv("RTG_DUAL")
    ds = gpu_lib.scene_create(s.desc)
    H = gpu_lib.camera_resolve(c).image_height
    ref = np.zeros((H, 240, 3), dtype=np.float32)
    rst = rtgpu.rtg_render_stats()
    job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, rtgpu.RTG_RENDER_SCHEDULE(4), None)
    gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                        ref.ctypes.data, C.byref(rst)))
    ds.close()
    (g1, st1), (g0, st0) = out["1"], out["0"]
    assert np.array_equal(g1, g0) and st1.segments == st0.segments
    assert np.array_equal(g1, ref) and st1.segments == rst.segments


@pytest.mark.parametrize("grid,W", [(11, 96), (500, 128)])
def test_treelet_schedule_matches_default(gpu_lib, scenes, oracle, grid, W, monkeypatch):
    """Schedule 5 (persistent workgroups, the breadth-first top of the 4-wide tree in LDS, the rest
    and every primitive through the caches; the default for scenes too large for LDS): book-1 (the
    whole tree fits the treelet) and the 1M-sphere scene (the treelet holds the top ~870 of ~330k
    nodes, the stack spills past 16 entries) render the plain grid's (schedule 4) frame and segment
    count; also with 3 LDS stack entries."""
    import ctypes as C

    s = scenes.build("bouncing_spheres", grid=grid, rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.aspect_ratio, c.samples_per_pixel, c.max_depth = W, 16.0 / 9.0, 4, 50
    ds = gpu_lib.scene_create(s.desc)
    H = gpu_lib.camera_resolve(c).image_height
    ref = np.zeros((H, W, 3), dtype=np.float32)
    rst = rtgpu.rtg_render_stats()
    job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, rtgpu.RTG_RENDER_SCHEDULE(4), None)
    gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                        ref.ctypes.data, C.byref(rst)))
    default, dst = ds.render_host(c)
    assert np.array_equal(default, ref) and dst.segments == rst.segments
    for entries in (None, "3"):
        if entries:
            monkeypatch.setenv("RTG_STACK_LDS_ENTRIES", entries)
            ds.close()
            ds = gpu_lib.scene_create(s.desc)  # knobs are read once per scene
        out = np.zeros((H, W, 3), dtype=np.float32)
        job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, rtgpu.RTG_RENDER_SCHEDULE(5), None)
        st = rtgpu.rtg_render_stats()
        gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                            out.ctypes.data, C.byref(st)))
        assert np.array_equal(out, ref) and st.segments == rst.segments, entries
    ds.close()
    o, segs = oracle.render_f32(s.desc, c)
    assert_parity(ref, o, rst, segs)


def test_hot_treelet_keeps_the_frame(gpu_lib, scenes, oracle, monkeypatch):
    """Hot treelet (rtg_scene_prepare): a probe render counts node visits for the camera
    and the node array is renumbered so the most-visited nodes form the LDS prefix of the treelet
    schedule. Same tree, same child slots: the frame and the segment count equal the breadth-first
    treelet's and the plain grid's, bit for bit, on the 1M-sphere scene (whose tree is ~1500x the
    treelet); the plan reports the tuning; a scene that fits LDS (book-1) is left alone."""
    s = scenes.build("bouncing_spheres", grid=500, rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.aspect_ratio, c.samples_per_pixel, c.max_depth = 160, 16.0 / 9.0, 8, 50
    monkeypatch.setenv("RTG_TREELET_HOT", "0")
    ds = gpu_lib.scene_create(s.desc)  # knobs are read once per scene
    monkeypatch.delenv("RTG_TREELET_HOT")
    bfs, bst = ds.render_host(c)
    assert ds.plan(c).treelet_hot == 0
    ds.close()
    ds = gpu_lib.scene_create(s.desc)
    p0 = ds.plan(c)
    assert (p0.schedule, p0.treelet_hot) == (5, 0), p0.as_dict()
    ds.prepare(c)
    p1 = ds.plan(c)
    assert p1.treelet_hot == 1 and p1.treelet_tune_us > 0, p1.as_dict()
    assert 500 < p1.treelet_visit_permille <= 1000, p1.as_dict()  # the LDS prefix takes most visits
    hot, hst = ds.render_host(c)
    assert np.array_equal(hot, bfs) and hst.segments == bst.segments
    # another camera is not the tuned one; its renders keep the tuned order (no probe inside
    # rtg_render after the scene's first tuning) until rtg_scene_prepare re-tunes
    c2 = rtgpu.rtg_camera_desc.from_buffer_copy(c)
    c2.lookfrom[0] += 3.0
    assert ds.plan(c2).treelet_hot == 0
    hot2, st2 = ds.render_host(c2)
    assert ds.plan(c2).treelet_hot == 0 and ds.plan(c).treelet_hot == 1
    ds.prepare(c2)
    assert ds.plan(c2).treelet_hot == 1 and ds.plan(c).treelet_hot == 0
    hot3, st3 = ds.render_host(c2)
    assert np.array_equal(hot3, hot2) and st3.segments == st2.segments
    ds.close()
    o, segs = oracle.render_f32(s.desc, c2)
    assert_parity(hot2, o, st2, segs)
    # a fresh scene's first render tunes implicitly
    ds = gpu_lib.scene_create(s.desc)
    ds.render_host(c2)
    assert ds.plan(c2).treelet_hot == 1
    ds.close()
    b = scenes.build("bouncing_spheres", grid=11, rand_seed=1)
    cb = rtgpu.rtg_camera_desc.from_buffer_copy(b.camera)
    cb.image_width, cb.samples_per_pixel = 96, 4
    db = gpu_lib.scene_create(b.desc)
    db.prepare(cb)
    pb = db.plan(cb)
    db.close()
    assert pb.schedule == 3 and pb.treelet_hot == 0 and pb.treelet_tune_us == 0


def test_tile_order_keeps_the_frame(gpu_lib, scenes, oracle, monkeypatch):
    """Cost-ordered tile hand-out (rtg_scene_prepare, DESIGN.md §3 "tile order"): a probe render counts each
    tile's segments for the camera and shard, and later renders of that camera and shard hand the tiles out
    most expensive first. Only when a unit is rendered changes: frames and segment counts equal the tile-major
    render's, bit for bit, on book-1 (LDS schedule, two sample chunks), a strided shard of it and Cornell (five
    4-wave workgroups); another camera or shard, the treelet schedule (1M spheres), the tile-ring kernels and
    RTG_TILE_ORDER=0 keep tile-major order."""
    b = scenes.build("bouncing_spheres", grid=11, rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(b.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 192, 32, 50
    ds = gpu_lib.scene_create(b.desc)
    f0, st0 = ds.render_host(c)
    assert st0.tile_order == 0
    ds.prepare(c)
    f1, st1 = ds.render_host(c)
    assert st1.tile_order == 1 and st1.tile_order_tune_us > 0
    assert np.array_equal(f1, f0) and st1.segments == st0.segments
    o, segs = oracle.render_f32(b.desc, c)
    assert_parity(f1, o, st1, segs)
    # the counting kernel reads the order where the product kernels do (from the kernel arguments) and
    # reports a mismatch with its DevJob as a corrupt render
    _, cst = ds.render_host(c, count=True)
    assert cst.tile_order == 1 and cst.segments == st0.segments
    # a strided shard is another tile layout: tile-major until prepared for it, then ordered, same rows
    s0, sst0 = ds.render_host(c, row_begin=1, row_stride=3)
    assert sst0.tile_order == 0
    ds.prepare(c, row_begin=1, row_stride=3)
    s1, sst1 = ds.render_host(c, row_begin=1, row_stride=3)
    assert sst1.tile_order == 1 and np.array_equal(s1, s0) and sst1.segments == sst0.segments
    assert np.array_equal(s1, f0[1::3])
    _, st2 = ds.render_host(c)  # the scene keeps one order: the full frame's was replaced
    assert st2.tile_order == 0
    # the tile-ring kernels keep tile-major order (their slot hand-off needs it)
    ds.close()
    monkeypatch.setenv("RTG_TILE_SLOTS", "8")
    dr = gpu_lib.scene_create(b.desc)
    monkeypatch.delenv("RTG_TILE_SLOTS")
    dr.prepare(c)
    fr, str_ = dr.render_host(c)
    dr.close()
    assert str_.tile_order == 0 and np.array_equal(fr, f0)
    monkeypatch.setenv("RTG_TILE_ORDER", "0")
    dk = gpu_lib.scene_create(b.desc)
    monkeypatch.delenv("RTG_TILE_ORDER")
    dk.prepare(c)
    fk, stk = dk.render_host(c)
    dk.close()
    assert stk.tile_order == 0 and np.array_equal(fk, f0)
    # the treelet schedule reads nodes and primitives through the caches, where tile-major order keeps a CU's
    # waves on neighbouring pixels: rtg_scene_prepare tunes its hot treelet and leaves the hand-out alone
    g = scenes.build("bouncing_spheres", grid=500, rand_seed=1)
    cg = rtgpu.rtg_camera_desc.from_buffer_copy(g.camera)
    cg.image_width, cg.aspect_ratio, cg.samples_per_pixel, cg.max_depth = 160, 16.0 / 9.0, 20, 50
    dg = gpu_lib.scene_create(g.desc)
    g0, gst0 = dg.render_host(cg)  # the first render tunes the hot treelet only
    assert gst0.tile_order == 0 and dg.plan(cg).treelet_hot == 1
    dg.prepare(cg)
    g1, gst1 = dg.render_host(cg)
    dg.close()
    assert gst1.tile_order == 0 and np.array_equal(g1, g0) and gst1.segments == gst0.segments
    # Cornell: five 4-wave workgroups per CU
    k = scenes.build("cornell_box", rand_seed=1)
    ck = rtgpu.rtg_camera_desc.from_buffer_copy(k.camera)
    ck.image_width, ck.samples_per_pixel, ck.max_depth = 96, 24, 100
    dc = gpu_lib.scene_create(k.desc)
    k0, kst0 = dc.render_host(ck)
    dc.prepare(ck)
    k1, kst1 = dc.render_host(ck)
    dc.close()
    assert kst1.tile_order == 1 and np.array_equal(k1, k0) and kst1.segments == kst0.segments


def test_repeated_host_renders_are_identical(gpu_lib, scenes):
    """Host-output renders go through a scene-owned device frame and a pinned staging buffer; with
    a stream-ordered (hipMallocAsync) frame the third render of a scene came back all zero."""
    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 96, 4, 20
    ds = gpu_lib.scene_create(s.desc)
    frames = [ds.render_host(c, count=bool(k % 2))[0] for k in range(5)]
    ds.close()
    assert float(frames[0].sum()) > 0.0
    assert all(np.array_equal(f, frames[0]) for f in frames[1:])


def test_shards_and_determinism(gpu_lib, scenes):
    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 200, 4, 50
    ds = gpu_lib.scene_create(s.desc)
    full, st = ds.render_host(c, seed=99)
    again, _ = ds.render_host(c, seed=99)
    assert np.array_equal(full, again)
    H = full.shape[0]
    for world in (2, 3, 8):
        shards = []
        for r in range(world):
            b, stride, n = rtgpu.shard_rows(H, r, world)
            shards.append(ds.render_host(c, seed=99, row_begin=b, row_stride=stride, row_count=n)[0])
        assert np.array_equal(rtgpu.deinterleave(shards, H), full)
    other, _ = ds.render_host(c, seed=100)
    assert not np.array_equal(other, full)
    # several sample chunks per pixel and the strided shards' 16x4 tiles: still bit-identical
    c.image_width, c.samples_per_pixel = 96, 40
    full, _ = ds.render_host(c, seed=5)
    H = full.shape[0]
    for world in (2, 8):
        shards = [ds.render_host(c, seed=5, row_begin=b, row_stride=stride, row_count=n)[0]
                  for b, stride, n in (rtgpu.shard_rows(H, r, world) for r in range(world))]
        assert np.array_equal(rtgpu.deinterleave(shards, H), full)
    ds.close()


@pytest.mark.parametrize("spp", [17, 65, 200])
def test_sample_chunks_match_oracle(gpu_lib, scenes, oracle, spp):
    """Above 16 spp a pixel's samples are accumulated in chunks (rtgpu.h rtg_chunk_samples) that the
    device renders as separate work units and combines in chunk order: bit-identical to cpu_ref32."""
    g, o, st, segs = compare(gpu_lib, scenes, oracle, "bouncing_spheres", image_width=48,
                             samples_per_pixel=spp, max_depth=20)
    assert rtgpu.chunk_samples(spp) < spp
    assert_parity(g, o, st, segs)
    gs, _, _, _ = compare(gpu_lib, scenes, oracle, "bouncing_spheres", image_width=48,
                          samples_per_pixel=spp, max_depth=20)
    assert np.array_equal(g, gs)  # deterministic whatever order the units ran in


@pytest.mark.parametrize("name,W,spp,schedule", [
    ("bouncing_spheres", 240, 40, 3), ("cornell_box", 96, 64, 3), ("bouncing_spheres", 160, 40, 5)])
def test_tile_ring_matches_full_frame_partials(gpu_lib, scenes, name, W, spp, schedule, monkeypatch):
    """One-shot chunked frames can sum each tile's chunks in chunk order in the wave whose batch of the
    tile finished last, through a ring of tile slots (DESIGN.md §4 "per-tile combine"; the default
    above 32 GiB of full-frame partials). The frame and the segment count must be those of the
    full-frame partial buffers + combine kernel (RTG_TILE_SLOTS=0) for a ring with a slot per tile
    and for rings of 1, 2 and 8 slots, where nearly every batch finds its slot still owned by an
    earlier tile and waits (book-1: the dual launch; Cornell: 4-wave workgroups; schedule 5: the
    treelet kernel)."""
    import ctypes as C

    s = scenes.build(name, rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = W, spp, 50
    assert rtgpu.num_chunks(spp) >= 3
    H = gpu_lib.camera_resolve(c).image_height
    out = {}
    for slots in ("0", "1", "2", "8", "65536", None):
        if slots is None:
            monkeypatch.delenv("RTG_TILE_SLOTS", raising=False)
        else:
            monkeypatch.setenv("RTG_TILE_SLOTS", slots)
        ds = gpu_lib.scene_create(s.desc)
        p = ds.plan(c)
        assert p.chunks >= 3
        if p.tile_slots:  # the ring and its slot words
            assert p.partial_bytes == p.tile_slots * (p.chunks * 1024 + 8)
        else:  # full-frame [chunk][row][column][3] partials
            assert p.partial_bytes == H * W * 12 * p.chunks
        if slots == "65536":  # more slots than tiles: one slot per tile (the ring never waits)
            tiles = -(-W // 8) * -(-H // 8)
            assert tiles <= p.tile_slots < 2 * tiles
        elif slots is None:  # small frames keep the full-frame partials by default
            assert p.tile_slots == 0
        else:
            assert p.tile_slots == int(slots)
        frame = np.zeros((H, W, 3), dtype=np.float32)
        st = rtgpu.rtg_render_stats()
        job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, rtgpu.RTG_RENDER_SCHEDULE(schedule), None)
        gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                            frame.ctypes.data, C.byref(st)))
        ds.close()
        out[slots] = (frame, st.segments)
    ref, ref_segs = out.pop("0")
    assert float(ref.sum()) > 0.0
    for slots, (frame, segs) in out.items():
        assert np.array_equal(frame, ref) and segs == ref_segs, slots


@pytest.mark.parametrize("schedule", [3, 5])
@pytest.mark.parametrize("world", [3, 8])
def test_tile_ring_on_strided_shards(gpu_lib, scenes, schedule, world, monkeypatch):
    """The ring's tile -> pixel mapping for row-interleaved shards (row_stride > 1: 16x4 tiles,
    tile_lw 4 — the layout of multi-rank renders): every rank's shard through rings of 1
    and 8 slots equals the same shard through the full-frame partials, pixel for pixel and segment for
    segment."""
    import ctypes as C

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 136, 40, 30
    H = gpu_lib.camera_resolve(c).image_height
    W = c.image_width
    for r in range(world):
        b, stride, n = rtgpu.shard_rows(H, r, world)
        out = {}
        for slots in ("0", "1", "8"):
            monkeypatch.setenv("RTG_TILE_SLOTS", slots)
            ds = gpu_lib.scene_create(s.desc)
            p = ds.plan(c, row_begin=b, row_stride=stride, row_count=n)
            assert p.tile_slots == int(slots), p.as_dict()
            frame = np.zeros((n, W, 3), dtype=np.float32)
            st = rtgpu.rtg_render_stats()
            job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, b, stride, n, rtgpu.RTG_RENDER_SCHEDULE(schedule), None)
            gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                                frame.ctypes.data, C.byref(st)))
            ds.close()
            out[slots] = (frame, st.segments)
        ref, ref_segs = out.pop("0")
        assert float(ref.sum()) > 0.0
        for slots, (frame, segs) in out.items():
            assert np.array_equal(frame, ref) and segs == ref_segs, (r, slots)


def test_tile_ring_bounds_fall_back_to_full_frame(gpu_lib, scenes):
    """The ring kernels index the shard's frame with 32-bit byte offsets: a shard of >= 2 GiB (here
    18432 x 10368 px x 12 B) keeps the full-frame partials even where the ring would be the default
    (above 32 GiB of partials); just below the bound the ring is chosen (plans only, nothing rendered)."""
    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.samples_per_pixel, c.max_depth = 1000, 50
    ds = gpu_lib.scene_create(s.desc)
    c.image_width = 18432
    H = gpu_lib.camera_resolve(c).image_height
    p = ds.plan(c)
    assert H * 18432 * 12 >= 1 << 31 and p.tile_slots == 0 and p.partial_bytes == H * 18432 * 12 * p.chunks
    c.image_width = 12288  # 12288 x 6912 x 12 B < 2 GiB
    H = gpu_lib.camera_resolve(c).image_height
    p = ds.plan(c)
    assert H * 12288 * 12 < 1 << 31 and p.tile_slots > 0, p.as_dict()
    ds.close()


def test_progressive_chunks_and_checkpoint(gpu_lib, scenes):
    """Progressive rendering (rtg_render_desc.partial): chunks rendered in several calls, with a
    checkpoint (partial sums copied to the host, the scene destroyed and rebuilt) in between,
    reproduce the one-shot frame bit for bit; the running mean uses the samples done so far."""
    import torch

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 80, 60, 20
    n = rtgpu.num_chunks(60)
    K = rtgpu.chunk_samples(60)
    assert (n, K) == (4, 15)
    ds = gpu_lib.scene_create(s.desc)
    full, _ = ds.render_host(c, seed=7)
    H = full.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    partial = torch.zeros((n, H, 80, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, 80, 3), dtype=torch.float32, device="cuda")
    st = ds.render_chunks(c, partial.data_ptr(), 0, 1, out.data_ptr(), stream, seed=7)
    torch.cuda.synchronize()
    assert st.samples == H * 80 * K
    first = partial[0].cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), np.float32(1.0 / K) * first)
    ds.render_chunks(c, partial.data_ptr(), 1, 2, 0, stream, seed=7)
    torch.cuda.synchronize()
    saved = partial.cpu()  # checkpoint
    ds.close()
    ds = gpu_lib.scene_create(s.desc)
    ds.prepare(c)  # the resumed chunks in the prepared tile order: the same sums
    resumed = saved.cuda()
    st = ds.render_chunks(c, resumed.data_ptr(), 3, 0, out.data_ptr(), stream, seed=7)
    torch.cuda.synchronize()
    assert st.tile_order == 1
    assert np.array_equal(out.cpu().numpy(), full)
    assert np.array_equal(resumed[:3].cpu().numpy(), saved[:3].numpy())  # finished chunks untouched
    ds.close()


@pytest.mark.parametrize("case", ["one_pixel", "odd_width", "depth0", "depth0_chunked", "depth1", "spp1",
                                  "pinhole", "tall"])
def test_edge_cases(gpu_lib, scenes, oracle, case):
    kw = dict(image_width=33, samples_per_pixel=3, max_depth=10)
    if case == "one_pixel":
        kw.update(image_width=1, aspect_ratio=1.0)
    elif case == "odd_width":
        kw.update(image_width=17, aspect_ratio=17 / 5)
    elif case == "depth0":
        kw.update(max_depth=0)
    elif case == "depth0_chunked":  # black frame written by rtg_render (no kernel), 3 sample chunks
        kw.update(max_depth=0, samples_per_pixel=40)
    elif case == "depth1":
        kw.update(max_depth=1)
    elif case == "spp1":
        kw.update(samples_per_pixel=1)
    elif case == "pinhole":
        kw.update(defocus_angle=0.0)
    elif case == "tall":
        kw.update(image_width=9, aspect_ratio=0.25)
    g, o, st, segs = compare(gpu_lib, scenes, oracle, "bouncing_spheres", **kw)
    assert_parity(g, o, st, segs)
    if case.startswith("depth0"):
        assert st.segments == 0 and not g.any()


def _desc(prims, materials, textures):
    import ctypes as C

    P = (rtgpu.rtg_primitive * max(1, len(prims)))(*prims)
    M = (rtgpu.rtg_material * max(1, len(materials)))(*materials)
    T = (rtgpu.rtg_texture * max(1, len(textures)))(*textures)
    d = rtgpu.rtg_scene_desc(abi_version=rtgpu.RTG_ABI_VERSION, bvh_mode=rtgpu.RTG_BVH_SAH,
                             prims=C.cast(P, C.POINTER(rtgpu.rtg_primitive)), num_prims=len(prims),
                             materials=C.cast(M, C.POINTER(rtgpu.rtg_material)),
                             num_materials=len(materials),
                             textures=C.cast(T, C.POINTER(rtgpu.rtg_texture)),
                             num_textures=len(textures))
    d._keep = (P, M, T)
    return d


def test_empty_world_and_single_sphere(gpu_lib, oracle):
    cam = rtgpu.camera(image_width=24, aspect_ratio=1.5, samples_per_pixel=4, max_depth=8,
                       background=(0.7, 0.8, 1.0), lookfrom=(0, 0, 3), lookat=(0, 0, 0))
    empty = _desc([], [], [])
    ds = gpu_lib.scene_create(empty)
    g, st = ds.render_host(cam)
    o, segs = oracle.render_f32(empty, cam)
    assert np.array_equal(g, o) and st.segments == segs == 24 * 16 * 4
    tex = rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(0.5, 0.2, 0.1))
    mat = rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=0)
    sph = rtgpu.rtg_primitive(kind=rtgpu.RTG_PRIM_SPHERE, material=0, p0=rtgpu.D3(0, 0, 0),
                              p1=rtgpu.D3(0, 0, 0), radius=1.0)
    one = _desc([sph], [mat], [tex])
    ds = gpu_lib.scene_create(one)
    g, st = ds.render_host(cam)
    o, segs = oracle.render_f32(one, cam)
    assert_parity(g, o, st, segs)


@pytest.mark.parametrize("bvh", [rtgpu.RTG_BVH_SAH, rtgpu.RTG_BVH_GPU, rtgpu.RTG_BVH_MEDIAN])
def test_ground_and_one_sphere(gpu_lib, oracle, bvh):
    """A ground sphere and one small sphere: the ground becomes the scene-spanning occluder in the
    4-wide modes, leaving a one-primitive tree (the device builder's n = 1 case)."""
    cam = rtgpu.camera(image_width=32, aspect_ratio=1.5, samples_per_pixel=4, max_depth=8,
                       background=(0.7, 0.8, 1.0), lookfrom=(0, 1, 4), lookat=(0, 0.5, 0))
    tex = rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(0.5, 0.2, 0.1))
    mat = rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=0)
    ground = rtgpu.rtg_primitive(kind=rtgpu.RTG_PRIM_SPHERE, material=0, p0=rtgpu.D3(0, -1000, 0),
                                 p1=rtgpu.D3(0, -1000, 0), radius=1000.0)
    ball = rtgpu.rtg_primitive(kind=rtgpu.RTG_PRIM_SPHERE, material=0, p0=rtgpu.D3(0, 0.5, 0),
                               p1=rtgpu.D3(0, 0.5, 0), radius=0.5)
    d = _desc([ground, ball], [mat], [tex])
    d.bvh_mode = bvh
    ds = gpu_lib.scene_create(d)
    if bvh != rtgpu.RTG_BVH_MEDIAN:
        # the occluder heuristic really left a one-primitive tree: one (leaf-only) 4-wide node
        assert ds.info().num_nodes == 1, ds.info().num_nodes
    g, st = ds.render_host(cam)
    ds.close()
    o, segs = oracle.render_f32(d, cam)
    assert_parity(g, o, st, segs)
    assert st.segments > 32 * 21 * 4  # rays bounce between the ball and the ground
    if bvh != rtgpu.RTG_BVH_MEDIAN:  # without the occluder: a two-primitive tree, the same frame
        os.environ["RTG_NO_OCCLUDER"] = "1"
        try:
            ds = gpu_lib.scene_create(d)
            g2, st2 = ds.render_host(cam)
            ds.close()
        finally:
            del os.environ["RTG_NO_OCCLUDER"]
        assert np.array_equal(g, g2) and st2.segments == st.segments


@pytest.mark.parametrize("tables,schedule", [(3, 3), (17, 5)])
def test_perlin_tables_match_oracle(gpu_lib, oracle, tables, schedule):
    """Noise textures on several perlin tables (perlin.hpp:95-158; the device's packed permutation words,
    rtg_internal.hpp kPerlinPermWords), one of them under a checker. Up to 16 tables ride in LDS (their
    rows' LDS addresses fit the 16-bit offsets): the default LDS schedule; 17 do not, so the plan falls to
    the cache-read schedule with the tables in global memory. Both, and the plain grid, give cpu_ref32's
    frame."""
    import ctypes as C

    rng = np.random.default_rng(20261018)
    P = (rtgpu.rtg_perlin * tables)()
    for pl in P:
        v = rng.uniform(-1.0, 1.0, (256, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        for i in range(256):
            pl.randvec[i][0], pl.randvec[i][1], pl.randvec[i][2] = v[i]
        for name in ("perm_x", "perm_y", "perm_z"):
            getattr(pl, name)[:] = [int(x) for x in rng.permutation(256)]
    scales = (4.0, 2.5, 7.0)
    texs = [rtgpu.rtg_texture(type=rtgpu.RTG_TEX_NOISE, perlin=k, scale=scales[k % 3]) for k in range(tables)]
    texs.append(rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(0.9, 0.3, 0.2)))
    texs.append(rtgpu.rtg_texture(type=rtgpu.RTG_TEX_CHECKER, even=tables, odd=tables - 1, scale=0.8))
    # the ground, a checker ball over the last table, and a ball on every other table
    mats = [rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=t) for t in range(tables - 1)]
    mats.append(rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=tables + 1))

    def ball(c, r, m):
        return rtgpu.rtg_primitive(kind=rtgpu.RTG_PRIM_SPHERE, material=m, p0=rtgpu.D3(*c), p1=rtgpu.D3(*c),
                                   radius=r)

    prims = [ball((0, -1000, 0), 1000.0, 0)]
    for m in range(1, tables):
        a = 2 * np.pi * m / tables
        prims.append(ball((2.2 * np.cos(a), 0.8, 2.2 * np.sin(a)), 0.6, m))
    d = _desc(prims, mats, texs)
    d.perlins, d.num_perlins = C.cast(P, C.POINTER(rtgpu.rtg_perlin)), tables
    d._keep = d._keep + (P,)
    cam = rtgpu.camera(image_width=64, aspect_ratio=1.5, samples_per_pixel=4, max_depth=6,
                       background=(0.7, 0.8, 1.0), lookfrom=(0, 3, 7), lookat=(0, 0.8, 0))
    o, segs = oracle.render_f32(d, cam)
    ds = gpu_lib.scene_create(d)
    assert ds.plan(cam).schedule == schedule
    g, st = ds.render_host(cam)
    assert_parity(g, o, st, segs)
    H = gpu_lib.camera_resolve(cam).image_height
    out = np.zeros((H, 64, 3), dtype=np.float32)
    job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, rtgpu.RTG_RENDER_SCHEDULE(4), None)
    st4 = rtgpu.rtg_render_stats()
    gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(cam), C.byref(job), out.ctypes.data,
                                                       C.byref(st4)))
    ds.close()
    assert np.array_equal(out, g) and st4.segments == st.segments
    # the tables really differ on this frame: no two balls show the same noise
    assert len({g[r, c].tobytes() for r in range(H) for c in range(64)}) > 500


@pytest.mark.parametrize("bvh", [rtgpu.RTG_BVH_SAH, rtgpu.RTG_BVH_GPU, rtgpu.RTG_BVH_MEDIAN])
def test_exact_t_ties_match_oracle(gpu_lib, oracle, bvh):
    """The exact-t tie rule: three identical quads hit at bit-identical
    t. Whatever order a BVH builder makes the kernel test them in, the frame is cpu_ref32's bit for bit
    and shows the last quad of the list (interval::contains, quad.hpp:62), as the reference keeps it."""
    from tie_scene import BLUE, GREEN, RED, WHITE, colour_counts, tie_scene

    d, cam = tie_scene(bvh, width=96)
    ds = gpu_lib.scene_create(d)
    g, st = ds.render_host(cam)
    ds.close()
    o, segs = oracle.render_f32(d, cam)
    assert np.array_equal(g, o) and st.segments == segs
    n = colour_counts(g)
    assert n[GREEN] > 200 and n[BLUE] > 100 and n[RED] == 0 and n[WHITE] == 0, n


@pytest.mark.parametrize("bvh", [rtgpu.RTG_BVH_SAH, rtgpu.RTG_BVH_GPU, rtgpu.RTG_BVH_MEDIAN])
def test_sphere_ties_follow_list_order(gpu_lib, oracle, bvh):
    """Sphere-sphere exact-t ties (DESIGN.md §4 "tie rule"): groups of three identical
    emitting spheres, every ray that reaches them an exact tie; the reference's list walk keeps each group's
    FIRST member (sphere::hit never replaces an equal-t hit, interval::surrounds, sphere.hpp:70). Whatever
    order a BVH builder makes the kernel test them in, the frame and the segment count are cpu_ref32's bit
    for bit, and equal to the frame of the scene holding only the first members."""
    from tie_scene import duplicate_sphere_scene

    d, cam = duplicate_sphere_scene(bvh, width=96)
    ds = gpu_lib.scene_create(d)
    g, st = ds.render_host(cam)
    ds.close()
    o, segs = oracle.render_f32(d, cam)
    assert np.array_equal(g, o) and st.segments == segs, float(np.mean(np.all(g == o, axis=-1)))
    d1, cam1 = duplicate_sphere_scene(bvh, width=96, dedup=True)
    ds = gpu_lib.scene_create(d1)
    g1, _ = ds.render_host(cam1)
    ds.close()
    assert np.array_equal(g, g1)


@pytest.mark.parametrize("bvh", [rtgpu.RTG_BVH_SAH, rtgpu.RTG_BVH_GPU, rtgpu.RTG_BVH_MEDIAN])
def test_bvh_node_world_ties_follow_leaf_order(gpu_lib, scenes, oracle, bvh):
    """Exact-t ties in a world the reference wraps in a bvh_node (main.cpp:76): the
    reference keeps the first sphere and the last quad in its median tree's LEAF order (bvh_node.hpp:89-90),
    which the C++ mirror's bvh_node hands the library as tie ranks (rtg_scene_desc.tie_rank). tie_world
    (identical sphere groups, coplanar quads, identical compound children, every object its own colour)
    rendered wrapped in bvh_node and as a plain list: each frame and segment count is cpu_ref32's bit for
    bit for every BVH builder (the oracle's rule is pinned to the reference's own winners by
    test_oracle_golden.py::test_tie_winners_match_reference), and the two frames differ (the ranks reach
    the kernel)."""
    frames = {}
    for grid, key in ((0, "bvh_node"), (1, "list")):
        s = scenes.build("tie_world", grid=grid, bvh_mode=bvh)
        assert bool(s.desc.tie_rank) == (key == "bvh_node")
        cam = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
        ds = gpu_lib.scene_create(s.desc)
        g, st = ds.render_host(cam)
        ds.close()
        o, segs = oracle.render_f32(s.desc, cam)
        assert np.array_equal(g, o) and st.segments == segs, (key, float(np.mean(np.all(g == o, axis=-1))))
        frames[key] = g
        if bvh == rtgpu.RTG_BVH_SAH:  # the counting kernel checks where it reads the ranks at a tie
            ds = gpu_lib.scene_create(s.desc)
            gc, _ = ds.render_host(cam, count=True)
            ds.close()
            assert np.array_equal(gc, g)
    differ = int(np.sum(np.any(frames["bvh_node"] != frames["list"], axis=-1)))
    assert differ > 200, differ  # 255 of the 96 x 64 pixels on the MI355X (tie regions)


@pytest.mark.parametrize("competitor", ["quad", "sphere"])
@pytest.mark.parametrize("bvh", [rtgpu.RTG_BVH_SAH, rtgpu.RTG_BVH_GPU, rtgpu.RTG_BVH_MEDIAN])
def test_near_tie_culling_is_conservative(gpu_lib, oracle, bvh, competitor):
    """Conservative BVH culling: small spheres whose tops poke a
    fraction of an fp32 ulp above a quad or a large sphere at y = 1000, seen from just above. The
    competitor is tested first and its hit lies within the slab test's rounding of the small sphere's box
    entry; with the host-padded boxes and the tbest margin the kernel still enters that box, so the frame
    and the segment count are cpu_ref32's (which culls in f64 with a margin) bit for bit, for every BVH
    builder. A second camera 2500 units up lies beyond twice the primitives' reach, so its render first
    widens the margin on the device (ensure_origin_bound; the plan reports the new bound)."""
    from tie_scene import GREEN, colour_counts, near_tie_scene

    for h in (2.0, 2500.0):
        d, cam = near_tie_scene(bvh, competitor, width=96, cam_height=h)
        ds = gpu_lib.scene_create(d)
        m0 = ds.plan(cam).origin_bound
        g, st = ds.render_host(cam)
        m1 = ds.plan(cam).origin_bound
        ds.close()
        o, segs = oracle.render_f32(d, cam)
        if h < 10:
            assert colour_counts(o)[GREEN] > 500 and m1 == m0 and 1000 <= m0 <= 1002, (m0, m1)
        else:
            assert m0 <= 1002 and m1 >= (1000 + h) / 2, (m0, m1)
        assert np.array_equal(g, o) and st.segments == segs, (h, colour_counts(g), colour_counts(o))


@pytest.mark.parametrize("bvh", [rtgpu.RTG_BVH_SAH, rtgpu.RTG_BVH_GPU, rtgpu.RTG_BVH_MEDIAN])
@pytest.mark.parametrize("offset", [0.0, 3000.0])
def test_quad_edges_culling_is_conservative(gpu_lib, oracle, bvh, offset):
    """Per-primitive culling boxes (DESIGN.md §4 "conservative culling", round 5): a room of quads meeting at
    shared edges — axis-aligned walls and blocks (thin flat-axis pads, extent-aware in-plane pads, exits
    widened in the quad kernel), blocks rotated about skew axes and quads rotated within their plane (the
    general 2^-18 pads), spheres on top — rendered at 8 spp, depth 8, near the origin and translated 3000
    units away, with every BVH builder: every pixel and the segment count are cpu_ref32's."""
    from tie_scene import quad_edge_scene

    d, cam = quad_edge_scene(bvh, width=96, offset=offset)
    ds = gpu_lib.scene_create(d)
    g, st = ds.render_host(cam)
    ds.close()
    o, segs = oracle.render_f32(d, cam, threads=_host_threads())
    assert float(np.mean(o > 0)) > 0.5
    assert np.array_equal(g, o) and st.segments == segs, (float(np.mean(np.all(g == o, axis=-1))), st.segments,
                                                          segs)


def test_traversal_stack_spill_matches_oracle(gpu_lib, scenes, oracle, monkeypatch):
    """Deep BVHs keep the first stack entries in LDS and the rest in a global per-wave spill area
    (the 1M-sphere scene needs 36 entries). RTG_STACK_LDS_ENTRIES lowers the LDS part so that the
    spill path carries most of the stack here: both default schedules must still match the oracle
    bit for bit."""
    import ctypes as C

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 96, 4, 20
    o, segs = oracle.render_f32(s.desc, c)
    H = gpu_lib.camera_resolve(c).image_height
    for entries in ("1", "3"):
        monkeypatch.setenv("RTG_STACK_LDS_ENTRIES", entries)
        ds = gpu_lib.scene_create(s.desc)  # knobs are read once per scene
        for flags in (0, rtgpu.RTG_RENDER_SCHEDULE(4)):
            out = np.zeros((H, 96, 3), dtype=np.float32)
            job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, flags, None)
            st = rtgpu.rtg_render_stats()
            gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                                out.ctypes.data, C.byref(st)))
            assert_parity(out, o, st, segs)
        ds.close()


@pytest.mark.parametrize("bvh", [rtgpu.RTG_BVH_SAH, rtgpu.RTG_BVH_GPU])
@pytest.mark.parametrize("name", ["bouncing_spheres", "simple_light", "earth_perlin"])
def test_occluder_changes_work_not_pixels(gpu_lib, scenes, monkeypatch, name, bvh):
    """A scene-spanning sphere (the ground) is kept out of the 4-wide tree (host SAH or
    device-built) and tested by every ray before its traversal (DESIGN.md §3 "Scene-spanning
    occluder"). The closest hit is the same minimum either way, so the frame and the segment count
    must not change."""
    frames, stats = [], []
    for off in (False, True):
        if off:
            monkeypatch.setenv("RTG_NO_OCCLUDER", "1")
        else:
            monkeypatch.delenv("RTG_NO_OCCLUDER", raising=False)
        s = scenes.build(name, rand_seed=1, bvh_mode=bvh)
        c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
        c.image_width, c.samples_per_pixel, c.max_depth = 96, 8, 20
        ds = gpu_lib.scene_create(s.desc)
        img, st = ds.render_host(c)
        ds.close()
        frames.append(img)
        stats.append(st)
    # exact-t ties resolve by list order (the spec's tie rule), whatever the tree: identical frames
    assert np.array_equal(frames[0], frames[1])
    assert int(stats[0].segments) == int(stats[1].segments)


@pytest.mark.parametrize("name,W", [("bouncing_spheres", 96), ("cornell_box", 64), ("simple_light", 64),
                                    ("quads", 48)])
def test_device_bvh_build_matches_oracle(gpu_lib, scenes, oracle, name, W):
    """RTG_BVH_GPU (Morton LBVH built on the device): a different tree, the
    same image as the oracle (closest hits are order-free up to exact ties, H9)."""
    g, o, st, segs = compare(gpu_lib, scenes, oracle, name, bvh=rtgpu.RTG_BVH_GPU, image_width=W,
                             samples_per_pixel=4, max_depth=20)
    assert_parity(g, o, st, segs)


def test_device_bvh_build_million_spheres(gpu_lib, scenes, oracle):
    s = scenes.build("bouncing_spheres", grid=500, rand_seed=1, bvh_mode=rtgpu.RTG_BVH_GPU)
    ds = gpu_lib.scene_create(s.desc)
    info = ds.info()
    assert info.num_nodes > 1_000_001 // 8 and info.build_ms < 2000, (info.num_nodes, info.build_ms)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 64, 2, 50
    g, st = ds.render_host(c)
    ds.close()
    o, segs = oracle.render_f32(s.desc, c)
    assert_parity(g, o, st, segs)


def test_million_sphere_scene(gpu_lib, scenes, oracle):
    """BASELINE config 5 scene (grid 500 -> 1,000,001 objects, deep BVH) at a small image. 192 px
    wide: enough far-away grazing rays that the old h^2 - a c discriminant made the frame depend
    on box-culling precision (0.03 % of the pixels at 384 px)."""
    g, o, st, segs = compare(gpu_lib, scenes, oracle, "bouncing_spheres", grid=500, image_width=192,
                             aspect_ratio=16.0 / 9.0, samples_per_pixel=2, max_depth=50)
    assert_parity(g, o, st, segs)


def _host_threads():
    """CPU threads for the oracle: the affinity set, at most 16 (the GPU box's cgroup quota)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


# BASELINE configs 2-5 at full frame size, low spp: name, scene, grid, W, aspect, spp, depth
FULL_SIZE = [("config2", "bouncing_spheres", 0, 1920, 16.0 / 9.0, 2, 50),
             ("config3", "earth_perlin", 0, 1920, 16.0 / 9.0, 2, 50),
             ("config4", "cornell_box", 0, 800, 1.0, 2, 100),
             ("config5", "bouncing_spheres", 500, 3840, 16.0 / 9.0, 1, 50)]


@pytest.mark.parametrize("cfg", FULL_SIZE, ids=[c[0] for c in FULL_SIZE])
def test_full_size_frame_matches_oracle(gpu_lib, scenes, oracle, cfg):
    """Every BASELINE GPU config at its full frame size (1920x1080, 1920x1080, 800x800, 3840x2160) and
    its depth, at 1-2 spp, against cpu_ref32 over the host's cores: every pixel and the segment count
    identical (the sampled-row bench parity covers the benchmark spp). Config 2 also renders an
    interleaved shard (rows 3, 11, ...) that must equal those rows of the full frame."""
    name, scene, grid, W, aspect, spp, depth = cfg
    s = scenes.build(scene, grid=grid, rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.aspect_ratio, c.samples_per_pixel, c.max_depth = W, aspect, spp, depth
    ds = gpu_lib.scene_create(s.desc)
    g, st = ds.render_host(c, seed=7)
    if name == "config2":
        part, _ = ds.render_host(c, seed=7, row_begin=3, row_stride=8, row_count=0)
        assert np.array_equal(part, g[3::8])
    ds.close()
    H = gpu_lib.camera_resolve(c).image_height
    assert g.shape == (H, W, 3) and st.samples == H * W * spp
    o, segs = oracle.render_f32(s.desc, c, seed=7, threads=_host_threads())
    bad = np.argwhere(np.any(g != o, axis=-1))
    assert bad.shape[0] == 0 and int(st.segments) == int(segs), (name, bad[:8].tolist(), st.segments, segs)


def _gamma_boundary_values():
    """Linear values whose sqrt lands on (or one float ulp either side of) a byte boundary k/256,
    plus the clamp edges: where an fp32 sqrt / clamp would move a byte by one."""
    k = np.arange(0, 257, dtype=np.float64) / 256.0
    x = (k * k).astype(np.float32)
    up = np.nextafter(x, np.float32(np.inf))
    dn = np.nextafter(x, np.float32(-np.inf))
    edges = np.array([0.0, -0.0, -1e-30, 1e-45, 0.998001, 0.998002, np.float32(0.999) ** 2, 1.0, 3.0,
                      np.inf], dtype=np.float32)
    v = np.concatenate([x, up, dn, edges])
    return v[: (v.size // 3) * 3]


def test_resolve_rgb8_matches_write_color(gpu_lib, scenes, oracle):
    """write_color on the device (rtg_resolve_rgb8) is byte-exact against the oracle's
    write_color (the reference's double sqrt and clamp, color.hpp:14-58): random values and the
    values that sit on byte boundaries."""
    import torch

    s = scenes.build("cornell_box", rand_seed=1)
    ds = gpu_lib.scene_create(s.desc)
    g = torch.Generator().manual_seed(3)
    rnd = (torch.rand(4096 * 3, generator=g) * 1.3 - 0.1).numpy().astype(np.float32)
    vals = np.concatenate([rnd, _gamma_boundary_values()])
    n = vals.size // 3
    x = torch.from_numpy(vals).cuda()
    out = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
    ds.resolve_rgb8(x.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(-1, 3)
    ref = np.array([oracle.write_color([float(v) for v in px]) for px in vals.reshape(-1, 3)])
    assert np.array_equal(got.astype(int), ref)
    assert np.array_equal(got, rtgpu.write_color_bytes(vals.reshape(-1, 3)))
    ds.close()


def test_resolve_rgb8_of_a_rendered_frame(gpu_lib, scenes, oracle):
    """The RGB8 gather path end to end on one GPU: a rendered frame resolved on the device
    equals the reference write_color bytes of the same float frame, pixel for pixel."""
    import torch

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 160, 8, 20
    ds = gpu_lib.scene_create(s.desc)
    H = gpu_lib.camera_resolve(c).image_height
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.zeros((H, 160, 3), device="cuda")
    ds.render_device(c, frame.data_ptr(), stream)
    rgb8 = torch.empty((H, 160, 3), dtype=torch.uint8, device="cuda")
    ds.resolve_rgb8(frame.data_ptr(), rgb8.data_ptr(), H * 160, stream)
    torch.cuda.synchronize()
    f = frame.cpu().numpy()
    got = rgb8.cpu().numpy()
    assert np.array_equal(got, rtgpu.write_color_bytes(f))
    sample = f.reshape(-1, 3)[::97]
    ref = np.array([oracle.write_color([float(v) for v in px]) for px in sample])
    assert np.array_equal(got.reshape(-1, 3)[::97].astype(int), ref)
    ds.close()


def test_async_render_and_wait(gpu_lib, scenes, oracle):
    """RTG_RENDER_ASYNC returns after the launch; rtg_render_wait collects the stats. A second
    render before the wait is refused, and a wait with nothing pending is an error."""
    import torch

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 64, 4, 20
    ds = gpu_lib.scene_create(s.desc)
    H = gpu_lib.camera_resolve(c).image_height
    out = torch.zeros((H, 64, 3), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    st0 = ds.render_device(c, out.data_ptr(), stream, asynchronous=True)
    assert st0.segments == 0  # not collected yet
    with pytest.raises(rtgpu.RtgError):
        ds.render_device(c, out.data_ptr(), stream)
    st = ds.wait()
    with pytest.raises(rtgpu.RtgError):
        ds.wait()
    o, segs = oracle.render_f32(s.desc, c)
    assert_parity(out.cpu().numpy(), o, st, segs)
    with pytest.raises(rtgpu.RtgError):  # host output cannot be asynchronous
        job = rtgpu.rtg_render_desc(rtgpu.DEFAULT_SEED, 0, 1, 0, rtgpu.RTG_RENDER_ASYNC, None)
        import ctypes as C
        host = np.zeros((H, 64, 3), dtype=np.float32)
        gpu_lib.check("rtg_render", gpu_lib.lib.rtg_render(ds.handle, C.byref(c), C.byref(job),
                                                            host.ctypes.data, None))
    ds.close()


def test_device_output_on_torch_stream(gpu_lib, scenes, oracle):
    import torch

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 64, 2, 10
    ds = gpu_lib.scene_create(s.desc)
    H = gpu_lib.camera_resolve(c).image_height
    out = torch.zeros((H, 64, 3), device="cuda")
    st = ds.render_device(c, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, segs = oracle.render_f32(s.desc, c)
    assert_parity(out.cpu().numpy(), o, st, segs)
    ds.close()


def test_raytracer_cli_writes_ppm(tmp_path):
    exe = os.path.join(REPO, "raytracing-practice_amd", "bin", "raytracer")
    out = tmp_path / "cornell.ppm"
    subprocess.run([exe, str(out), "cornell_box", "64", "8", "20"], check=True, timeout=120,
                   capture_output=True)
    tokens = out.read_text().split()
    assert tokens[:4] == ["P3", "64", "64", "255"]
    vals = np.array(tokens[4:], dtype=int)
    assert vals.size == 64 * 64 * 3 and vals.min() >= 0 and vals.max() <= 255 and vals.max() > 0
    # rows split over several devices (here the same GPU twice, one host thread each): same bytes
    out2 = tmp_path / "cornell2.ppm"
    subprocess.run([exe, str(out2), "cornell_box", "64", "8", "20", "0,0,0"], check=True, timeout=120,
                   capture_output=True)
    assert out2.read_bytes() == out.read_bytes()
    # distinct devices: the RCCL frame path (rtg_render_frame); on a one-GPU box a world of one
    out3 = tmp_path / "cornell3.ppm"
    subprocess.run([exe, str(out3), "cornell_box", "64", "8", "20", "0"], check=True, timeout=120,
                   capture_output=True)
    assert out3.read_bytes() == out.read_bytes()


@pytest.mark.parametrize("nranks,height,W,dtype", [(2, 37, 24, np.float32), (3, 20, 16, np.float32),
                                                    (8, 135, 32, np.float32), (8, 9, 5, np.uint8),
                                                    (5, 3, 64, np.uint8)])
def test_deinterleave_kernel(gpu_lib, nranks, height, W, dtype):
    """The root's de-interleave step of rtg_gather_rows (rtg_comm.cpp) on its own: nranks blocks of
    ceil(H/N) padded rows -> image rows r + k*N; 16-byte path (fp32 RGB rows) and byte path (RGB8
    rows of 15 bytes), ranks past the last row (N=5, H=3)."""
    import torch

    P = (height + nranks - 1) // nranks
    g = torch.Generator().manual_seed(nranks * 1000 + height)
    if dtype == np.float32:
        blocks = torch.rand((nranks, P, W, 3), generator=g)
    else:
        blocks = torch.randint(0, 256, (nranks, P, W, 3), generator=g, dtype=torch.uint8)
    dev = blocks.cuda()
    out = torch.zeros((height, W, 3), dtype=blocks.dtype, device="cuda")
    row_bytes = W * 3 * blocks.element_size()
    gpu_lib.deinterleave_rows(0, dev.data_ptr(), out.data_ptr(), nranks, height, row_bytes,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    expect = rtgpu.deinterleave([b.numpy() for b in blocks], height)
    assert np.array_equal(out.cpu().numpy(), expect)


def test_comm_world_of_one(gpu_lib, scenes):
    """rtg_comm at world size 1 (the one-GPU box): ncclCommInitAll / ncclCommInitRank, the RCCL
    gather + de-interleave of a rendered shard, and rtg_render_frame == a plain render."""
    import torch

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 80, 4, 20
    ds = gpu_lib.scene_create(s.desc)
    ref, st = ds.render_host(c, seed=11)
    H, W = ref.shape[:2]
    comm = gpu_lib.comm_local([0])
    assert comm.size() == (1, 1)
    frame, fst = comm.render_frame([ds], c, seed=11)
    assert np.array_equal(frame, ref) and fst.segments == st.segments
    # the gather on its own, through a one-process-per-GPU communicator of one rank
    comm2 = gpu_lib.comm_rank(gpu_lib.comm_unique_id(), 1, 0, 0)
    shard = torch.from_numpy(ref).cuda()
    out = torch.zeros_like(shard)
    stream = torch.cuda.current_stream().cuda_stream
    comm2.gather_rows([shard.data_ptr()], H, W * 12, 0, out.data_ptr(), [stream])
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    comm2.close()
    comm.close()
    ds.close()


def test_far_camera_repad_then_prepare_on_another_stream(gpu_lib, scenes, oracle):
    """a camera beyond twice the primitives' reach makes a render widen the culling margin on the
    device (the repad) on the render's stream; rtg_scene_prepare with a NULL stream then downloads the node
    array for the hot treelet and uploads it renumbered. The repad is synchronous, so that download already
    holds the widened boxes and the plan's origin_bound is true of the device array: renders of the far
    camera after the prepare are cpu_ref32's frames bit for bit (treelet schedule, 14k spheres)."""
    import torch

    s = scenes.build("bouncing_spheres", grid=60)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.aspect_ratio, c.samples_per_pixel, c.max_depth = 64, 16.0 / 9.0, 2, 8
    c.lookfrom, c.lookat, c.vfov, c.defocus_angle = rtgpu.D3(4500.0, 800.0, 900.0), rtgpu.D3(0.0, 0.0, 0.0), 1.0, 0.0
    ds = gpu_lib.scene_create(s.desc)
    assert ds.plan(c).schedule == 5
    bound0 = ds.plan(c).origin_bound
    out = torch.zeros((36, 64, 3), dtype=torch.float32, device="cuda")
    user = torch.cuda.Stream()
    ds.render_device(c, out.data_ptr(), user.cuda_stream)
    assert ds.plan(c).origin_bound > bound0 >= 0
    c2 = rtgpu.rtg_camera_desc.from_buffer_copy(c)
    c2.lookat = rtgpu.D3(10.0, 0.0, 5.0)  # another camera: the prepare re-tunes (downloads the nodes)
    ds.prepare(c2)
    g, st = ds.render_host(c)
    o, segs = oracle.render_f32(s.desc, c)
    torch.cuda.synchronize()
    assert np.array_equal(g, o) and st.segments == segs
    assert np.array_equal(out.cpu().numpy(), o)
    ds.close()


@pytest.mark.parametrize("world,height", [(2, 5), (3, 7), (8, 21)])
def test_frame_gather_device_deinterleave(gpu_lib, world, height):
    """bench.py's timed N > 1 gather (rtgpu.FrameGather) de-interleaves CUDA staging blocks with
    the library's kernel on the stream; the CPU tests only reach the host twin. Here the staging blocks are
    filled by hand (every element its own value, the padding rows included) and FrameGather's CUDA step must
    give the host twin's frame exactly."""
    import torch

    padded, W = -(-height // world), 5
    fg = rtgpu.FrameGather.__new__(rtgpu.FrameGather)  # no process group: the dst rank's state set up by hand
    fg.lib, fg.height, fg.dst, fg.device, fg.world, fg.rank = gpu_lib, height, 0, 0, world, 0
    fg.shape, fg.row_bytes = (padded, W, 3), W * 3 * 4
    fg.stage = torch.arange(world * padded * W * 3, dtype=torch.float32, device="cuda").reshape(world, padded, W, 3)
    fg.frame = torch.full((height, W, 3), -1.0, device="cuda")
    out = fg.deinterleave(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = gpu_lib.deinterleave_rows_host(fg.stage.cpu().numpy().reshape(world * padded, W, 3), world, height)
    assert want.shape == (height, W, 3) and np.array_equal(out.cpu().numpy(), want)


def test_frames_allocate_nothing_after_the_first(gpu_lib, scenes):
    """the C-ABI frame path keeps its buffers (the scene's render scratch and output,
    the communicator's shard, frame and gather staging buffers), so after the first frame neither
    rtg_render_frame nor rtg_gather_rows nor a chunked rtg_render allocates anything
    (rtg_allocation_count counts every device / pinned allocation of the library). World of one."""
    import torch

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 96, 40, 20  # 3 chunks: partial sums in use
    ds = gpu_lib.scene_create(s.desc)
    comm = gpu_lib.comm_local([0])
    frames, counts = [], []
    for k in range(5):
        f, _ = comm.render_frame([ds], c, seed=3)
        frames.append(f)
        counts.append(gpu_lib.allocation_count()[0])
    assert counts[1:] == [counts[0]] * 4, counts
    assert all(np.array_equal(f, frames[0]) for f in frames)
    ref, _ = ds.render_host(c, seed=3)
    assert np.array_equal(ref, frames[0])
    comm2 = gpu_lib.comm_rank(gpu_lib.comm_unique_id(), 1, 0, 0)
    H, W = ref.shape[:2]
    shard = torch.from_numpy(ref).cuda()
    out = torch.zeros_like(shard)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    counts = []
    for k in range(5):
        comm2.gather_rows([shard.data_ptr()], H, W * 12, 0, out.data_ptr(), [stream])
        counts.append(gpu_lib.allocation_count()[0])
    torch.cuda.synchronize()
    assert counts[1:] == [counts[0]] * 4, counts
    assert np.array_equal(out.cpu().numpy(), ref)
    n0 = gpu_lib.allocation_count()[0]
    for k in range(3):
        g, _ = ds.render_host(c, seed=3)
    assert gpu_lib.allocation_count()[0] == n0 and np.array_equal(g, ref)
    comm2.close()
    comm.close()
    ds.close()


def test_gathers_in_flight_on_two_streams(gpu_lib, scenes):
    """rtg_gather_rows's staging buffer belongs to the communicator (ABI 7: kept between gathers); a
    gather on another stream waits for the previous one's de-interleave first: two gathers of different
    frames enqueued back to back on two streams both land intact."""
    import torch

    s = scenes.build("bouncing_spheres", rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = 64, 2, 10
    ds = gpu_lib.scene_create(s.desc)
    a, _ = ds.render_host(c, seed=1)
    b, _ = ds.render_host(c, seed=2)
    H, W = a.shape[:2]
    comm = gpu_lib.comm_rank(gpu_lib.comm_unique_id(), 1, 0, 0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    oa, ob = torch.zeros_like(da), torch.zeros_like(db)
    torch.cuda.synchronize()
    comm.gather_rows([da.data_ptr()], H, W * 12, 0, oa.data_ptr(), [sa.cuda_stream])
    comm.gather_rows([db.data_ptr()], H, W * 12, 0, ob.data_ptr(), [sb.cuda_stream])
    torch.cuda.synchronize()
    assert np.array_equal(oa.cpu().numpy(), a) and np.array_equal(ob.cpu().numpy(), b)
    assert comm.size() == (1, 1)  # ncclCommCount
    comm.close()
    ds.close()


def test_render_frame_over_two_devices(gpu_lib, scenes):
    """rtg_render_frame over two GPUs of one process (ncclCommInitAll; the RCCL gather of interleaved
    shards + the root's de-interleave) equals a one-device render bit for bit, also when the image has
    fewer rows than ranks (a rank that only sends padding). Needs two devices: skipped on a one-GPU box
    (RCCL takes one rank per device, profiles/r02_ab/comm_probe_two_ranks_one_gpu.log)."""
    if gpu_lib.device_count() < 2:
        pytest.skip("needs two GPUs")
    s = scenes.build("bouncing_spheres", rand_seed=1)
    for W, aspect in ((96, 16.0 / 9.0), (64, 64.0)):  # H = 54, then H = 1 < 2 ranks
        c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
        c.image_width, c.aspect_ratio, c.samples_per_pixel, c.max_depth = W, aspect, 4, 20
        d0, d1 = gpu_lib.scene_create(s.desc, device=0), gpu_lib.scene_create(s.desc, device=1)
        ref, st = d0.render_host(c, seed=5)
        comm = gpu_lib.comm_local([0, 1])
        assert comm.size() == (2, 2)
        frame, fst = comm.render_frame([d0, d1], c, seed=5)
        assert np.array_equal(frame, ref) and fst.segments == st.segments
        comm.close()
        d0.close()
        d1.close()


@pytest.mark.parametrize("name,grid,W,schedule,dual,waves_per_simd", [
    ("bouncing_spheres", 11, 1920, 3, 1, 5), ("cornell_box", 0, 800, 3, 0, 5),
    ("earth_perlin", 0, 1920, 3, 0, 5), ("bouncing_spheres", 500, 3840, 5, 0, 4)])
def test_render_plan_names_the_kernel(gpu_lib, scenes, name, grid, W, schedule, dual, waves_per_simd):
    """rtg_render_plan reports the launch the benchmark configs run: the schedule, the
    dual launch, the waves per SIMD and the compiled kernel's own VGPR count (the bench record's
    binding field quotes it instead of rocprofv3's allocation granule)."""
    s = scenes.build(name, grid=grid, rand_seed=1)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.samples_per_pixel, c.max_depth = W, 500, 50
    ds = gpu_lib.scene_create(s.desc)
    p = ds.plan(c)
    ds.close()
    assert (p.schedule, p.dual, p.waves_per_simd) == (schedule, dual, waves_per_simd), p.as_dict()
    assert 0 < p.vgprs <= 512 // waves_per_simd and p.chunks == 32 and p.chunk_samples == 16
    assert p.num_cus > 0 and p.workgroups > 0
    H = gpu_lib.camera_resolve(c).image_height
    assert p.tile_slots == 0 and p.partial_bytes == H * W * 12 * 32, p.as_dict()  # < 32 GiB: full-frame
    if grid == 500:  # config 5 as benchmarked (1000 spp): 6.3 GB of full-frame partials, below the tile
        # ring's 32 GiB default bound since round 5; forced on, the ring holds ~2^17 batches of 1 KiB
        # (R * chunks) plus 8 B of slot words per slot
        c.samples_per_pixel = 1000
        ds = gpu_lib.scene_create(s.desc)
        p = ds.plan(c)
        assert p.chunks == 63 and p.tile_slots == 0 and p.partial_bytes == H * W * 12 * 63, p.as_dict()
        ds.close()
        import os

        os.environ["RTG_TILE_SLOTS"] = "2048"
        try:
            ds = gpu_lib.scene_create(s.desc)
            p = ds.plan(c)
            ds.close()
        finally:
            del os.environ["RTG_TILE_SLOTS"]
        assert p.chunks == 63 and p.tile_slots == 2048, p.as_dict()
        assert p.partial_bytes == 2048 * 63 * 1024 + 8 * 2048 < H * W * 12 * 63 // 40


def test_bench_rtg_gather_check_world_of_one(tmp_path):
    """bench.py's N > 1 cross-check of the product gather (rtg_gather_check: rtg_comm_create_rank with the id
    broadcast over torch.distributed, rtg_gather_rows once per timed step, each call timed, the library's
    allocations counted) only runs on a multi-GPU node; here the same function at world 1 (gloo for the id
    broadcast, a one-rank RCCL communicator): status ok, the frame byte-identical, 4 calls, no allocation
    after the first."""
    import json
    import socket
    import sys

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = f"""
import json, os, sys
sys.path.insert(0, {REPO!r})
sys.path.insert(0, os.path.join({REPO!r}, "raytracing-practice_amd", "python"))
import torch, torch.distributed as dist
import rtgpu, bench
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="{port}")
dist.init_process_group("gloo", rank=0, world_size=1)
lib = rtgpu.Library()
H, W = 54, 96
shard = torch.rand((H, W, 3), device="cuda")
rec = bench.rtg_gather_check(lib, dist, torch, 1, 0, 0, H, W, shard, shard.clone(),
                             torch.cuda.current_stream().cuda_stream, 4)
print(json.dumps(rec))
dist.destroy_process_group()
"""
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert rec["status"] == "ok" and rec["identical_to_timed_frame"] is True and rec["ranks_seen"] == 1
    assert rec["calls"] == 4 and rec["allocations_after_first_call"] == 0 and rec["gather_ms"] > 0


def test_bench_two_ranks_rehearsal(tmp_path):
    """bench.py's N > 1 flow (interleaved shards, the gather on rank 0, per-rank records, the per-pixel
    check of the gathered frame against cpu_ref32, max-over-ranks timing) with two ranks on this one GPU
    over gloo (RCCL takes one rank per device, so the rtg_gather_rows cross-check is the driver's
    multi-GPU run's). The gathered frame must match the oracle on the sampled rows."""
    import json
    import socket
    import sys

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--dist-backend", "gloo", "--width", "192", "--height", "108", "--spp", "8",
           "--depth", "10", "--steps", "2", "--warmup", "1", "--full", "--parity-seconds", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and [x["rank"] for x in line["ranks"]] == [0, 1]
    assert [x["rows"] for x in line["ranks"]] == [54, 54] and all(x["segments"] > 0 for x in line["ranks"])
    assert line["parity"]["pass"] and line["parity"]["rows"] >= 2, line["parity"]
    assert line["parity"]["identical_frac"] > 0.999
    assert all(g is not None and g >= 0 for g in line["gather_ms"])
    assert line["cpu_baseline"] is None  # rank 0 at N = 1 only


def test_bench_launches_its_own_ranks(tmp_path):
    """A plain `bench.py --gpus 2` (no torch.distributed.run around it, as a driver may invoke
    `bench.py --gpus 8`) starts its two ranks itself: the line must say n_gpus 2,
    carry both ranks' records and pass the per-pixel check of the gathered frame. gloo: two ranks share
    this one GPU (RCCL takes one rank per device)."""
    import json
    import sys

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
           "--width", "160", "--height", "90", "--spp", "4", "--depth", "8", "--steps", "1", "--warmup", "1",
           "--full", "--parity-seconds", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and [x["rank"] for x in line["ranks"]] == [0, 1]
    assert [x["rows"] for x in line["ranks"]] == [45, 45]
    assert line["parity"]["pass"] and line["parity"]["identical_frac"] > 0.999, line["parity"]


def test_bench_plain_run_dumps_its_last_frame(tmp_path, scenes, oracle):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times its K steps and nothing else: the line says
    so (`full` false, no roofline record, CPU baseline or per-pixel check), and `--dump-outputs DIR` leaves
    the last timed frame (seed + W + K - 1) there as float32, every row of it at this size: the oracle's
    frame on that seed (north star: RMSE < 1e-3), with that step's segment count."""
    import json
    import sys

    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--width", "160", "--height", "90", "--spp", "4", "--depth", "8", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "Mrays/s" and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"] is None and line["cpu_baseline"] is None and "parity" not in line
    frame, rows, segs = (np.load(out / f"{k}.npy") for k in ("frame", "frame_rows", "segments"))
    assert frame.dtype == np.float32 and frame.shape == (90, 160, 3)
    assert rows.dtype == np.float64 and np.array_equal(rows, np.arange(90))
    s = scenes.build("bouncing_spheres", grid=11, image_width=160, aspect_ratio=160 / 90, spp=4, max_depth=8,
                     rand_seed=1)
    ref, ref_segs = oracle.render_f32(s.desc, s.camera, seed=0x5EED + 2)
    assert np.all(np.isfinite(frame)) and rmse(frame, ref) < RMSE_TOL
    assert segs.dtype == np.float64 and abs(int(segs[0]) - int(ref_segs)) <= max(2, 1e-4 * ref_segs)


def test_numerics_helpers_match_ieee():
    """div_rn / sqrt_rn (csrc/rtg_numerics.hpp) give the same bits as hipcc's correctly
    rounded `x / y` and `sqrtf` on 2^24 random operands of each kind from the ranges the kernels use:
    numerators 2^-60..2^61 (with zeros and ones), divisors 2^-30..2^31, sqrt operands 0 and
    2^-90..2^101, and the kernels' own sqrt operands (a 24-bit uniform U, 1 - z^2 for z = 1 - 2U,
    plain and fused); and the sphere test's near-root division c / q on the small divisors its guard
    lets through (2^-100 .. 2^-20, numerators 2^-60..2^40; ADVICE r02: tangent rays make q arbitrarily
    small, and |q| < 2^-100 is a miss in the spec)."""
    import ctypes as C
    so = C.CDLL(os.path.join(REPO, "tests", "native", "libnumcheck.so"))
    so.rtg_numerics_check.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_ulonglong), C.POINTER(C.c_float)]
    so.rtg_numerics_check.restype = C.c_int
    out, ex = (C.c_ulonglong * 5)(), (C.c_float * 4)()
    for seed in (0x5EED, 0xC0FFEE):
        assert so.rtg_numerics_check(1 << 24, seed, out, ex) == 0
        assert out[3] == 1 << 24
        assert (out[0], out[1], out[2], out[4]) == (0, 0, 0, 0), (list(out), list(ex))



def test_library_before_torch_keeps_one_hip_runtime():
    """Loading the library before torch must leave torch's device usable (one HIP runtime per
    process: rtgpu loads torch's first; the other order made torch report "No HIP GPUs")."""
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, %r); import rtgpu; L = rtgpu.Library(); "
            "assert L.device_count() >= 1; import torch; torch.cuda.init(); "
            "x = torch.ones(4, device='cuda'); print(float(x.sum()))"
            % os.path.join(REPO, "raytracing-practice_amd", "python"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("4.0"), r.stderr[-2000:]
