"""The render kernels' restart path (everything a wave runs between two traversal trip loops: path end, unit
hand-out, sample start, the occluder test): late kernel-argument reads, the occluder's test from scene constants
and the per-wave trace in the counting kernels. None of it changes a value, so every frame here equals cpu_ref32
(Oracle.render_f32) pixel for pixel, and the segment counts agree, on the same seed."""
import ctypes as C

import numpy as np
import pytest

import rtgpu
from test_gpu import _desc

pytestmark = pytest.mark.gpu


def _render(lib, ds, cam, schedule=0, seed=rtgpu.DEFAULT_SEED, row_begin=0, row_stride=1):
    p = lib.camera_resolve(cam)
    rows = (p.image_height - 1 - row_begin) // row_stride + 1
    out = np.zeros((rows, p.image_width, 3), dtype=np.float32)
    job = rtgpu.rtg_render_desc(seed, row_begin, row_stride, rows, rtgpu.RTG_RENDER_SCHEDULE(schedule), None)
    st = rtgpu.rtg_render_stats()
    lib.check("rtg_render", lib.lib.rtg_render(ds.handle, C.byref(cam), C.byref(job), out.ctypes.data, C.byref(st)))
    return out, st


def _same(g, st, o, segs):
    bad = int(np.any(g != o, axis=-1).sum())
    print(f"pixels off the oracle: {bad} of {g.shape[0] * g.shape[1]}, segments gpu {st.segments} cpu_ref32 {segs}")
    assert g.shape == o.shape and bad == 0
    assert int(st.segments) == int(segs)


def _book1(scenes, W, spp):
    s = scenes.build("bouncing_spheres", rand_seed=1, grid=2)
    c = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
    c.image_width, c.aspect_ratio, c.samples_per_pixel, c.max_depth = W, 16.0 / 9.0, spp, 50
    assert c.defocus_angle > 0  # the lens-disk half of the sample start
    return s, c


@pytest.mark.parametrize("spp", [17, 16, 1])
def test_chunk_edges(gpu_lib, scenes, oracle, spp):
    """Chunks of 16 + 1 samples (partial sums and their combine), one full chunk (the pixel stored directly), one
    sample."""
    s, c = _book1(scenes, 64, spp)
    assert rtgpu.num_chunks(spp) == (2 if spp == 17 else 1)
    ds = gpu_lib.scene_create(s.desc)
    g, st = _render(gpu_lib, ds, c)
    ds.close()
    assert g.shape == (36, 64, 3)
    _same(g, st, *oracle.render_f32(s.desc, c))


def test_late_reads_with_a_shard_and_a_tile_order(gpu_lib, scenes, oracle):
    """A prepared (cost-ordered) strided shard of a frame whose width is no multiple of the tile: the hand-out's
    image-edge branch, row_begin / row_stride in the sample start, the tile order's late read."""
    s, c = _book1(scenes, 70, 17)
    c.aspect_ratio = 70.0 / 37.5  # 37 rows
    ds = gpu_lib.scene_create(s.desc)
    ds.prepare(c, row_begin=1, row_stride=3)
    g, st = _render(gpu_lib, ds, c, row_begin=1, row_stride=3)
    ds.close()
    assert g.shape == (12, 70, 3) and st.tile_order == 1
    _same(g, st, *oracle.render_f32(s.desc, c, row_begin=1, row_stride=3))


def _ground_scene(ground_p1, ground_at=(0.0, -1000.0, 0.0), bvh=rtgpu.RTG_BVH_SAH):
    """A ground sphere (the scene-spanning occluder of the 4-wide trees, as in test_ground_and_one_sphere) under
    three small spheres: lambertian, metal, glass."""
    tex = rtgpu.rtg_texture(type=rtgpu.RTG_TEX_SOLID, color=rtgpu.D3(0.5, 0.5, 0.2))
    mats = [rtgpu.rtg_material(type=rtgpu.RTG_MAT_LAMBERTIAN, texture=0),
            rtgpu.rtg_material(type=rtgpu.RTG_MAT_METAL, texture=-1, albedo=rtgpu.D3(0.8, 0.6, 0.4), fuzz=0.1),
            rtgpu.rtg_material(type=rtgpu.RTG_MAT_DIELECTRIC, texture=-1, refraction_index=1.5)]
    prims = [rtgpu.rtg_primitive(kind=rtgpu.RTG_PRIM_SPHERE, material=0, p0=rtgpu.D3(*ground_at),
                                 p1=rtgpu.D3(*ground_p1), radius=1000.0)]
    for k, x in enumerate((-1.1, 0.0, 1.1)):
        prims.append(rtgpu.rtg_primitive(kind=rtgpu.RTG_PRIM_SPHERE, material=k, p0=rtgpu.D3(x, 0.5, 0.0),
                                         p1=rtgpu.D3(x, 0.5, 0.0), radius=0.5))
    d = _desc(prims, mats, [tex])
    d.bvh_mode = bvh
    return d


GROUND_CAM = dict(image_width=40, aspect_ratio=40.0 / 27.5, samples_per_pixel=4, max_depth=12,
                  background=(0.7, 0.8, 1.0), lookfrom=(0, 1.2, 4), lookat=(0, 0.4, 0), vfov=40.0)


@pytest.mark.parametrize("schedule", [3, 4])
@pytest.mark.parametrize("case", ["static", "moving", "none"])
def test_occluder_static_moving_none(gpu_lib, scenes, oracle, case, schedule):
    """The occluder's test from the scene's constants (zero velocity), the general test on its record (a ground
    that moves: its centre depends on the ray's time), and a scene without a sphere occluder."""
    if case == "none":
        s = scenes.build("cornell_box", rand_seed=1)
        desc = s.desc
        cam = rtgpu.rtg_camera_desc.from_buffer_copy(s.camera)
        cam.image_width, cam.aspect_ratio, cam.samples_per_pixel, cam.max_depth = 32, 1.0, 4, 100
    else:
        desc = _ground_scene((0.0, -1000.0, 0.0) if case == "static" else (0.0, -999.75, 0.125))
        cam = rtgpu.camera(**GROUND_CAM)
    ds = gpu_lib.scene_create(desc)
    g, st = _render(gpu_lib, ds, cam, schedule=schedule)
    ds.close()
    o, segs = oracle.render_f32(desc, cam)
    _same(g, st, o, segs)
    assert st.segments > st.samples  # paths bounce


def test_update_refreshes_the_occluder_constants(gpu_lib, oracle):
    """rtg_scene_update moves (and shrinks) the ground: the frame equals a fresh scene's of the moved primitives,
    bit for bit, and cpu_ref32's; moved again with a velocity, the general path's."""
    cam = rtgpu.camera(**GROUND_CAM)
    ds = gpu_lib.scene_create(_ground_scene((0.0, -1000.0, 0.0), bvh=rtgpu.RTG_BVH_SAH | rtgpu.RTG_BVH_REFIT))
    try:
        before, _ = _render(gpu_lib, ds, cam)
        for at, p1, radius in (((0.25, -900.25, 0.5), (0.25, -900.25, 0.5), 900.0),
                               ((0.0, -1000.0, 0.0), (0.0, -999.5, 0.0), 1000.0)):
            row = np.zeros((1, 12), np.float32)
            row[0, 0:3], row[0, 3], row[0, 4:7] = at, radius, p1
            st = ds.update(np.array([0], np.int32), row)
            assert st.updated == 1 and st.invalid == 0
            got, gst = _render(gpu_lib, ds, cam)
            moved = _ground_scene(p1, ground_at=at)
            moved.prims[0].radius = radius
            fresh = gpu_lib.scene_create(moved)
            want, wst = _render(gpu_lib, fresh, cam)
            fresh.close()
            assert np.array_equal(got, want) and gst.segments == wst.segments
            assert not np.array_equal(got, before)
            _same(got, gst, *oracle.render_f32(moved, cam))
    finally:
        ds.close()


def test_wave_trace_still_works(gpu_lib, scenes, oracle, tmp_path, monkeypatch):
    """RTG_WAVE_TRACE (read when the scene is created) renders with the counting kernels: the same frame, and the
    waves' finished units add up to W x H x chunks."""
    s, c = _book1(scenes, 64, 17)
    ds = gpu_lib.scene_create(s.desc)
    plain, pst = _render(gpu_lib, ds, c)
    ds.close()
    path = tmp_path / "trace.bin"
    monkeypatch.setenv("RTG_WAVE_TRACE", str(path))
    ds = gpu_lib.scene_create(s.desc)
    monkeypatch.delenv("RTG_WAVE_TRACE")
    traced, tst = _render(gpu_lib, ds, c)
    ds.close()
    assert np.array_equal(traced, plain) and tst.segments == pst.segments
    _same(traced, tst, *oracle.render_f32(s.desc, c))
    t = np.fromfile(path, dtype=np.uint64).reshape(-1, 4)
    t = t[t[:, 1] > 0]
    assert len(t) > 0 and np.all(t[:, 1] >= t[:, 0])
    assert int(t[:, 2].sum()) == 64 * 36 * rtgpu.num_chunks(17)
