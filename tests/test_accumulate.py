"""Progressive accumulation (FR_FLAG_ACCUMULATE) on the GPU against the oracle, bit for bit.

The contract (include/forma_rt.h): an accumulating frame is traced like the plain frame; its
per-pixel sum S (spp samples added in sample order from zero) joins the context's accumulator
as a unit, A = S or A = A + S in f32, n += spp, mean = A / (float)n, u8 = to_u8(mean).

The exact reference: for spp a power of two the oracle's mean is S / spp exactly (no nonzero
mean is near the subnormals, asserted below), so S_k = mean_k * spp exactly in f32, and the
expected image after frame k is A_1 = S_1, A_k = A_(k-1) + S_k, mean = A_k / float32(n) in
numpy f32, with to_u8 restated in numpy. Bits are compared, not a tolerance. After every
frame: the mean's bits, the u8 image, accum_info == (k, sum of spp) and the frame's own
segments and hits against the oracle frame's.

Images are 33x17 or 32x24: 15 or 12 tiles of 64 pixel slots, so several sum workgroups, the
last one partly filled, and at 33x17 partial tiles and a partial strip."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0 = 0xACC0


@functools.lru_cache(maxsize=None)
def _scene_text(key):
    if key == "cubes100":  # tests/golden/generator_100_cubes.json pins this text: 100 diffuse cubes, a BVH scene
        spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(ROOT, "tools", "gen_scene.py"))
        gs = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gs)
        return gs.dumps(gs.generator_scene(100, "cube"))
    import forma_rt
    return open(forma_rt.scene_path(key)).read()


def _product_scene(gpu, key, w, h):
    if key == "builtin0":
        return gpu.Scene.builtin(0, w, h)
    return gpu.Scene.from_json(_scene_text(key), w, h)


def _oracle_scene(key, w, h):
    if key == "builtin0":
        return S.BUILTIN[0](), O.camera_new(w, h)
    prims, (frm, at, vup, fov) = S.load_json(_scene_text(key))
    return prims, O.camera_look(frm, at, vup, fov, 0.1, w, h)


@functools.lru_cache(maxsize=None)
def _oracle_frame(key, w, h, spp, depth, seed):
    """One oracle frame, computed once and shared: (mean, u8, segments, hits), read-only."""
    prims, cam = _oracle_scene(key, w, h)
    mean, u8, cnt, rows = O.render(prims, cam, w, h, spp, depth, seed=seed, threads=8)
    assert rows == h and not np.isnan(mean).any()
    mean.setflags(write=False)
    u8.setflags(write=False)
    return mean, u8, cnt["segments"], cnt["hits"]


def _to_u8(mean):
    """rt_core.h to_u8 in numpy f32: sqrt * 255, NaN or <= 0 -> 0, >= 255 -> 255, truncation."""
    with np.errstate(invalid="ignore"):
        s = np.sqrt(mean.astype(np.float32)) * np.float32(255.0)
    return np.where(~(s > 0), 0, np.where(s >= 255, 255, np.trunc(np.nan_to_num(s)))).astype(np.uint8)


def _frame_sum(mean, spp):
    """S = mean * spp, exact for spp a power of two while no nonzero mean is near the subnormals."""
    assert spp & (spp - 1) == 0
    nz = mean[mean != 0]
    assert nz.size == 0 or float(np.min(np.abs(nz))) >= 2.0 ** -100
    s = (mean * np.float32(spp)).astype(np.float32)
    assert np.array_equal((s / np.float32(spp)).view(np.uint32), mean.view(np.uint32))
    return s


class Composite:
    """The expected accumulator, in numpy f32."""

    def __init__(self):
        self.a, self.n, self.frames = None, 0, 0

    def add(self, s, spp):
        self.a = s.copy() if self.a is None else (self.a + s).astype(np.float32)
        self.n += spp
        self.frames += 1
        mean = (self.a / np.float32(self.n)).astype(np.float32)
        return mean, _to_u8(mean)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _accumulate(gpu, key, w, h, depth, spps, scene_jit=False, ctx=None, sc=None, comp=None):
    """Renders len(spps) accumulating frames of distinct seeds on one context, syncing after
    each, and checks every frame against the composite of the oracle's frames. sc, comp: the
    scene object and the composite of an accumulation to go on with."""
    sc = _product_scene(gpu, key, w, h) if sc is None else sc
    own = ctx is None
    ctx = gpu.RenderContext(0) if own else ctx
    comp = Composite() if comp is None else comp
    for spp in spps:
        k = comp.frames
        seed = SEED0 + k
        omean, _, osegs, ohits = _oracle_frame(key, w, h, spp, depth, seed)
        want_mean, want_u8 = comp.add(_frame_sum(omean, spp), spp)
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, seed, accumulate=True, scene_jit=scene_jit))
        st = ctx.sync()
        mean, u8 = ctx.download(w, h)
        assert _same_bits(mean, want_mean), (k, float(np.max(np.abs(mean - want_mean))))
        assert np.array_equal(u8, want_u8), k
        assert ctx.accum_info() == (comp.frames, comp.n), k
        assert (st["segments"], st["hits"]) == (osegs, ohits), k
        assert st["samples"] == w * h * spp
    if scene_jit:
        assert ctx.jit_state() == gpu.FR_JIT_USED
    if own:
        ctx.close()
    return comp


# the sum paths, at the smallest shapes that reach them
def test_short_frames_sum_kernel_8_byte_records(gpu):  # spp < 16: sum_kernel<2>
    _accumulate(gpu, "scene_08", 33, 17, 8, [4] * 5)


@pytest.mark.parametrize("spp,jit", [(16, False), (32, False), (16, "wait")])
def test_full_blocks_sum_nib_kernel(gpu, spp, jit):  # 32: two blocks, the last one as sub-blocks
    _accumulate(gpu, "scene_08", 33, 17, 8, [spp] * 4, scene_jit=jit)


def test_deferred_12_byte_records(gpu):  # 43 primitives with a plane: sum_kernel<3>, deferred records
    _accumulate(gpu, "scene_01", 33, 17, 8, [2] * 4)


def test_colour_records_at_update_shape(gpu):  # depth 50: sum_kernel<3> adds colours; update()'s frame
    _accumulate(gpu, "builtin0", 32, 24, 50, [1] * 6)


def test_bvh_class_records(gpu):  # sum_nib_kernel reads the attenuation-class table
    _accumulate(gpu, "cubes100", 33, 17, 8, [16] * 3)


def test_frames_of_different_spp_add_up(gpu):  # the resolve kernel changes from frame to frame
    comp = _accumulate(gpu, "scene_08", 33, 17, 8, [1, 4, 16, 2])
    assert comp.n == 23


def test_multi_pass_frames(gpu, monkeypatch):
    """FR_PIPELINE=3: a 64-spp frame's four blocks in passes; `running` carries S between them
    and only the last pass touches the accumulator."""
    monkeypatch.setenv("FR_PIPELINE", "3")
    ctx = gpu.RenderContext(0)
    _accumulate(gpu, "scene_08", 33, 17, 8, [64] * 3, ctx=ctx)
    assert ctx.sync()["trace_launches"] >= 2
    ctx.close()


@pytest.mark.parametrize("pipe", [None, "2"])
def test_streamed_frames(gpu, pipe, monkeypatch):
    """Six frames enqueued with no sync between them (frame slots; pipe "2": overlapping
    traces): the sum stream alone orders the accumulator's read-modify-writes."""
    if pipe is None:
        monkeypatch.delenv("FR_FRAME_PIPE", raising=False)
    else:
        monkeypatch.setenv("FR_FRAME_PIPE", pipe)
    key, w, h, spp, depth = "scene_08", 33, 17, 16, 8
    sc = _product_scene(gpu, key, w, h)
    comp = Composite()
    frames = [_oracle_frame(key, w, h, spp, depth, SEED0 + k) for k in range(6)]
    for omean, _, _, _ in frames:
        want_mean, want_u8 = comp.add(_frame_sum(omean, spp), spp)
    ctx = gpu.RenderContext(0)
    for k in range(6):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate=True))
    assert ctx.accum_info() == (6, 96)  # host-side, before any sync
    st = ctx.sync()
    mean, u8 = ctx.download(w, h)
    assert _same_bits(mean, want_mean) and np.array_equal(u8, want_u8)
    assert (st["segments"], st["hits"]) == frames[-1][2:]
    ctx.close()


def test_first_frame_is_the_plain_render(gpu):
    for key, w, h, spp, depth in (("scene_08", 33, 17, 37, 8), ("builtin0", 32, 24, 1, 50), ("scene_01", 33, 17, 3, 8)):
        sc = _product_scene(gpu, key, w, h)
        ref, ref_u8, ref_st = gpu.render(sc, sc.camera, w, h, spp, depth, seed=5)
        ctx = gpu.RenderContext(0)
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, 5, accumulate=True))
        st = ctx.sync()
        mean, u8 = ctx.download(w, h)
        assert _same_bits(mean, ref) and np.array_equal(u8, ref_u8), key
        assert (st["segments"], st["hits"]) == (ref_st["segments"], ref_st["hits"])
        assert ctx.accum_info() == (1, spp)
        ctx.close()


def test_restarts(gpu):
    """A camera orbit, a scene edit, another size, another depth and accum_reset each start a new
    accumulation: the next frame equals its plain render, and the one after continues it."""
    spp = 2
    state = {"w": 32, "h": 24, "depth": 8}
    sc = _product_scene(gpu, "builtin0", 32, 24)
    cam = sc.camera
    ctx = gpu.RenderContext(0)
    seed = [100]

    def frame():
        seed[0] += 1
        w, h, depth = state["w"], state["h"], state["depth"]
        ctx.render(sc, cam, gpu.make_params(w, h, spp, depth, seed[0], accumulate=True))
        ctx.sync()
        return ctx.download(w, h), gpu.render(sc, cam, w, h, spp, depth, seed=seed[0])

    def orbit():
        gpu.camera_orbit(cam, (0.3, 0.1, 0.0))

    def edit():
        sc.translate(0, (-1.0, 0.0, 0.0))

    def resize():
        state.update(w=33, h=17)

    def deepen():
        state.update(depth=9)

    causes = [("first", lambda: None), ("orbit", orbit), ("scene_translate", edit), ("size", resize), ("depth", deepen),
              ("accum_reset", ctx.accum_reset)]
    for name, cause in causes:
        cause()
        if name == "accum_reset":
            assert ctx.accum_info() == (0, 0)
        (mean, u8), (ref, ref_u8, _) = frame()
        assert _same_bits(mean, ref) and np.array_equal(u8, ref_u8), name
        assert ctx.accum_info() == (1, spp), name
        (mean, u8), (ref, _, _) = frame()  # continues: no longer the plain render of its own seed
        assert ctx.accum_info() == (2, 2 * spp), name
        assert not _same_bits(mean, ref), name
    ctx.close()


def test_plain_render_in_between_leaves_the_accumulation_alone(gpu):
    key, w, h, spp, depth = "scene_08", 33, 17, 4, 8
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    comp = Composite()
    for k in range(2):
        omean, _, _, _ = _oracle_frame(key, w, h, spp, depth, SEED0 + k)
        want_mean, want_u8 = comp.add(_frame_sum(omean, spp), spp)
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate=True))
        ctx.sync()
        if k == 0:  # save_image between two update() calls: another seed and spp, no flag
            pmean, pu8, _, _ = _oracle_frame(key, w, h, 16, depth, 77)
            ctx.render(sc, sc.camera, gpu.make_params(w, h, 16, depth, 77))
            ctx.sync()
            mean, u8 = ctx.download(w, h)
            assert _same_bits(mean, pmean) and np.array_equal(u8, pu8)
            assert ctx.accum_info() == (1, spp)
    mean, u8 = ctx.download(w, h)
    assert _same_bits(mean, want_mean) and np.array_equal(u8, want_u8)
    assert ctx.accum_info() == (2, 2 * spp)
    ctx.close()


def test_multi_context_accumulates_like_one_context(gpu):
    key, w, h, spp, depth = "scene_08", 33, 17, 4, 8  # three strips: shard 0 has two, shard 1 one
    sc = _product_scene(gpu, key, w, h)
    m = gpu.MultiContext([0, 0])
    assert m.accum_info() == (0, 0)
    comp = Composite()
    for k in range(3):
        omean, _, osegs, ohits = _oracle_frame(key, w, h, spp, depth, SEED0 + k)
        want_mean, want_u8 = comp.add(_frame_sum(omean, spp), spp)
        m.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate=True))
        st = m.sync()
        mean, u8 = m.frame()
        assert _same_bits(mean, want_mean) and np.array_equal(u8, want_u8), k
        assert (st["segments"], st["hits"]) == (osegs, ohits)
        assert m.accum_info() == (k + 1, (k + 1) * spp)
        assert [m.context(i).accum_info() for i in range(2)] == [m.accum_info()] * 2
    m.accum_reset()
    assert m.accum_info() == (0, 0) and m.context(1).accum_info() == (0, 0)
    m.close()


def test_errors(gpu):
    w, h = 32, 24
    sc = _product_scene(gpu, "builtin0", w, h)
    ctx = gpu.RenderContext(0)
    with pytest.raises(gpu.ForMaError) as e:
        ctx.render(sc, sc.camera, gpu.make_params(w, h, 2, 50, accumulate=True, mt_bands=True))
    assert e.value.code == gpu.FR_EARG and "FR_FLAG_MT_BANDS" in str(e.value)
    assert ctx.accum_info() == (0, 0)
    ctx.close()
    p = gpu.make_params(w, h, 2, 8, accumulate=True)
    mean = np.zeros((h, w, 3), np.float32)
    rc = gpu.lib().fr_render_hip(sc._h, C.byref(sc.camera), C.byref(p), 0, mean.ctypes.data_as(C.POINTER(C.c_float)),
                                 None, None)
    assert rc == gpu.FR_EARG and b"FR_FLAG_ACCUMULATE" in gpu.lib().fr_last_error()
    rc = gpu.lib().fr_render_hip_multi(sc._h, C.byref(sc.camera), C.byref(p), 1,
                                       mean.ctypes.data_as(C.POINTER(C.c_float)), None, None)
    assert rc == gpu.FR_EARG


def test_prepare_sets_the_accumulator_up_and_changes_no_state(gpu):
    key, w, h, spp, depth = "scene_08", 33, 17, 4, 8
    sc = _product_scene(gpu, key, w, h)
    big = _product_scene(gpu, key, 64, 40)
    ctx = gpu.RenderContext(0)
    ctx.prepare(sc, sc.camera, gpu.make_params(w, h, spp, depth, accumulate=True))
    assert ctx.accum_info() == (0, 0)
    comp = _accumulate(gpu, key, w, h, depth, [spp] * 2, ctx=ctx, sc=sc)
    # a larger frame prepared in the middle grows the accumulator; what it holds goes on
    ctx.prepare(big, big.camera, gpu.make_params(64, 40, spp, depth, accumulate=True))
    assert ctx.accum_info() == (2, 2 * spp)
    _accumulate(gpu, key, w, h, depth, [spp], ctx=ctx, sc=sc, comp=comp)  # the third frame of the same accumulation
    assert comp.frames == 3
    ctx.close()


def test_update_converges_while_no_key_is_pressed(gpu):
    w, h = 32, 24
    m = gpu.create_model(w, h)
    ocam = O.camera_new(w, h)
    comp = Composite()
    d = (C.c_float * 3)()
    for frame in range(5):
        pix = gpu.update(m, 0, 0.1, accumulate=True)
        gpu.check(gpu.lib().fr_update_delta(0, 0.1, d))
        O.camera_orbit(ocam, list(d))  # the first call moves the camera to its orbit; the others leave it there
        assert np.array_equal(m.scene.camera.to_array(), O.camera_to_array(ocam))
        seed = m.seed ^ (0x9E3779B97F4A7C15 * (frame + 1) & 0xFFFFFFFFFFFFFFFF)
        omean, _, ocnt, _ = O.render(S.BUILTIN[0](), ocam, w, h, 1, 50, seed=seed)
        _, want_u8 = comp.add(_frame_sum(omean, 1), 1)
        assert np.array_equal(pix.reshape(h, w, 3), want_u8), frame
        assert m.ctx.accum_info() == (frame + 1, frame + 1)
        assert (m.last_stats["segments"], m.last_stats["hits"]) == (ocnt["segments"], ocnt["hits"])
    pix = gpu.update(m, 0b001000, 0.1, accumulate=True)  # a key press moves the camera: a new accumulation
    gpu.check(gpu.lib().fr_update_delta(0b001000, 0.1, d))
    O.camera_orbit(ocam, list(d))
    seed = m.seed ^ (0x9E3779B97F4A7C15 * 6 & 0xFFFFFFFFFFFFFFFF)
    _, ou8, _, _ = O.render(S.BUILTIN[0](), ocam, w, h, 1, 50, seed=seed)
    assert np.array_equal(pix.reshape(h, w, 3), ou8)
    assert m.ctx.accum_info() == (1, 1)
    pix = gpu.update(m, 0b001000, 0.1)  # the default: a plain frame, the accumulation untouched
    assert m.ctx.accum_info() == (1, 1)
    m.close()


@pytest.mark.parametrize("spp", [3, 37])
def test_spp_that_is_no_power_of_two(gpu, spp):
    """Extra evidence beside the exact cases. The oracle's mean is RN(S / spp), so S recovered
    as RN(mean * spp) carries at most two roundings (relative 2^-23); K frames of such sums,
    all non-negative, added in f32 and divided once more: the composite built from them is
    within (K + 2) * 2^-23 of the device's, relatively, per channel, and equal where it is 0."""
    key, w, h, depth, frames = "scene_08", 33, 17, 8, 3
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    a = None
    for k in range(frames):
        omean, _, osegs, ohits = _oracle_frame(key, w, h, spp, depth, SEED0 + k)
        assert (omean >= 0).all()
        s = (omean * np.float32(spp)).astype(np.float32)
        a = s if a is None else (a + s).astype(np.float32)
        want = (a / np.float32((k + 1) * spp)).astype(np.float32)
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate=True))
        st = ctx.sync()
        mean, _ = ctx.download(w, h)
        bound = (frames + 2) * 2.0 ** -23
        err = np.abs(mean.astype(np.float64) - want.astype(np.float64))
        print(f"spp {spp} frame {k}: max relative error {float(np.max(err / np.maximum(want, 1e-30))):.3g} "
              f"(bound {bound:.3g})")
        assert (err <= bound * want.astype(np.float64)).all(), k
        assert np.array_equal(mean[want == 0], want[want == 0])
        assert ctx.accum_info() == (k + 1, (k + 1) * spp)
        assert (st["segments"], st["hits"]) == (osegs, ohits)
    ctx.close()
