"""Python host mirror of fo-rma's tracer API over libforma_rt's C ABI.

Same names, argument meaning and failure behaviour as the reference's operator
API in cpu_ray_tracer/tracer.rs (paths relative to the reference root):

    create_model(width, height)          tracer.rs:19-28
    update(model, keys, delta_time)      tracer.rs:30-55   (orbit camera + 1-spp frame)
    save_image(model, sample, path)      tracer.rs:160-187 (sample spp, PNG)
    TraceModel                           tracer.rs:12-17

and the Hitable plugin API (shapes/hitable.rs:4-14): Sphere / Plane / Box objects
with translate()/rotate(), flattened into the ordered primitive list the GPU
kernel consumes. Rendering always runs the HIP kernel: if libforma_rt.so or a
GPU is missing this module raises — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# FORMA_RT_LIB selects another build of the same ABI (used for A/B kernel variants)
LIB_PATH = os.environ.get("FORMA_RT_LIB") or os.path.join(HERE, "libforma_rt.so")
SCENES_DIR = os.path.join(HERE, "scenes")

FR_ABI_VERSION = 6  # include/forma_rt.h FR_ABI_VERSION
FR_OK, FR_EARG, FR_EPARSE, FR_EHIP, FR_ENODEV, FR_ENOMEM = 0, -1, -2, -3, -4, -5
FR_SPHERE, FR_PLANE, FR_AABB, FR_OBB, FR_STUB, FR_TRIANGLE = 0, 1, 2, 3, 4, 5
FR_LAMBERTIAN, FR_METAL, FR_DIELECTRIC, FR_LIGHT = 0, 1, 2, 3
FR_FLAG_WRITE_U8 = 1
FR_FLAG_MT_BANDS = 2  # save_image_mt semantics (forma_rt.h)
FR_FLAG_SCENE_JIT = 4  # scene-specialised trace kernel (hiprtc, cached; same image bits)
FR_FLAG_SCENE_JIT_WAIT = 8  # ... compiled on the render's thread when missing (else in the background)
FR_FLAG_SCENE_JIT_CACHED = 16  # ... only when already built or on disk; never compiled (one-shot callers)
FR_FLAG_ACCUMULATE = 32  # the frame's sum joins the context's accumulator; outputs show the running mean
# with FR_FLAG_ACCUMULATE: the accumulation also carries Q (sum of S^2 / spp), for accum_error()
FR_FLAG_ACCUM_ERROR = 64
# with both: the frame traces only the tiles of the context's active tile list (RenderContext.adapt)
FR_FLAG_ADAPTIVE = 128
FR_ERR_FLOOR = 2.0 ** -7  # the relative error's smallest denominator (forma_rt.h)
# fr_ctx_denoise (forma_rt.h): the defaults, the edge-stopping floor and the validity caps
FR_DN_LEVELS_DEFAULT, FR_DN_K_DEFAULT = 4, 4.0
FR_DN_EPS, FR_DN_MEAN_MAX, FR_DN_VAR_MAX = 2.0 ** -20, 2.0 ** 40, 2.0 ** 80
# fr_ctx_gbuffer / fr_ctx_denoise_guided (forma_rt.h): the miss id, the feature and albedo caps
# and the guide's defaults
FR_GBUFFER_MISS = 0xFFFFFFFF
FR_DN_FEAT_MAX, FR_DN_NORMAL_MAX, FR_DN_ALB_MIN, FR_DN_ALB_MAX = 2.0 ** 40, 2.0 ** 10, 2.0 ** -6, 2.0 ** 6
FR_DN_SIGMA_Z_DEFAULT, FR_DN_NORMAL_POW2_DEFAULT = 2.0 ** -5, 4
# fr_ctx_temporal (forma_rt.h): the source map's "none", the reason codes, the defaults
FR_TP_NONE = 0xFFFFFFFF
(FR_TP_REUSED, FR_TP_NO_HISTORY, FR_TP_MISS, FR_TP_OFFSCREEN, FR_TP_ID, FR_TP_NORMAL, FR_TP_PLANE,
 FR_TP_HISTORY) = range(8)
FR_TP_N_MAX_DEFAULT, FR_TP_N_MAX_SPECULAR_DEFAULT, FR_TP_N_MAX_MAX = 32.0, 4.0, 2.0 ** 24
FR_TP_SIGMA_Z_DEFAULT, FR_TP_NORMAL_MIN_DEFAULT = 2.0 ** -5, float(np.float32(0.9))
FR_JIT_OFF, FR_JIT_USED, FR_JIT_PENDING, FR_JIT_FAILED, FR_JIT_MISS = 0, 1, 2, 3, 4  # fr_ctx_jit_state
MAX_DEPTH = 50  # tracer.rs:10
DEFAULT_SEED = 0x5EED


class ForMaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libforma_rt error {code}: {msg}")
        self.code = code


class FrPrim(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("material", C.c_uint32), ("color", C.c_float * 3), ("fuzz", C.c_float),
                ("g", C.c_float * 16)]


class FrCamera(C.Structure):
    _fields_ = [(n, C.c_float * 3) for n in ("position", "lower_left", "horizontal", "vertical", "u", "v", "w")] + [
        (n, C.c_float) for n in ("aspect", "lens_radius", "focus_dist", "radius", "rotation")]

    def to_array(self):
        vals = []
        for n in ("position", "lower_left", "horizontal", "vertical", "u", "v", "w"):
            vals.extend(getattr(self, n))
        vals += [self.aspect, self.lens_radius, self.focus_dist, self.radius, self.rotation]
        return np.asarray(vals, dtype=np.float32)


class FrParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("max_depth", C.c_uint32),
                ("seed", C.c_uint64), ("strip_rows", C.c_uint32), ("shard_index", C.c_uint32),
                ("shard_count", C.c_uint32), ("flags", C.c_uint32)]


class FrStats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("hits", C.c_uint64), ("samples", C.c_uint64), ("prim_tests", C.c_uint64),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("trace_ms", C.c_double),
                ("trace_launches", C.c_uint32), ("occupancy", C.c_uint32), ("scatters", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrAccumError(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("samples", C.c_uint32), ("pixels", C.c_uint64), ("converged", C.c_uint64),
                ("max_rel", C.c_float), ("threshold", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrAdaptInfo(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("samples", C.c_uint32), ("tiles", C.c_uint32), ("active_tiles", C.c_uint32),
                ("pixels", C.c_uint64), ("active_pixels", C.c_uint64), ("converged", C.c_uint64),
                ("max_rel", C.c_float), ("threshold", C.c_float), ("min_samples", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class FrDenoiseGuide(C.Structure):
    _fields_ = [("sigma_z", C.c_float), ("normal_pow2", C.c_uint32), ("demodulate", C.c_uint32), ("pad", C.c_uint32)]


class FrTemporal(C.Structure):
    _fields_ = [("n_max", C.c_float), ("n_max_specular", C.c_float), ("sigma_z", C.c_float), ("normal_min", C.c_float),
                ("pad", C.c_uint32 * 4)]


class FrRay(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("pad0", C.c_float), ("d", C.c_float * 3), ("pad1", C.c_float)]


class FrCastInfo(C.Structure):
    _fields_ = [("n", C.c_uint32), ("tree", C.c_uint32), ("waves_tree", C.c_uint32), ("waves_list", C.c_uint32)]


class FrOcclInfo(C.Structure):
    _fields_ = [("n", C.c_uint32), ("tree", C.c_uint32), ("waves_tree", C.c_uint32), ("waves_list", C.c_uint32),
                ("occluded", C.c_uint32), ("pad", C.c_uint32 * 3)]


class FrSceneInfo(C.Structure):
    _fields_ = [("last_sync", C.c_uint32), ("prims_patched", C.c_uint32), ("nodes_refit", C.c_uint32),
                ("refit_launches", C.c_uint32), ("packs", C.c_uint64), ("refits", C.c_uint64),
                ("version", C.c_uint64), ("edit_seq", C.c_uint64), ("host_ms", C.c_float), ("h2d_ms", C.c_float),
                ("patch_ms", C.c_float), ("refit_ms", C.c_float), ("has_tree", C.c_uint32), ("n_nodes", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# moving scenes (forma_rt.h): fr_scene_update's flag, what a use did to the device copy, the tables
FR_UPDATE_REBUILD = 1
FR_SCENE_SYNC_NONE, FR_SCENE_SYNC_PACK, FR_SCENE_SYNC_REFIT = 0, 1, 2
FR_TABLE_RECORDS, FR_TABLE_LEAF_RECORDS, FR_TABLE_LEAF_ORDER, FR_TABLE_NODES = 0, 1, 2, 3
FR_TABLE_SLOT_BOUNDS, FR_TABLE_NODE_UNIONS = 4, 5
_TABLES = {"records": 0, "leaf_records": 1, "leaf_order": 2, "nodes": 3, "slot_bounds": 4, "node_unions": 5}

# fr_ctx_cast / fr_ctx_occluded flags (forma_rt.h)
FR_CAST_LIST = 1
FR_CAST_RAYS_DEVICE = 2
FR_CAST_TMAX = 16  # (4 stays an unknown flag: fr_ctx_cast has refused it since it was built)
FR_CAST_OUT_DEVICE = 8


# Every symbol include/forma_rt.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "fr_last_error", "fr_abi_version", "fr_device_count",
    "fr_scene_create", "fr_scene_builtin", "fr_scene_from_json", "fr_scene_free", "fr_scene_count",
    "fr_scene_get_prims", "fr_scene_translate", "fr_scene_rotate",
    "fr_camera_init", "fr_camera_look", "fr_camera_orbit", "fr_camera_translate", "fr_update_delta",
    "fr_ctx_create", "fr_ctx_free", "fr_ctx_render", "fr_ctx_sync", "fr_ctx_download", "fr_ctx_download_async",
    "fr_ctx_wait", "fr_ctx_device_buffers", "fr_host_alloc", "fr_host_free", "fr_ctx_trace_log",
    "fr_ctx_trace_log_read", "fr_mctx_create", "fr_mctx_free", "fr_mctx_count", "fr_mctx_ctx", "fr_mctx_render",
    "fr_mctx_sync", "fr_mctx_frame", "fr_mctx_download",
    "fr_render_hip", "fr_render_hip_multi", "fr_selftest_ops", "fr_selftest_rng", "fr_selftest_recip",
    "fr_selftest_div",
    "fr_post_process", "fr_post_process_device", "fr_rgb_to_rgba_device", "fr_ctx_jit_info", "fr_selftest_jit",
    "fr_ctx_prepare", "fr_ctx_jit_state", "fr_jit_wait",
    "fr_ctx_accum_reset", "fr_ctx_accum_info", "fr_mctx_accum_reset", "fr_mctx_accum_info",
    "fr_ctx_accum_error", "fr_ctx_download_error", "fr_mctx_accum_error",
    "fr_ctx_adapt", "fr_ctx_download_counts", "fr_mctx_adapt",
    "fr_ctx_denoise", "fr_ctx_download_denoised", "fr_ctx_denoised_buffers",
    "fr_ctx_gbuffer", "fr_ctx_download_gbuffer", "fr_ctx_denoise_guided",
    "fr_camera_axial", "fr_ctx_camera_path", "fr_selftest_camray", "fr_selftest_boxinv",
    "fr_ctx_temporal", "fr_ctx_temporal_reset", "fr_ctx_download_temporal",
    "fr_ctx_gbuffer_info", "fr_camera_pixel_ray", "fr_ctx_cast", "fr_ctx_download_hits", "fr_ctx_cast_info",
    "fr_ctx_hit_buffers", "fr_ctx_occluded", "fr_ctx_download_occluded", "fr_ctx_occluded_info",
    "fr_scene_update", "fr_scene_rebuild", "fr_ctx_scene_info", "fr_scene_download_table",
)

_lib = None


def _load_torch_runtime_first():
    # If torch is importable, load it first so this library binds the same
    # libamdhip64 (soname libamdhip64.so.7) as torch: one HIP runtime per process.
    # FR_NO_TORCH=1 skips it (a short-lived profiled child that never imports torch).
    if os.environ.get("FR_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib():
    """Load libforma_rt.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ForMaError(FR_ENODEV, f"{LIB_PATH} not built; run __graft_entry__.build() or make -C fo-rma_amd")
    _load_torch_runtime_first()
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp = C.c_void_p
    f3 = P(C.c_float)
    L.fr_last_error.restype = C.c_char_p
    L.fr_abi_version.restype = C.c_int
    L.fr_device_count.argtypes = [P(C.c_int)]
    L.fr_scene_create.argtypes = [P(FrPrim), C.c_uint32, P(vp)]
    L.fr_scene_builtin.argtypes = [C.c_int, C.c_uint32, C.c_uint32, P(vp), P(FrCamera)]
    L.fr_scene_from_json.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, P(vp), P(FrCamera)]
    L.fr_scene_free.argtypes = [vp]
    L.fr_scene_free.restype = None
    L.fr_scene_count.argtypes = [vp]
    L.fr_scene_count.restype = C.c_uint32
    L.fr_scene_get_prims.argtypes = [vp, P(FrPrim), C.c_uint32]
    L.fr_scene_translate.argtypes = [vp, C.c_uint32, f3]
    L.fr_scene_rotate.argtypes = [vp, C.c_uint32, f3]
    L.fr_camera_init.argtypes = [P(FrCamera), C.c_uint32, C.c_uint32]
    L.fr_camera_look.argtypes = [P(FrCamera), f3, f3, f3, C.c_float, C.c_float, C.c_uint32, C.c_uint32]
    L.fr_camera_orbit.argtypes = [P(FrCamera), f3]
    L.fr_camera_translate.argtypes = [P(FrCamera), f3]
    L.fr_update_delta.argtypes = [C.c_uint8, C.c_float, f3]
    L.fr_ctx_create.argtypes = [C.c_int, vp, P(vp)]
    L.fr_ctx_free.argtypes = [vp]
    L.fr_ctx_free.restype = None
    L.fr_ctx_render.argtypes = [vp, vp, P(FrCamera), P(FrParams)]
    L.fr_ctx_sync.argtypes = [vp, P(FrStats)]
    L.fr_ctx_download.argtypes = [vp, f3, P(C.c_uint8)]
    L.fr_ctx_device_buffers.argtypes = [vp, P(vp), P(vp)]
    if hasattr(L, "fr_ctx_download_async"):  # absent from A/B builds of older sources
        L.fr_ctx_download_async.argtypes = [vp, f3, P(C.c_uint8)]
        L.fr_ctx_wait.argtypes = [vp]
        L.fr_host_alloc.argtypes = [C.c_size_t, P(vp)]
        L.fr_host_free.argtypes = [vp]
        L.fr_host_free.restype = None
    if hasattr(L, "fr_mctx_create"):  # absent from A/B builds of older sources
        L.fr_ctx_trace_log.argtypes = [vp, C.c_int]
        L.fr_ctx_trace_log_read.argtypes = [vp, C.c_int, P(C.c_double), C.c_uint32, P(C.c_uint32)]
        L.fr_mctx_create.argtypes = [P(C.c_int), C.c_int, P(vp)]
        L.fr_mctx_free.argtypes = [vp]
        L.fr_mctx_free.restype = None
        L.fr_mctx_count.argtypes = [vp]
        L.fr_mctx_ctx.argtypes = [vp, C.c_int, P(vp)]
        L.fr_mctx_render.argtypes = [vp, vp, P(FrCamera), P(FrParams)]
        L.fr_mctx_sync.argtypes = [vp, P(FrStats)]
        L.fr_mctx_frame.argtypes = [vp, P(P(C.c_float)), P(P(C.c_uint8))]
        L.fr_mctx_download.argtypes = [vp, f3, P(C.c_uint8)]
    L.fr_render_hip.argtypes = [vp, P(FrCamera), P(FrParams), C.c_int, f3, P(C.c_uint8), P(FrStats)]
    L.fr_render_hip_multi.argtypes = [vp, P(FrCamera), P(FrParams), C.c_int, f3, P(C.c_uint8), P(FrStats)]
    L.fr_selftest_ops.argtypes = [C.c_int, C.c_int, f3, f3, C.c_uint32, f3]
    L.fr_selftest_rng.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32)]
    if hasattr(L, "fr_post_process"):  # absent from A/B builds of older sources
        L.fr_post_process.argtypes = [C.c_int, P(C.c_int), C.c_uint32, C.c_float, C.c_uint32, C.c_uint32,
                                      P(C.c_uint8), P(C.c_uint8)]
        L.fr_post_process_device.argtypes = [vp, P(C.c_int), C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, vp, vp]
        L.fr_rgb_to_rgba_device.argtypes = [vp, vp, vp, C.c_size_t]
    if hasattr(L, "fr_selftest_recip"):  # absent from A/B builds of older sources
        L.fr_selftest_recip.argtypes = [C.c_int, C.c_uint64, C.c_uint64, P(C.c_uint64), P(C.c_uint32)]
    if hasattr(L, "fr_selftest_div"):  # absent from A/B builds of older sources
        L.fr_selftest_div.argtypes = [C.c_int, C.c_uint32, C.c_uint32, P(C.c_uint64), P(C.c_uint64)]
    if hasattr(L, "fr_ctx_jit_info"):  # absent from A/B builds of older sources
        L.fr_ctx_jit_info.argtypes = [vp, P(C.c_int), P(C.c_double), P(C.c_int)]
        L.fr_ctx_prepare.argtypes = [vp, vp, P(FrCamera), P(FrParams)]
    if hasattr(L, "fr_ctx_jit_state"):  # absent from A/B builds of older sources
        L.fr_ctx_jit_state.argtypes = [vp, P(C.c_int)]
        L.fr_jit_wait.argtypes = []
        L.fr_selftest_jit.argtypes = [C.c_char_p, P(C.c_uint32), C.c_uint32, P(C.c_int), P(C.c_size_t), P(C.c_double)]
    if hasattr(L, "fr_ctx_accum_info"):  # absent from A/B builds of older sources
        L.fr_ctx_accum_reset.argtypes = [vp]
        L.fr_ctx_accum_info.argtypes = [vp, P(C.c_uint32), P(C.c_uint32)]
        L.fr_mctx_accum_reset.argtypes = [vp]
        L.fr_mctx_accum_info.argtypes = [vp, P(C.c_uint32), P(C.c_uint32)]
    if hasattr(L, "fr_ctx_accum_error"):  # absent from A/B builds of older sources
        L.fr_ctx_accum_error.argtypes = [vp, C.c_float, P(FrAccumError)]
        L.fr_ctx_download_error.argtypes = [vp, f3]
        L.fr_mctx_accum_error.argtypes = [vp, C.c_float, P(FrAccumError), f3]
    if hasattr(L, "fr_ctx_adapt"):  # absent from A/B builds of older sources
        L.fr_ctx_adapt.argtypes = [vp, C.c_float, C.c_uint32, P(FrAdaptInfo)]
        L.fr_ctx_download_counts.argtypes = [vp, P(C.c_uint32), P(C.c_uint32)]
        L.fr_mctx_adapt.argtypes = [vp, C.c_float, C.c_uint32, P(FrAdaptInfo)]
    if hasattr(L, "fr_ctx_denoise"):  # absent from A/B builds of older sources
        L.fr_ctx_denoise.argtypes = [vp, C.c_uint32, C.c_float]
        L.fr_ctx_download_denoised.argtypes = [vp, f3, P(C.c_uint8), f3]
        L.fr_ctx_denoised_buffers.argtypes = [vp, P(vp), P(vp)]
    if hasattr(L, "fr_camera_axial"):  # absent from A/B builds of older sources
        L.fr_camera_axial.argtypes = [P(FrCamera)]
        L.fr_ctx_camera_path.argtypes = [vp, P(C.c_int)]
        L.fr_selftest_camray.argtypes = [C.c_int, P(FrCamera), f3, C.c_uint32, P(C.c_uint32)]
    if hasattr(L, "fr_selftest_boxinv"):
        L.fr_selftest_boxinv.argtypes = [C.c_int, f3, C.c_uint32, P(C.c_uint32)]
    if hasattr(L, "fr_ctx_gbuffer"):
        L.fr_ctx_gbuffer.argtypes = [vp, vp, P(FrCamera), C.c_uint32, C.c_uint32]
        L.fr_ctx_download_gbuffer.argtypes = [vp, P(C.c_uint32), f3, f3, f3, f3]
        L.fr_ctx_denoise_guided.argtypes = [vp, C.c_uint32, C.c_float, P(FrDenoiseGuide)]
    if hasattr(L, "fr_ctx_temporal"):
        L.fr_ctx_temporal.argtypes = [vp, C.c_uint32, C.c_float, P(FrDenoiseGuide), P(FrTemporal)]
        L.fr_ctx_temporal_reset.argtypes = [vp]
        L.fr_ctx_download_temporal.argtypes = [vp] + [f3] * 8 + [P(C.c_uint32)] * 2
    if hasattr(L, "fr_ctx_cast"):
        L.fr_ctx_gbuffer_info.argtypes = [vp, P(C.c_int)]
        L.fr_camera_pixel_ray.argtypes = [P(FrCamera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(FrRay)]
        L.fr_ctx_cast.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32]
        L.fr_ctx_download_hits.argtypes = [vp, P(C.c_uint32), f3, f3, f3, f3]
        L.fr_ctx_cast_info.argtypes = [vp, P(FrCastInfo)]
    if hasattr(L, "fr_ctx_occluded"):
        L.fr_ctx_hit_buffers.argtypes = [vp, P(vp), P(vp), P(vp), P(C.c_uint32)]
        L.fr_ctx_occluded.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp]
        L.fr_ctx_download_occluded.argtypes = [vp, vp]
        L.fr_ctx_occluded_info.argtypes = [vp, P(FrOcclInfo)]
    if hasattr(L, "fr_scene_update"):
        L.fr_scene_update.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32]
        L.fr_scene_rebuild.argtypes = [vp]
        L.fr_ctx_scene_info.argtypes = [vp, vp, P(FrSceneInfo)]
        L.fr_scene_download_table.argtypes = [vp, C.c_int, C.c_uint32, vp, C.c_size_t, P(C.c_size_t)]
    _lib = L
    return L


def check(rc):
    if rc != FR_OK:
        raise ForMaError(rc, lib().fr_last_error().decode(errors="replace"))
    return rc


def _f3(v):
    return (C.c_float * 3)(*[float(np.float32(x)) for x in v])


def device_count():
    n = C.c_int(0)
    rc = lib().fr_device_count(C.byref(n))
    return n.value if rc == FR_OK else 0


# ---- Hitable plugin objects (shapes/hitable.rs:4-14) ------------------------

class Hitable:
    """Base of the tracer's shapes. translate/rotate are no-ops unless a shape
    overrides them (hitable.rs:12-13)."""
    kind = FR_STUB

    def __init__(self, material=0, color=(0.0, 0.0, 0.0), fuzz=0.0):
        self.material, self.color, self.fuzz = int(material), tuple(color), float(fuzz)

    def geometry(self):
        return ()

    def translate(self, v):
        pass

    def rotate(self, v):
        pass

    def to_prim(self):
        p = FrPrim()
        p.kind, p.material, p.fuzz = self.kind, self.material, self.fuzz
        for i in range(3):
            p.color[i] = self.color[i]
        for i, g in enumerate(self.geometry()):
            p.g[i] = g
        return p


class Sphere(Hitable):
    """shapes/sphere.rs: Sphere::new(center, radius, material, color, fuzz)"""
    kind = FR_SPHERE

    def __init__(self, center, radius, material, color, fuzz):
        super().__init__(material, color, fuzz)
        self.center, self.radius = tuple(center), float(radius)

    def geometry(self):
        return tuple(self.center) + (self.radius,)


class Plane(Hitable):
    """shapes/plane.rs: Plane::new(position, orientation, size, material, color, fuzz)"""
    kind = FR_PLANE

    def __init__(self, position, orientation, size, material, color, fuzz):
        super().__init__(material, color, fuzz)
        self.position, self.orientation, self.size = tuple(position), tuple(orientation), tuple(size)

    def geometry(self):
        return tuple(self.position) + tuple(self.orientation) + tuple(self.size)

    def translate(self, v):  # plane.rs:62-64
        self.position = tuple(v)

    def rotate(self, v):  # plane.rs:66-68
        self.orientation = tuple(v)


class Box(Hitable):
    """The build's axis-aligned box (FR_AABB), given by min/max corners."""
    kind = FR_AABB

    def __init__(self, mn, mx, material, color, fuzz):
        super().__init__(material, color, fuzz)
        self.mn, self.mx = tuple(mn), tuple(mx)

    def geometry(self):
        return tuple(self.mn) + tuple(self.mx)


class Triangle(Hitable):
    """The build's triangle (FR_TRIANGLE), vertices v0, v1, v2 in winding order."""
    kind = FR_TRIANGLE

    def __init__(self, v0, v1, v2, material, color, fuzz):
        super().__init__(material, color, fuzz)
        self.v = (tuple(v0), tuple(v1), tuple(v2))

    def geometry(self):
        return self.v[0] + self.v[1] + self.v[2]


class Stub(Hitable):
    """shapes/aabb.rs / rectangle.rs: never hit, never scatter."""
    kind = FR_STUB


# ---- scenes and cameras -----------------------------------------------------

def _prim_of(p):
    """FrPrim of a dict with kind / material / color / fuzz / g."""
    q = FrPrim()
    q.kind, q.material, q.fuzz = p["kind"], p["material"], float(p["fuzz"])
    for k in range(3):
        q.color[k] = float(p["color"][k])
    for k in range(16):
        q.g[k] = float(p["g"][k])
    return q


class Scene:
    """An ordered primitive list on the host plus its resident device copies
    (cpu_ray_tracer/scene.rs:4-7)."""

    def __init__(self, handle, camera=None):
        self._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self.camera = camera

    @classmethod
    def from_objects(cls, objects, camera=None):
        arr = (FrPrim * max(1, len(objects)))(*[o.to_prim() for o in objects])
        h = C.c_void_p()
        check(lib().fr_scene_create(arr, len(objects), C.byref(h)))
        return cls(h, camera)

    @classmethod
    def from_prims(cls, prims, camera=None):
        """prims: sequence of FrPrim (or dicts with kind/material/color/fuzz/g)"""
        arr = (FrPrim * max(1, len(prims)))()
        for i, p in enumerate(prims):
            if isinstance(p, FrPrim):
                arr[i] = p
            else:
                arr[i].kind, arr[i].material, arr[i].fuzz = p["kind"], p["material"], float(p["fuzz"])
                for k in range(3):
                    arr[i].color[k] = float(p["color"][k])
                for k in range(16):
                    arr[i].g[k] = float(p["g"][k])
        h = C.c_void_p()
        check(lib().fr_scene_create(arr, len(prims), C.byref(h)))
        return cls(h, camera)

    @classmethod
    def builtin(cls, which, width, height):
        """0 get_simple_scene, 1 get_plane_scene, 2 get_objects (scenes.rs), 3 simple
        scene in the interactive frontend's state. Camera = Camera::new(w, h)."""
        h, cam = C.c_void_p(), FrCamera()
        check(lib().fr_scene_builtin(which, width, height, C.byref(h), C.byref(cam)))
        return cls(h, cam)

    @classmethod
    def from_json(cls, text, width, height):
        if isinstance(text, str):
            text = text.encode()
        h, cam = C.c_void_p(), FrCamera()
        check(lib().fr_scene_from_json(text, len(text), width, height, C.byref(h), C.byref(cam)))
        return cls(h, cam)

    @classmethod
    def from_file(cls, path, width, height):
        with open(path, "rb") as f:
            return cls.from_json(f.read(), width, height)

    def __len__(self):
        return lib().fr_scene_count(self._h)

    def prims(self):
        n = len(self)
        arr = (FrPrim * max(1, n))()
        check(lib().fr_scene_get_prims(self._h, arr, n))
        return [arr[i] for i in range(n)]

    def translate(self, index, v):
        check(lib().fr_scene_translate(self._h, index, _f3(v)))

    def rotate(self, index, v):
        check(lib().fr_scene_rotate(self._h, index, _f3(v)))

    def update(self, indices, prims_or_objects, rebuild=False):
        """Replace primitives (fr_scene_update): indices None means 0..n-1. prims_or_objects holds
        FrPrim, Hitable objects or oracle-style dicts, or is an [n, 22] uint32 array of fr_prim
        words. A geometric edit is caught up in place on the device; rebuild=True forces the
        full re-pack."""
        if isinstance(prims_or_objects, np.ndarray):
            words = np.ascontiguousarray(prims_or_objects, np.uint32).reshape(-1, 22)
            n, pptr = len(words), words.ctypes.data
        else:
            items = list(prims_or_objects)
            n = len(items)
            arr = (FrPrim * max(1, n))()
            for i, p in enumerate(items):
                arr[i] = p if isinstance(p, FrPrim) else p.to_prim() if isinstance(p, Hitable) else _prim_of(p)
            pptr = C.addressof(arr)
        idx = None
        if indices is not None:
            idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
            if len(idx) != n:
                raise ValueError(f"update: {len(idx)} indices for {n} primitives")
        check(lib().fr_scene_update(self._h, idx.ctypes.data if idx is not None and n else None, pptr if n else None, n,
                                    FR_UPDATE_REBUILD if rebuild else 0))

    def set_spheres(self, indices, centers, radii=None):
        """Move the spheres at `indices` (None: primitives 0..n-1) to `centers` [n, 3], with new
        `radii` [n] if given: one fr_scene_update of the list's own primitives with the geometry
        replaced, formed in numpy."""
        centers = np.asarray(centers, np.float32).reshape(-1, 3)
        n = len(centers)
        count = len(self)
        idx = np.arange(n, dtype=np.uint32) if indices is None else np.ascontiguousarray(indices, np.uint32).reshape(-1)
        if len(idx) != n or (n and int(idx.max()) >= count):
            raise ValueError("set_spheres: indices do not match the centers or the scene")
        words = np.zeros((max(1, count), 22), np.uint32)
        check(lib().fr_scene_get_prims(self._h, words.ctypes.data_as(C.POINTER(FrPrim)), count))
        sel = words[idx]
        if n and not (sel[:, 0] == FR_SPHERE).all():
            raise ValueError("set_spheres: a listed primitive is not a sphere")
        sel[:, 6:9] = centers.view(np.uint32)
        if radii is not None:
            sel[:, 9] = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (n,))).view(np.uint32)
        self.update(idx, sel)

    def rebuild(self):
        """The next use packs and builds the scene again (fr_scene_rebuild)."""
        check(lib().fr_scene_rebuild(self._h))

    def download_table(self, device, which):
        """One table of the device copy as a uint32 array [rows, words per row] (diagnostics; waits):
        "records", "leaf_records", "nodes" (16 words), "leaf_order" (1), "slot_bounds", "node_unions" (8)."""
        w = _TABLES[which] if isinstance(which, str) else int(which)
        size = C.c_size_t(0)
        check(lib().fr_scene_download_table(self._h, device, w, None, 0, C.byref(size)))
        out = np.zeros(size.value // 4, np.uint32)
        check(lib().fr_scene_download_table(self._h, device, w, out.ctypes.data, out.nbytes, C.byref(size)))
        return out.reshape(-1, {2: 1, 4: 8, 5: 8}.get(w, 16))

    def close(self):
        if self._h and self._h.value:
            lib().fr_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_new(width, height):
    cam = FrCamera()
    check(lib().fr_camera_init(C.byref(cam), width, height))
    return cam


def camera_look(frm, at, vup, fov, aperture, width, height):
    cam = FrCamera()
    check(lib().fr_camera_look(C.byref(cam), _f3(frm), _f3(at), _f3(vup), float(fov), float(aperture), width,
                               height))
    return cam


def camera_orbit(cam, delta):
    check(lib().fr_camera_orbit(C.byref(cam), _f3(delta)))
    return cam


def camera_translate(cam, delta):
    check(lib().fr_camera_translate(C.byref(cam), _f3(delta)))
    return cam


def pixel_ray(cam, x, y, width, height):
    """(o [3], d [3]) f32: the pinhole ray of pixel (x, y) of the view, gbuffer()'s
    (fr_camera_pixel_ray). Needs no device."""
    r = FrRay()
    check(lib().fr_camera_pixel_ray(C.byref(cam), int(x), int(y), int(width), int(height), C.byref(r)))
    return np.array(list(r.o), dtype=np.float32), np.array(list(r.d), dtype=np.float32)


def scene_path(name):
    """Path of a bundled scene file (the reference's scenes/*.json, re-serialised)."""
    return os.path.join(SCENES_DIR, f"{name}.min.json")


# ---- rendering ----------------------------------------------------------------

def make_params(width, height, spp, max_depth=MAX_DEPTH, seed=DEFAULT_SEED, shard_index=0, shard_count=1,
                write_u8=True, mt_bands=False, scene_jit=False, accumulate=False):
    """scene_jit: False, True (the scene kernel once it is compiled; until then renders run
    the compiled-in kernel, same bits), "wait" (compile on the render's thread if needed) or
    "cached" (the scene kernel only if already built or on disk; never a compile).
    accumulate: FR_FLAG_ACCUMULATE, the frame refines the context's accumulation of this view
    (forma_rt.h); give every frame its own seed. accumulate="error": FR_FLAG_ACCUM_ERROR as
    well, the accumulation carries what accum_error() needs (same picture).
    accumulate="adaptive": FR_FLAG_ADAPTIVE on top of both, the frame traces only the tiles of
    the context's active tile list (RenderContext.adapt) and leaves every other pixel as it is."""
    p = FrParams()
    p.width, p.height, p.spp, p.max_depth, p.seed = width, height, spp, max_depth, seed
    p.strip_rows, p.shard_index, p.shard_count = 8, shard_index, shard_count
    p.flags = ((FR_FLAG_WRITE_U8 if write_u8 else 0) | (FR_FLAG_MT_BANDS if mt_bands else 0) |
               (FR_FLAG_SCENE_JIT if scene_jit else 0) | (FR_FLAG_SCENE_JIT_WAIT if scene_jit == "wait" else 0) |
               (FR_FLAG_SCENE_JIT_CACHED if scene_jit == "cached" else 0) | (FR_FLAG_ACCUMULATE if accumulate else 0) |
               (FR_FLAG_ACCUM_ERROR if isinstance(accumulate, str) and accumulate in ("error", "adaptive") else 0) |
               (FR_FLAG_ADAPTIVE if isinstance(accumulate, str) and accumulate == "adaptive" else 0))
    return p


def jit_wait():
    """Block until no scene-kernel compile is queued or running in this process."""
    check(lib().fr_jit_wait())


class _PinnedBlock:
    """One fr_host_alloc allocation. Freed when the last reference goes: every numpy view
    made by _pinned_views holds one (through its ctypes buffer), so an array a caller kept
    never points at freed memory."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        check(lib().fr_host_alloc(max(1, nbytes), C.byref(self.ptr)))
        self.nbytes = nbytes

    def __del__(self):
        try:
            if self.ptr and self.ptr.value:
                lib().fr_host_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def _pinned_views(block, width, height):
    n = width * height * 3
    buf = (C.c_uint8 * block.nbytes).from_address(block.ptr.value)
    buf._owner = block  # the buffer (the arrays' base) keeps the allocation alive
    mean = np.frombuffer(buf, dtype=np.float32, count=n).reshape(height, width, 3)
    u8 = np.frombuffer(buf, dtype=np.uint8, count=n, offset=n * 4).reshape(height, width, 3)
    return mean, u8


class PinnedFrame:
    """Full-image host buffers in page-locked memory (fr_host_alloc): mean [H, W, 3] f32
    and u8 [H, W, 3], the targets of RenderContext.download_async. close() drops the
    frame's own views; the memory is returned once no view of it is left anywhere."""

    def __init__(self, width, height):
        self.width, self.height = width, height
        self._block = _PinnedBlock(width * height * 3 * 5)
        self.mean, self.u8 = _pinned_views(self._block, width, height)

    def close(self):
        self.mean = self.u8 = None
        self._block = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RenderContext:
    """One device, one HIP stream, resident output buffers (fr_ctx)."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        check(lib().fr_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = device

    def render(self, scene, cam, params):
        check(lib().fr_ctx_render(self._h, scene._h, C.byref(cam), C.byref(params)))
        if params.flags & FR_FLAG_ACCUMULATE:
            self._accum_shape = (params.height, params.width)

    def sync(self):
        st = FrStats()
        check(lib().fr_ctx_sync(self._h, C.byref(st)))
        return st.as_dict()

    def download(self, width, height, mean=None, u8=None):
        mean = np.full((height, width, 3), np.nan, dtype=np.float32) if mean is None else mean
        u8 = np.zeros((height, width, 3), dtype=np.uint8) if u8 is None else u8
        check(lib().fr_ctx_download(self._h, mean.ctypes.data_as(C.POINTER(C.c_float)),
                                    u8.ctypes.data_as(C.POINTER(C.c_uint8))))
        return mean, u8

    def download_into(self, mean=None, u8=None):
        """Copy the last render's strips into caller-owned full-image arrays (either may be
        None: that output is not copied). Page-locked arrays (PinnedFrame) copy by DMA."""
        fp = None if mean is None else mean.ctypes.data_as(C.POINTER(C.c_float))
        up = None if u8 is None else u8.ctypes.data_as(C.POINTER(C.c_uint8))
        check(lib().fr_ctx_download(self._h, fp, up))

    def download_async(self, frame):
        """Enqueue the last render's D2H gather into `frame` (a PinnedFrame); returns at
        once. The copies finish before wait() returns and before the next render writes
        its outputs; the next render's trace kernel overlaps them."""
        check(lib().fr_ctx_download_async(self._h, frame.mean.ctypes.data_as(C.POINTER(C.c_float)),
                                          frame.u8.ctypes.data_as(C.POINTER(C.c_uint8))))

    def wait(self):
        """Block until every render and download enqueued on this context has finished."""
        check(lib().fr_ctx_wait(self._h))

    def prepare(self, scene, cam, params):
        """Set up everything a render of `params` needs (scene copy, buffers, and with
        scene_jit the scene-specialised kernel) without rendering; returns jit_info()."""
        check(lib().fr_ctx_prepare(self._h, scene._h, C.byref(cam), C.byref(params)))
        return self.jit_info()

    def jit_info(self):
        """The last render's trace kernel: {"used": scene-specialised kernel ran, "ms": time
        that render spent getting it (compile or cache load), "compiled": hiprtc ran}."""
        used, ms, comp = C.c_int(0), C.c_double(0.0), C.c_int(0)
        check(lib().fr_ctx_jit_info(self._h, C.byref(used), C.byref(ms), C.byref(comp)))
        return {"used": bool(used.value), "ms": ms.value, "compiled": bool(comp.value), "state": self.jit_state()}

    def accum_reset(self):
        """The next accumulating frame (make_params(accumulate=True)) starts a new accumulation."""
        check(lib().fr_ctx_accum_reset(self._h))

    def accum_info(self):
        """(frames, samples per pixel) in the accumulator as of the last enqueued frame; (0, 0)
        when there is none. No sync."""
        frames, samples = C.c_uint32(0), C.c_uint32(0)
        check(lib().fr_ctx_accum_info(self._h, C.byref(frames), C.byref(samples)))
        return frames.value, samples.value

    def accum_error(self, threshold, want_map=False):
        """The error estimate of the live accumulation (frames rendered with
        make_params(accumulate="error"), two or more): a dict of frames, samples, pixels,
        converged (pixels whose relative standard error is <= threshold), max_rel and
        threshold. Waits for the frames enqueued so far. want_map: (summary, rel) with rel the
        [H, W] f32 map, rows of other shards NaN."""
        e = FrAccumError()
        check(lib().fr_ctx_accum_error(self._h, float(threshold), C.byref(e)))
        if not want_map:
            return e.as_dict()
        return e.as_dict(), self.download_error()

    def download_error(self, rel=None):
        """The map of the last accum_error() as [H, W] f32: this shard's rows are written into
        `rel` (a new NaN-filled array when None; the shape is the last accumulating frame's)."""
        if rel is None:
            rel = np.full(self._err_shape(), np.nan, dtype=np.float32)
        check(lib().fr_ctx_download_error(self._h, rel.ctypes.data_as(C.POINTER(C.c_float))))
        return rel

    def adapt(self, threshold, min_samples=0):
        """Builds the context's active tile list from the error estimate of the live
        accumulation (fr_ctx_adapt): an 8x8 tile is active iff one of its pixels has a relative
        standard error > threshold or the tile holds fewer than min_samples samples per pixel.
        Frames of make_params(accumulate="adaptive") then trace those tiles only. A dict of
        frames, samples, tiles, active_tiles, pixels, active_pixels, converged, max_rel,
        threshold and min_samples. Waits for the frames enqueued so far; download_error() gives
        the map it used, download_counts() the per-pixel sample counts."""
        e = FrAdaptInfo()
        check(lib().fr_ctx_adapt(self._h, float(threshold), int(min_samples), C.byref(e)))
        return e.as_dict()

    def download_counts(self, samples=None, frames=None):
        """(samples, frames): the per-pixel sample and frame counts of the live accumulation as
        [H, W] uint32, this shard's rows written into the arrays given (new zero-filled ones
        when None; the shape is the last accumulating frame's)."""
        if samples is None:
            samples = np.zeros(self._err_shape(), dtype=np.uint32)
        if frames is None:
            frames = np.zeros(self._err_shape(), dtype=np.uint32)
        check(lib().fr_ctx_download_counts(self._h, samples.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           frames.ctypes.data_as(C.POINTER(C.c_uint32))))
        return samples, frames

    def denoise(self, levels=FR_DN_LEVELS_DEFAULT, k=FR_DN_K_DEFAULT, guided=False, sigma_z=FR_DN_SIGMA_Z_DEFAULT,
                normal_pow2=FR_DN_NORMAL_POW2_DEFAULT, demodulate=True):
        """Enqueues the variance-guided filter of the live accumulation (fr_ctx_denoise: frames
        of make_params(accumulate="error") or "adaptive", two or more, shard_count 1) and
        returns at once: `levels` a-trous levels (1 to 6, steps 1, 2, 4, ...) with edge-stopping
        scale k (0 < k <= 1024). The result describes the accumulation as of the call;
        download_denoised() waits for it. The frames' own outputs are untouched.
        guided: the feature-guided filter instead (fr_ctx_denoise_guided), steered also by the
        G-buffer of the same scene, camera and size (gbuffer() first): sigma_z in (0, 1024]
        scales the plane-distance weight by the depth, the normal weight is the clamped dot
        product to the power 2^normal_pow2 (0 to 8), demodulate filters the colour divided by
        the first hit's albedo. The three are ignored without guided."""
        if not guided:
            check(lib().fr_ctx_denoise(self._h, int(levels), float(k)))
            return
        g = FrDenoiseGuide(float(sigma_z), int(normal_pow2), int(demodulate), 0)
        check(lib().fr_ctx_denoise_guided(self._h, int(levels), float(k), C.byref(g)))

    def gbuffer(self, scene, cam, width, height):
        """Enqueues the first-hit feature pass of the view (fr_ctx_gbuffer) and returns at once:
        per pixel the pinhole primary ray's closest primitive, its root, normal, point and
        albedo. Renders, the accumulation and their outputs are untouched. A scene with a tree is
        walked through it (gbuffer_info() says which walk ran); the bits are the list loop's."""
        check(lib().fr_ctx_gbuffer(self._h, scene._h, C.byref(cam), int(width), int(height)))

    def download_gbuffer(self, width, height):
        """The last gbuffer() as a dict: "prim" [H, W] uint32 (FR_GBUFFER_MISS for a miss),
        "depth" [H, W] f32, "normal", "position" and "albedo" [H, W, 3] f32. Waits for it."""
        out = {"prim": np.zeros((height, width), dtype=np.uint32), "depth": np.zeros((height, width), dtype=np.float32)}
        for name in ("normal", "position", "albedo"):
            out[name] = np.zeros((height, width, 3), dtype=np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        check(lib().fr_ctx_download_gbuffer(self._h, out["prim"].ctypes.data_as(C.POINTER(C.c_uint32)), fp(out["depth"]),
                                            fp(out["normal"]), fp(out["position"]), fp(out["albedo"])))
        return out

    def scene_info(self, scene):
        """What this context's last use of `scene` did to its device copy (fr_ctx_scene_info): a dict
        with last_sync (FR_SCENE_SYNC_*), prims_patched, nodes_refit, refit_launches, packs, refits."""
        info = FrSceneInfo()
        check(lib().fr_ctx_scene_info(self._h, scene._h, C.byref(info)))
        return info.as_dict()

    def gbuffer_info(self):
        """"tree" or "list": the walk the last gbuffer() took (fr_ctx_gbuffer_info). No wait."""
        t = C.c_int(0)
        check(lib().fr_ctx_gbuffer_info(self._h, C.byref(t)))
        return "tree" if t.value else "list"

    @staticmethod
    def _rays(who, origins, directions, t_max):
        """(a [n, 8] f32 array or torch tensor to keep alive, its address, n, flags) of a query's
        rays: origins and directions numpy [n, 3] with t_max None, a scalar or an [n] array, or
        origins a torch [n, 8] device tensor (directions None) with t_max None or True (column 7)."""
        if directions is None and hasattr(origins, "data_ptr"):
            t = origins
            if t.dim() != 2 or t.shape[1] != 8 or str(t.dtype) != "torch.float32" or not t.is_cuda or not t.is_contiguous():
                raise ForMaError(FR_EARG, f"{who}: device rays must be a contiguous float32 [n, 8] tensor on the device")
            if t_max is not None and t_max is not True and t_max is not False:
                raise ForMaError(FR_EARG, f"{who}: t_max of device rays is True (column 7 holds it) or None")
            return t, t.data_ptr(), int(t.shape[0]), FR_CAST_RAYS_DEVICE | (FR_CAST_TMAX if t_max else 0)
        o = np.ascontiguousarray(origins, dtype=np.float32)
        d = np.ascontiguousarray(directions, dtype=np.float32)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ForMaError(FR_EARG, f"{who}: origins and directions must be [n, 3] arrays of one length")
        n = int(o.shape[0])
        rays = np.zeros((n, 8), dtype=np.float32)
        rays[:, 0:3] = o
        rays[:, 4:7] = d
        flags = 0
        if t_max is not None:
            tm = np.asarray(t_max, dtype=np.float32)
            if tm.ndim > 1 or (tm.ndim == 1 and tm.shape[0] != n):
                raise ForMaError(FR_EARG, f"{who}: t_max must be a scalar or an [n] array")
            rays[:, 7] = tm
            flags = FR_CAST_TMAX
        return rays, rays.ctypes.data, n, flags

    def cast(self, scene, origins, directions=None, list_walk=False, t_max=None):
        """The closest hit of each ray (fr_ctx_cast, fr_ctx_download_hits): origins and directions
        numpy [n, 3] f32 arrays, or origins a torch tensor [n, 8] f32 on the context's device
        holding (o, pad, d, pad) per row, complete on the device at the call (directions None).
        list_walk: the list in order even if the scene has a tree. t_max: each ray's range
        (FR_CAST_TMAX), a scalar or an [n] array; for a device tensor True, and column 7 holds it.
        None: FLT_MAX, and the pad is ignored. Returns download_gbuffer()'s
        dict with "t" for "depth": "prim" [n] uint32 (FR_GBUFFER_MISS for a miss), "t" [n] f32,
        "normal", "position" and "albedo" [n, 3] f32. Waits for the hits."""
        keep, addr, n, flags = self._rays("cast", origins, directions, t_max)
        check(lib().fr_ctx_cast(self._h, scene._h, C.c_void_p(addr), n, flags | (FR_CAST_LIST if list_walk else 0)))
        del keep
        return self.download_hits(n)

    def occluded(self, scene, origins, directions=None, t_max=None, list_walk=False, out=None):
        """Whether anything of the scene lies within (0.001, t_max) of each ray (fr_ctx_occluded):
        rays and t_max as cast()'s. Returns an [n] bool numpy array, or, with out a contiguous
        torch.uint8 [n] tensor on the context's device, fills it with 0 / 1 on the device, waits and
        returns it."""
        keep, addr, n, flags = self._rays("occluded", origins, directions, t_max)
        flags |= FR_CAST_LIST if list_walk else 0
        if out is not None:
            if (not hasattr(out, "data_ptr") or out.dim() != 1 or out.shape[0] != n or str(out.dtype) != "torch.uint8"
                    or not out.is_cuda or not out.is_contiguous()):
                raise ForMaError(FR_EARG, "occluded: out must be a contiguous uint8 [n] tensor on the device")
            check(lib().fr_ctx_occluded(self._h, scene._h, C.c_void_p(addr), n, flags | FR_CAST_OUT_DEVICE,
                                        C.c_void_p(out.data_ptr())))
            check(lib().fr_ctx_download_occluded(self._h, None))  # the wait
            del keep
            return out
        check(lib().fr_ctx_occluded(self._h, scene._h, C.c_void_p(addr), n, flags, None))
        del keep
        return self.download_occluded(n)

    def visible(self, scene, a, b):
        """[n] bool: nothing of the scene lies between the points a and b ([n, 3] each):
        ~occluded() of the rays o = a, d = b - a (in f32) with t_max = 1."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        with np.errstate(all="ignore"):
            d = (b - a).astype(np.float32)
        return ~self.occluded(scene, a, d, t_max=1.0)

    def download_occluded(self, n):
        """The last occluded()'s n answers as an [n] bool array. Waits for them."""
        i = FrOcclInfo()
        check(lib().fr_ctx_occluded_info(self._h, C.byref(i)))
        if n != i.n:
            raise ForMaError(FR_EARG, f"download_occluded: the last query had {i.n} rays, not {n}")
        got = np.zeros(n, dtype=np.uint8)
        check(lib().fr_ctx_download_occluded(self._h, got.ctypes.data_as(C.c_void_p)))
        return got != 0

    def occluded_info(self):
        """The last occluded() as a dict: cast_info()'s fields and "occluded", the number of
        occluded rays counted on the device. Waits for it."""
        i = FrOcclInfo()
        check(lib().fr_ctx_occluded_info(self._h, C.byref(i)))
        return {"n": i.n, "tree": i.tree, "waves_tree": i.waves_tree, "waves_list": i.waves_list, "occluded": i.occluded}

    def hit_buffers(self):
        """(g0, g1, alb, n): the device addresses of the last cast()'s hits, three arrays of n
        16-byte words (normal xyz, t), (position xyz, prim bits), (albedo rgb, 0), and n
        (fr_ctx_hit_buffers). Waits for nothing: sync through cast_info() or download_hits()."""
        g0, g1, alb, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32(0)
        check(lib().fr_ctx_hit_buffers(self._h, C.byref(g0), C.byref(g1), C.byref(alb), C.byref(n)))
        return g0.value, g1.value, alb.value, n.value

    def download_hits(self, n):
        """The last cast()'s n hits as cast() returns them. Waits for them."""
        out = {"prim": np.zeros(n, dtype=np.uint32), "t": np.zeros(n, dtype=np.float32)}
        for name in ("normal", "position", "albedo"):
            out[name] = np.zeros((n, 3), dtype=np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        check(lib().fr_ctx_download_hits(self._h, out["prim"].ctypes.data_as(C.POINTER(C.c_uint32)), fp(out["t"]),
                                         fp(out["normal"]), fp(out["position"]), fp(out["albedo"])))
        return out

    def cast_info(self):
        """The last cast() as a dict: "n", "tree" (1: the scene's tree was walked) and the waves of
        64 rays that walked the tree ("waves_tree") or fell back to the list ("waves_list")."""
        i = FrCastInfo()
        check(lib().fr_ctx_cast_info(self._h, C.byref(i)))
        return {"n": i.n, "tree": i.tree, "waves_tree": i.waves_tree, "waves_list": i.waves_list}

    def pick(self, scene, cam, x, y, width, height):
        """The list index of the primitive under pixel (x, y) of the view, or None."""
        o, d = pixel_ray(cam, x, y, width, height)
        prim = int(self.cast(scene, o[None, :], d[None, :])["prim"][0])
        return None if prim == FR_GBUFFER_MISS else prim

    def download_denoised(self, width, height, want_var=False):
        """(mean [H, W, 3] f32, u8 [H, W, 3]) of the last denoise(), with want_var also the
        [H, W] f32 variance map the filter steered by (not an error estimate of the filtered
        picture). Waits for it."""
        mean = np.full((height, width, 3), np.nan, dtype=np.float32)
        u8 = np.zeros((height, width, 3), dtype=np.uint8)
        var = np.full((height, width), np.nan, dtype=np.float32) if want_var else None
        check(lib().fr_ctx_download_denoised(self._h, mean.ctypes.data_as(C.POINTER(C.c_float)),
                                             u8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             var.ctypes.data_as(C.POINTER(C.c_float)) if want_var else None))
        return (mean, u8, var) if want_var else (mean, u8)

    def download_denoised_into(self, u8):
        """Copy the last denoise()'s u8 image into a caller-owned [H, W, 3] array (page-locked
        arrays copy by DMA). Waits for it."""
        check(lib().fr_ctx_download_denoised(self._h, None, u8.ctypes.data_as(C.POINTER(C.c_uint8)), None))

    def denoised_buffers(self):
        """(d_mean_rgb, d_rgb8) device addresses of the last denoise()'s mean and u8 image."""
        dm, du = C.c_void_p(), C.c_void_p()
        check(lib().fr_ctx_denoised_buffers(self._h, C.byref(dm), C.byref(du)))
        return dm.value, du.value

    def temporal(self, levels=FR_DN_LEVELS_DEFAULT, k=FR_DN_K_DEFAULT, guide=None, n_max=FR_TP_N_MAX_DEFAULT,
                 n_max_specular=FR_TP_N_MAX_SPECULAR_DEFAULT, sigma_z=FR_TP_SIGMA_Z_DEFAULT,
                 normal_min=FR_TP_NORMAL_MIN_DEFAULT):
        """Enqueues temporal reuse of the live accumulation (fr_ctx_temporal: frames of
        make_params(accumulate="error") or "adaptive", one or more, shard_count 1, and the
        gbuffer() of the same scene, camera and size) and returns at once. On the first call of
        a new accumulation the previous view's totals are reprojected into a per-pixel prior
        (n_max / n_max_specular cap its samples, sigma_z and normal_min accept a source); every
        call adds the prior to the accumulation, keeps the totals as the view's history and
        shows them: levels 0 as they are, 1 to 6 through denoise()'s levels with scale k.
        guide: None for the unguided levels, True for the guided ones at their defaults, or a
        dict of denoise()'s sigma_z, normal_pow2 and demodulate. The results land in denoise()'s
        buffers (download_denoised)."""
        g = None
        if guide is not None and guide is not False:
            kw = {} if guide is True else dict(guide)
            g = FrDenoiseGuide(float(kw.pop("sigma_z", FR_DN_SIGMA_Z_DEFAULT)),
                               int(kw.pop("normal_pow2", FR_DN_NORMAL_POW2_DEFAULT)), int(kw.pop("demodulate", True)), 0)
            if kw:
                raise TypeError(f"guide: unknown keys {sorted(kw)}")
        o = FrTemporal(float(n_max), float(n_max_specular), float(sigma_z), float(normal_min))
        check(lib().fr_ctx_temporal(self._h, int(levels), float(k), C.byref(g) if g is not None else None, C.byref(o)))

    def temporal_reset(self):
        """Drops the temporal history: the next temporal() starts with an empty prior."""
        check(lib().fr_ctx_temporal_reset(self._h))

    def download_temporal(self, width, height):
        """The last temporal() as a dict: "prior_a", "prior_q", "total_a", "total_q" [H, W, 3] f32,
        "prior_n", "prior_k", "total_n", "total_k" [H, W] f32, "source" [H, W] uint32 (y0 W + x0 or
        FR_TP_NONE) and "reason" [H, W] uint32 (FR_TP_*). Waits for it."""
        out = {}
        for kind in ("prior", "total"):
            for name, shape in (("a", (height, width, 3)), ("q", (height, width, 3)), ("n", (height, width)),
                                ("k", (height, width))):
                out[f"{kind}_{name}"] = np.full(shape, np.nan, dtype=np.float32)
        out["source"] = np.zeros((height, width), dtype=np.uint32)
        out["reason"] = np.zeros((height, width), dtype=np.uint32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check(lib().fr_ctx_download_temporal(
            self._h, *[fp(out[f"{kind}_{name}"]) for kind in ("prior", "total") for name in ("a", "q", "n", "k")],
            up(out["source"]), up(out["reason"])))
        return out

    def _err_shape(self):
        shape = getattr(self, "_accum_shape", None)
        if shape is None:
            raise ForMaError(FR_EARG, "download_error: pass `rel` ([H, W] f32) on a context that rendered elsewhere")
        return shape

    def camera_path(self):
        """"axial" when the last render (or prepare) generated its camera rays by the short
        form of an axis-aligned camera, else "general" (fr_ctx_camera_path)."""
        a = C.c_int(0)
        check(lib().fr_ctx_camera_path(self._h, C.byref(a)))
        return "axial" if a.value else "general"

    def jit_state(self):
        """FR_JIT_OFF / USED / PENDING / FAILED for the last render (fr_ctx_jit_state)."""
        s = C.c_int(0)
        check(lib().fr_ctx_jit_state(self._h, C.byref(s)))
        return s.value

    def trace_log(self, enable=True):
        """Start (or stop) logging every trace-kernel launch's HIP-event duration."""
        check(lib().fr_ctx_trace_log(self._h, 1 if enable else 0))

    def trace_log_read(self, frames=False, timeline=False, temporal=False, cast=False):
        """HIP-event durations (ms) logged since trace_log(True): every trace-kernel launch,
        or (frames=True) every whole render (trace + sum kernels). timeline=True: (start, end)
        pairs instead, in ms from the first logged trace launch's start. temporal=True: the
        stages of every temporal() call, three durations per call: the prior, totals and prep,
        the picture. cast=True: every cast kernel and G-buffer pass."""
        which = 5 if cast else 4 if temporal else (1 if frames else 0) + (2 if timeline else 0)
        n = C.c_uint32(0)
        check(lib().fr_ctx_trace_log_read(self._h, which, None, 0, C.byref(n)))
        k = 2 if timeline else 1
        arr = (C.c_double * max(1, k * n.value))()
        check(lib().fr_ctx_trace_log_read(self._h, which, arr, k * n.value, C.byref(n)))
        if timeline:
            return [(arr[2 * i], arr[2 * i + 1]) for i in range(n.value)]
        return [arr[i] for i in range(n.value)]

    def device_buffers(self):
        """(d_mean_rgb, d_rgb8) device addresses of the last render's full-image outputs."""
        dm, du = C.c_void_p(), C.c_void_p()
        check(lib().fr_ctx_device_buffers(self._h, C.byref(dm), C.byref(du)))
        return dm.value, du.value

    def close(self):
        if getattr(self, "_borrowed", False):
            return
        if self._h and self._h.value:
            lib().fr_ctx_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiContext:
    """fr_mctx: one fr_ctx per entry of `devices` (entries may repeat), shard i of n of
    every frame on entry i, the strips gathered asynchronously into one page-locked host
    frame. Persistent: frames of the same size allocate nothing (tracer.rs:83-134's row
    tiling, one device per shard instead of one thread)."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._h = C.c_void_p()
        check(lib().fr_mctx_create(devs, len(devices), C.byref(self._h)))
        self.devices = list(devices)
        self._shape = None

    def render(self, scene, cam, params):
        """Enqueue one frame (all shards and their gathers); returns at once."""
        check(lib().fr_mctx_render(self._h, scene._h, C.byref(cam), C.byref(params)))
        self._shape = (params.height, params.width, 3)

    def sync(self):
        st = FrStats()
        check(lib().fr_mctx_sync(self._h, C.byref(st)))
        return st.as_dict()

    def frame(self):
        """(mean, u8) numpy copies of the host frame of the last render (after sync)."""
        fp, up = C.POINTER(C.c_float)(), C.POINTER(C.c_uint8)()
        check(lib().fr_mctx_frame(self._h, C.byref(fp), C.byref(up)))
        n = self._shape[0] * self._shape[1] * 3
        mean = np.ctypeslib.as_array(fp, shape=(n,)).reshape(self._shape).copy()
        u8 = np.ctypeslib.as_array(up, shape=(n,)).reshape(self._shape).copy()
        return mean, u8

    def frame_ptrs(self):
        """Host addresses of the page-locked frame (mean, u8)."""
        fp, up = C.POINTER(C.c_float)(), C.POINTER(C.c_uint8)()
        check(lib().fr_mctx_frame(self._h, C.byref(fp), C.byref(up)))
        return C.cast(fp, C.c_void_p).value, C.cast(up, C.c_void_p).value

    def accum_reset(self):
        """Every shard's next accumulating frame starts a new accumulation."""
        check(lib().fr_mctx_accum_reset(self._h))

    def accum_info(self):
        """(frames, samples per pixel) accumulated: shard 0's figures, which every shard shares."""
        frames, samples = C.c_uint32(0), C.c_uint32(0)
        check(lib().fr_mctx_accum_info(self._h, C.byref(frames), C.byref(samples)))
        return frames.value, samples.value

    def accum_error(self, threshold, want_map=False):
        """RenderContext.accum_error over every shard: pixels and converged are the shards'
        sums, max_rel their maximum; want_map: (summary, the whole [H, W] f32 map)."""
        e = FrAccumError()
        rel = np.full(self._shape[:2], np.nan, dtype=np.float32) if want_map else None
        check(lib().fr_mctx_accum_error(self._h, float(threshold), C.byref(e),
                                        rel.ctypes.data_as(C.POINTER(C.c_float)) if want_map else None))
        return (e.as_dict(), rel) if want_map else e.as_dict()

    def adapt(self, threshold, min_samples=0):
        """RenderContext.adapt over every shard: the counts are the shards' sums, max_rel their
        maximum, frames and samples the largest of the shards'."""
        e = FrAdaptInfo()
        check(lib().fr_mctx_adapt(self._h, float(threshold), int(min_samples), C.byref(e)))
        return e.as_dict()

    def context(self, i):
        """The i-th shard's RenderContext view (not owned: do not close it)."""
        h = C.c_void_p()
        check(lib().fr_mctx_ctx(self._h, i, C.byref(h)))
        rc = RenderContext.__new__(RenderContext)
        rc._h, rc.device, rc._borrowed = h, self.devices[i], True
        return rc

    def close(self):
        if self._h and self._h.value:
            lib().fr_mctx_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_converged(ctx, scene, cam, w, h, spp, max_depth, seed, target, fraction=1.0, max_frames=64, check_every=1,
                     scene_jit=False, adaptive=False, min_samples=0):
    """Accumulating frames of `spp` samples on `ctx` (frame k = 1, 2, ... has seed `seed + k`)
    until, at a checked frame k >= 2 (every check_every-th), converged >= fraction * pixels for
    the relative standard error `target` (accum_error), or max_frames are done. Starts a new
    accumulation. Returns (mean[H,W,3] f32, u8[H,W,3], the last summary, or None if none was
    taken).
    adaptive: the check is adapt(target, min_samples) and the frames after it trace only the
    tiles it found active; it also stops when no tile is active. The summary is then adapt()'s,
    with "traced": the samples traced in all frames (the sum of their stats' samples; a uniform
    run traces pixels * samples)."""
    ctx.accum_reset()
    summary = None
    mode = "error"
    uniform_frames, traced, per_frame = 0, 0, None  # per_frame: samples an adaptive frame traces
    for k in range(1, max_frames + 1):
        ctx.render(scene, cam, make_params(w, h, spp, max_depth, seed + k, accumulate=mode, scene_jit=scene_jit))
        if per_frame is None:
            uniform_frames += 1
        else:
            traced += per_frame
        if k >= 2 and k % check_every == 0:
            if adaptive:
                summary = ctx.adapt(target, min_samples)
                mode = "adaptive"
                per_frame = summary["active_pixels"] * spp
                if summary["active_tiles"] == 0:
                    break
            else:
                summary = ctx.accum_error(target)
            if summary["converged"] >= fraction * summary["pixels"]:
                break
    ctx.sync()
    mean, u8 = ctx.download(w, h)
    if adaptive and summary is not None:
        summary["traced"] = traced + uniform_frames * summary["pixels"] * spp
    return mean, u8, summary


def render(scene, cam, width, height, spp, max_depth=MAX_DEPTH, seed=DEFAULT_SEED, device=0, shard_index=0,
           shard_count=1, n_gpus=1, mt_bands=False, scene_jit=False):
    """Render on the GPU. Returns (mean[H,W,3] f32, u8[H,W,3], stats). Rows outside the
    shard are NaN / 0. n_gpus > 1 row-shards the whole image across devices 0..n-1.
    mt_bands: save_image_mt semantics (mean then holds the u8 average, 0..255).
    scene_jit: the scene-specialised trace kernel (FR_FLAG_SCENE_JIT; same bits)."""
    mean = np.full((height, width, 3), np.nan, dtype=np.float32)
    u8 = np.zeros((height, width, 3), dtype=np.uint8)
    st = FrStats()
    p = make_params(width, height, spp, max_depth, seed, shard_index, shard_count, mt_bands=mt_bands,
                    scene_jit=scene_jit)
    fm, fu = mean.ctypes.data_as(C.POINTER(C.c_float)), u8.ctypes.data_as(C.POINTER(C.c_uint8))
    if n_gpus > 1:
        check(lib().fr_render_hip_multi(scene._h, C.byref(cam), C.byref(p), n_gpus, fm, fu, C.byref(st)))
    else:
        check(lib().fr_render_hip(scene._h, C.byref(cam), C.byref(p), device, fm, fu, C.byref(st)))
    return mean, u8, st.as_dict()


# ---- post-process effects (src/shaders/compute/*.wgsl) -------------------------

EFFECTS = ["none", "noise", "pixelate", "invert_color", "wave", "interlace", "flipaxis", "grayscale", "step",
           "watercolor", "chromostereopsis", "anaglyph"]  # shader_utils.rs:58-88 order and names


def post_process(rgba, effects, time=0.0, device=0):
    """Run the effect chain (post_processor.rs:101-129) on an [H, W, 4] uint8 image (or an
    [H, W, 3] one, given alpha 255). `effects`: ids or names. Returns a new [H, W, 4] array."""
    img = np.ascontiguousarray(rgba, dtype=np.uint8)
    if img.shape[-1] == 3:
        img = np.concatenate([img, np.full(img.shape[:2] + (1,), 255, np.uint8)], -1)
    ids = [EFFECTS.index(e) if isinstance(e, str) else int(e) for e in effects]
    h, w, _ = img.shape
    out = np.empty_like(img)
    arr = (C.c_int * max(1, len(ids)))(*ids)
    check(lib().fr_post_process(device, arr, len(ids), float(time), w, h,
                                img.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


# ---- tracer.rs operator API ---------------------------------------------------

_DENOISE_MODES = (False, True, "guided", "temporal", "temporal-guided")


class TraceModel:
    """tracer.rs:12-17 {scene, width, height, pixels}, plus the render context the frames
    run on: one fr_ctx per model, created on the first frame and reused by every later
    update() / save_image() (no per-frame stream, event or buffer allocation)."""

    def __init__(self, scene, width, height):
        self.scene, self.width, self.height = scene, width, height
        self.pixels = np.zeros(width * height * 3, dtype=np.uint8)
        self.frame = 0
        self.seed = DEFAULT_SEED
        self.device = 0
        self.ctx = None
        self.last_stats = None
        self._pinned = None  # page-locked home of `pixels` once update() runs on the device

    def context(self):
        if self.ctx is None:
            self.ctx = RenderContext(self.device)
        return self.ctx

    def render(self, scene, spp, max_depth, seed, mt_bands=False, scene_jit=False):
        """One frame on the model's context: (mean[H,W,3], u8[H,W,3], stats). scene_jit: the
        trace kernel compiled for the scene once ready (same bits; compiled in the background,
        so a render never waits for it)."""
        ctx = self.context()
        ctx.render(scene, self.scene.camera, make_params(self.width, self.height, spp, max_depth, seed,
                                                         mt_bands=mt_bands, scene_jit=scene_jit))
        self.last_stats = ctx.sync()
        mean, u8 = ctx.download(self.width, self.height)
        return mean, u8, self.last_stats

    def frame_u8(self, scene, max_depth, seed, accumulate=False, denoise=False):
        """update()'s frame: 1 spp, only the u8 image copied back, by DMA into page-locked
        memory that `pixels` views (overwritten by the next frame, as tracer.rs's
        model.pixels is). The view keeps the page-locked block alive, so an array returned
        here stays valid memory after the model is closed or collected; copy it to keep a
        frame past the next update(). accumulate: the frame joins the context's accumulation
        (FR_FLAG_ACCUMULATE) and the image is the mean of every frame in it; "error": the
        accumulation also carries the error estimate (model.ctx.accum_error). denoise (with
        accumulate "error" or "adaptive"): from the second frame of an accumulation on the image
        is the accumulation's denoised u8 (RenderContext.denoise at the defaults); on its first
        frame, which has no variance yet, the plain u8. denoise="guided": the feature-guided
        filter at its defaults; the view's G-buffer is enqueued when an accumulation starts.
        denoise="temporal" / "temporal-guided": RenderContext.temporal at its defaults (with the
        guided levels), from the first frame on: a moved camera's first frame shows the previous
        view's accumulation reprojected under it."""
        if denoise not in _DENOISE_MODES:
            raise ValueError(f'denoise={denoise!r}: False, True or "guided", "temporal", "temporal-guided"')
        if denoise and accumulate not in ("error", "adaptive"):
            raise ValueError(f'denoise={denoise!r} needs accumulate="error" or "adaptive": the filter is steered by '
                             "the accumulation's variance")
        ctx = self.context()
        ctx.render(scene, self.scene.camera, make_params(self.width, self.height, 1, max_depth, seed,
                                                         accumulate=accumulate))
        self.last_stats = ctx.sync()
        if self._pinned is None:
            self._pinned = PinnedFrame(self.width, self.height)
        guided = denoise in ("guided", "temporal-guided")
        temporal = denoise in ("temporal", "temporal-guided")
        if (guided or temporal) and ctx.accum_info()[0] == 1:  # a new accumulation: a new view
            ctx.gbuffer(scene, self.scene.camera, self.width, self.height)
        if temporal:
            ctx.temporal(guide=guided or None)
            ctx.download_denoised_into(self._pinned.u8)
        elif denoise and ctx.accum_info()[0] >= 2:
            ctx.denoise(guided=guided)
            ctx.download_denoised_into(self._pinned.u8)
        else:
            ctx.download_into(u8=self._pinned.u8)
        self.pixels = self._pinned.u8.reshape(-1)
        return self.pixels

    def close(self):
        if self._pinned is not None:
            # model.pixels (and any array update() returned) keeps the page-locked block
            # alive by itself; only the model's own frame object goes
            self._pinned.close()
            self._pinned = None
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None


def create_model(width, height, scene=None):
    """tracer.rs:19-28: Scene::new = get_simple_scene + Camera::new(w, h)."""
    if scene is None:
        scene = Scene.builtin(0, width, height)
    elif scene.camera is None:
        scene.camera = camera_new(width, height)
    return TraceModel(scene, width, height)


def update(model, keys, delta_time, max_depth=MAX_DEPTH, accumulate=False, denoise=False):
    """tracer.rs:30-55: key bitmask 00EQADWS -> camera.orbit(delta), then one 1-spp frame
    into model.pixels. Each frame draws from its own RNG key. accumulate: while no key is
    pressed the frames add up on the model's context and model.pixels converges (the mean of
    every frame since the camera last moved); a key press moves the camera, which starts anew.
    accumulate="error": the same picture, and model.ctx.accum_error(threshold) tells how far the
    accumulation has converged (FR_FLAG_ACCUM_ERROR). denoise=True (with accumulate="error" or
    "adaptive", ValueError otherwise): model.pixels is the accumulation filtered by its own
    per-pixel variance (RenderContext.denoise) from its second frame on, the plain picture on
    its first frame and right after a key press restarts it. denoise="guided": the same with the
    feature-guided filter (RenderContext.denoise(guided=True)), whose G-buffer is enqueued on the
    first frame of each accumulation. denoise="temporal": temporal reuse (RenderContext.temporal)
    from the first frame of every accumulation on, so the frames shown while a key is held carry
    the previous view's samples; "temporal-guided": the same through the guided levels."""
    if denoise not in _DENOISE_MODES:
        raise ValueError(f'denoise={denoise!r}: False, True or "guided", "temporal", "temporal-guided"')
    if denoise and accumulate not in ("error", "adaptive"):
        raise ValueError(f'denoise={denoise!r} needs accumulate="error" or "adaptive"')
    d = (C.c_float * 3)()
    check(lib().fr_update_delta(int(keys) & 0xFF, float(delta_time), d))
    camera_orbit(model.scene.camera, list(d))
    seed = model.seed ^ (0x9E3779B97F4A7C15 * (model.frame + 1) & 0xFFFFFFFFFFFFFFFF)
    model.frame += 1
    return model.frame_u8(model.scene, max_depth, seed, accumulate=accumulate, denoise=denoise)


def write_png(path, rgb8):
    """Minimal RGB8 PNG writer (the reference uses the image crate, tracer.rs:186)."""
    h, w, _ = rgb8.shape
    raw = b"".join(b"\x00" + rgb8[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))


def save_image_mt(model, sample, path="out/basic_mt.png", max_depth=MAX_DEPTH):
    """tracer.rs:136-158: `sample` passes of render_mt (4 row bands over the plain simple
    scene, scenes::get_simple_scene, with the model's camera), each pass gamma-corrected
    to u8, the u8 frames averaged and truncated, PNG."""
    simple = Scene.builtin(0, model.width, model.height)
    # a one-shot call: the scene kernel if it is cached, never a compile (which a process that
    # exits after this call would wait for at exit)
    acc, u8, stats = model.render(simple, sample, max_depth, model.seed, mt_bands=True, scene_jit="cached")
    write_png(path, u8)
    return acc, u8, stats


def save_image(model, sample, path="out/basic.png", max_depth=MAX_DEPTH):
    """tracer.rs:160-187: `sample` spp per pixel, gamma 2, u8, PNG. Like the reference it
    fails if the output directory is missing (tracer.rs:186 unwrap)."""
    mean, u8, stats = model.render(model.scene, sample, max_depth, model.seed, scene_jit="cached")
    write_png(path, u8)
    return mean, u8, stats
