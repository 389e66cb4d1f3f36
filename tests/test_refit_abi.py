"""The moving-scene calls in the header, the Python mirror and the integration notes."""
import ctypes as C
import os

import numpy as np

from tests.test_plan import ROOT

FR_EARG = -1


def test_header_and_python_mirror(fr):
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    for decl in (
            "int fr_scene_update(fr_scene* scene, const uint32_t* index /* NULL: 0..n-1 */, const fr_prim* prims, uint32_t n, uint32_t flags);",
            "int fr_scene_rebuild(fr_scene* scene);",
            "int fr_ctx_scene_info(fr_ctx* ctx, fr_scene* scene, fr_scene_info* out);",
            "int fr_scene_download_table(fr_scene* scene, int device, uint32_t which, void* out, size_t cap, size_t* bytes);",
            "#define FR_UPDATE_REBUILD 1u", "#define FR_SCENE_SYNC_NONE 0u", "#define FR_SCENE_SYNC_PACK 1u",
            "#define FR_SCENE_SYNC_REFIT 2u", "#define FR_TABLE_RECORDS 0u", "#define FR_TABLE_LEAF_RECORDS 1u",
            "#define FR_TABLE_LEAF_ORDER 2u", "#define FR_TABLE_NODES 3u", "} fr_scene_info;", "#define FR_ABI_VERSION 6"):
        assert decl in hdr, decl
    # the names are in the header's list of additive entries
    additive = hdr[hdr.index("#define FR_ABI_VERSION 6"):hdr.index("/* error codes */")]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fr_scene_update", "fr_scene_rebuild", "fr_ctx_scene_info", "fr_scene_download_table"):
        assert name in additive and name in fr.EXPORTS and hasattr(fr.lib(), name) and name in integ, name
    assert "fr_scene_info" in additive and "FR_UPDATE_REBUILD" in additive and "FR_SCENE_SYNC_" in additive
    assert fr.lib().fr_abi_version() == 6
    # sizeof(fr_scene_info): 4 u32, 4 u64, 4 f32, 2 u32
    assert C.sizeof(fr.FrSceneInfo) == 72
    fields = hdr[hdr.index("typedef struct fr_scene_info {"):hdr.index("} fr_scene_info;")]
    at = -1
    for name, _ in fr.FrSceneInfo._fields_:  # the mirror's fields in the header's order
        pos = fields.index(name)
        assert pos > at, name
        at = pos
    assert (fr.FR_UPDATE_REBUILD, fr.FR_SCENE_SYNC_NONE, fr.FR_SCENE_SYNC_PACK, fr.FR_SCENE_SYNC_REFIT) == (1, 0, 1, 2)
    assert (fr.FR_TABLE_RECORDS, fr.FR_TABLE_LEAF_RECORDS, fr.FR_TABLE_LEAF_ORDER, fr.FR_TABLE_NODES) == (0, 1, 2, 3)
    for name in ("update", "set_spheres", "rebuild", "download_table"):
        assert callable(getattr(fr.Scene, name))
    assert callable(fr.RenderContext.scene_info)


def test_update_edits_the_host_list_without_a_device(fr):
    L = fr.lib()
    assert L.fr_scene_update(None, None, None, 0, 0) == FR_EARG and L.fr_scene_rebuild(None) == FR_EARG
    assert L.fr_ctx_scene_info(None, None, None) == FR_EARG
    assert L.fr_scene_download_table(None, 0, 0, None, 0, None) == FR_EARG
    objs = [fr.Sphere((float(i), 0.0, -4.0), 1.0, 0, (0.5, 0.5, 0.5), 0.0) for i in range(4)]
    sc = fr.Scene.from_objects(objs)
    before = [bytes(p) for p in sc.prims()]
    # duplicates: the last one wins
    sc.update([2, 2], [fr.Sphere((9.0, 9.0, 9.0), 1.0, 0, (0.5, 0.5, 0.5), 0.0),
                       fr.Sphere((7.0, 8.0, 9.0), 2.0, 0, (0.5, 0.5, 0.5), 0.0)])
    p = sc.prims()
    assert list(p[2].g[:4]) == [7.0, 8.0, 9.0, 2.0] and [bytes(q) for q in p[:2]] == before[:2] and bytes(p[3]) == before[3]
    # indices None: primitives 0..n-1
    sc.update(None, [fr.Sphere((1.5, 0.0, 0.0), 1.0, 0, (0.5, 0.5, 0.5), 0.0)])
    assert list(sc.prims()[0].g[:3]) == [1.5, 0.0, 0.0]
    # an index out of range, an unknown kind, unknown flags: FR_EARG and nothing moves
    have = [bytes(q) for q in sc.prims()]
    idx = (C.c_uint32 * 2)(1, 4)
    arr = (fr.FrPrim * 2)(objs[0].to_prim(), objs[1].to_prim())
    assert L.fr_scene_update(sc._h, idx, arr, 2, 0) == FR_EARG
    arr[0].kind = 77
    idx[1] = 0
    assert L.fr_scene_update(sc._h, idx, arr, 2, 0) == FR_EARG
    arr[0].kind = 0
    assert L.fr_scene_update(sc._h, idx, arr, 2, 6) == FR_EARG
    assert L.fr_scene_update(sc._h, None, arr, 5, 0) == FR_EARG  # more than the list holds
    assert [bytes(q) for q in sc.prims()] == have
    assert L.fr_scene_update(sc._h, None, None, 0, 0) == 0
    # set_spheres: numpy in, the radii kept unless given
    sc.set_spheres([3, 1], np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]], np.float32))
    p = sc.prims()
    assert list(p[3].g[:4]) == [0.0, 1.0, 2.0, 1.0] and list(p[1].g[:4]) == [3.0, 4.0, 5.0, 1.0]
    sc.set_spheres([0], np.array([[0.5, 0.5, 0.5]], np.float32), radii=[0.25])
    assert list(sc.prims()[0].g[:4]) == [0.5, 0.5, 0.5, 0.25]
    # no device copy yet: the table call says so
    size = C.c_size_t(0)
    assert L.fr_scene_download_table(sc._h, 0, 0, None, 0, C.byref(size)) == FR_EARG
    sc.rebuild()
    sc.close()
