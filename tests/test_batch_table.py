"""The claim step's per-wave batch table (trace_kernel.h) at the edges of a
batch: when a wave seeds 64 items, each lane stores its item's whole start state as one
LDS entry, and a claiming lane only fetches it. Every case renders a frame the oracle
renders whole and must match it bit for bit: means, u8 and path counters.

The list kernels with 8-B records (scene_08's) have the table; the other families share
the claim code and keep the batch in registers, so each of them runs here too.
"""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests.test_gpu_parity import ROOT, assert_parity

pytestmark = pytest.mark.gpu


def _oracle(gpu, scene, w, h, spp, depth, text=None, **kw):
    text = text if text is not None else open(gpu.scene_path(scene)).read()
    prims, (frm, at, vup, fov) = S.load_json(text)
    cam = O.camera_look(frm, at, vup, fov, 0.1, w, h)
    return O.render(prims, cam, w, h, spp, depth, threads=8, **kw)[:3]


def _assert_bits(mean, u8, st, omean, ou8, ocnt, rows=None):
    assert_parity(mean, u8, st, omean, ou8, ocnt, rows=rows)
    if rows is not None:
        mean, omean = mean[rows], omean[rows]
    assert np.array_equal(mean.view(np.uint32), omean.view(np.uint32))


def _render_vs_oracle(gpu, scene, w, h, spp, depth=8, **kw):
    sc = gpu.Scene.from_file(gpu.scene_path(scene), w, h)
    mean, u8, st = gpu.render(sc, sc.camera, w, h, spp, depth, **kw)
    _assert_bits(mean, u8, st, *_oracle(gpu, scene, w, h, spp, depth))
    return st


@pytest.mark.parametrize("w,h", [(20, 12), (9, 17), (67, 9)])
def test_invalid_slots_inside_a_batch(gpu, w, h, monkeypatch):
    """Image sizes that are no multiple of the 8x8 tile: every edge tile's batch holds entries
    past the image, which a claim must leave without an item. One workgroup claims them all."""
    monkeypatch.setenv("FR_MAX_WGS", "1")
    _render_vs_oracle(gpu, "scene_08", w, h, 21)


@pytest.mark.parametrize("w,h,spp", [(4, 4, 1), (8, 8, 16), (16, 8, 32)])
def test_fewer_items_than_a_batch_and_exact_multiples(gpu, w, h, spp):
    """16 items of one sample in one batch; exactly one full batch; two tiles x (one block +
    four sub-blocks): the queue ends on a batch boundary."""
    _render_vs_oracle(gpu, "scene_08", w, h, spp)


@pytest.mark.parametrize("shard", [1, 2])
def test_sub_block_items_across_shards(gpu, shard):
    """spp 37: the third block runs as sub-blocks of 4, 1 samples, whose entries' buffer slot
    is the block's (item - k P) with the shard's own P."""
    w, h, spp, depth = 40, 24, 37, 8
    sc = gpu.Scene.from_file(gpu.scene_path("scene_08"), w, h)
    mean, u8, st = gpu.render(sc, sc.camera, w, h, spp, depth, shard_index=shard, shard_count=3)
    rows = [y for y in range(h) if (y // 8) % 3 == shard]
    assert np.isnan(mean[[y for y in range(h) if y not in rows]]).all()
    omean, ou8, ocnt = _oracle(gpu, "scene_08", w, h, spp, depth, shard_index=shard, shard_count=3)
    _assert_bits(mean, u8, st, omean, ou8, ocnt, rows=rows)


@pytest.mark.parametrize("jit", [False, "wait"])
def test_grab_between_the_claims_of_one_step(gpu, jit, monkeypatch):
    """One workgroup, 160 batches over three blocks: the waves' free lanes outnumber the
    batch's remaining items again and again, on the compiled-in kernel and on the
    scene-specialised one."""
    monkeypatch.setenv("FR_MAX_WGS", "1")
    _render_vs_oracle(gpu, "scene_08", 64, 40, 40, scene_jit=jit)


def test_family_12_byte_records_with_a_plane(gpu, monkeypatch):
    monkeypatch.setenv("FR_MAX_WGS", "1")
    _render_vs_oracle(gpu, "scene_01", 40, 24, 20)


def test_family_bvh_with_class_records(gpu, monkeypatch):
    """A 200-sphere generator scene: the BVH kernel with attenuation-class records."""
    spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(ROOT, "tools", "gen_scene.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    text = gs.dumps(gs.generator_scene(200, "sphere"))
    monkeypatch.setenv("FR_MAX_WGS", "1")
    monkeypatch.setenv("FR_BVH", "1")  # the BVH whatever the scene's cost estimate
    w, h, spp, depth = 40, 24, 8, 8
    sc = gpu.Scene.from_json(text, w, h)
    mean, u8, st = gpu.render(sc, sc.camera, w, h, spp, depth)
    _assert_bits(mean, u8, st, *_oracle(gpu, None, w, h, spp, depth, text=text))
    assert st["hits"] > 0


def test_family_mt_bands_with_rows_left_over(gpu, monkeypatch):
    """save_image_mt at 40x26: bands of 6 rows, rows 24 and 25 belong to no band (their
    slots stay without an item)."""
    monkeypatch.setenv("FR_MAX_WGS", "1")
    w, h, sample = 40, 26, 3
    sc = gpu.Scene.builtin(0, w, h)
    acc, u8, st = gpu.render(sc, sc.camera, w, h, sample, 50, seed=0x5EED, mt_bands=True)
    oacc, ou8, ocnt = O.render_mt(S.BUILTIN[0](), O.camera_new(w, h), w, h, sample, 50, 0x5EED)
    assert np.array_equal(acc.view(np.uint32), oacc.view(np.uint32))
    assert np.array_equal(u8, ou8)
    assert (st["segments"], st["hits"]) == (ocnt["segments"], ocnt["hits"])
    assert not u8[4 * (h // 4):].any()


def test_two_passes(gpu, monkeypatch):
    """Three blocks in two launches: the second launch's entries start at block b0 = 2 and
    its items are the last block's sub-blocks only."""
    monkeypatch.setenv("FR_PIPELINE", "2")
    st = _render_vs_oracle(gpu, "scene_08", 40, 24, 48)
    assert st["trace_launches"] == 2
