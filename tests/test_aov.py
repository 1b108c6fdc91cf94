"""First-hit AOV buffers (rt_render_aov) without a GPU: the ABI surface, the status codes the entry points return before they
need a device, and the CPU checker (tests/aov_checker.py) pinned to the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_checker as K
import scenes

abi = scenes.abi
ROOT = scenes.ROOT


def _buffers(n, **which):
    """rt_aov_buffers over host arrays for the channels named in `which` (name -> True)"""
    b, keep = abi.AovBuffers(), []
    for name in which:
        a = np.zeros(n * (3 if name in ("albedo", "normal") else 1), dtype=np.uint32 if name in ("primitive", "material") else np.float32)
        keep.append(a)
        setattr(b, name, a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_float)))
    return b, keep


def test_aov_symbols_and_struct(hb):
    lib = hb.lib()
    for sym in ("rt_render_aov", "rt_render_aov_device"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(abi.AovBuffers) == abi.EXPECTED_SIZES["rt_aov_buffers"][1] == 48
    assert tuple(n for n, _ in abi.AovBuffers._fields_) == abi.AOV_CHANNELS


def test_aov_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    cam = hb.camera_new(**ls.camera_params)
    lib = hb.lib()
    w, h = 16, 9

    def call(opts, bufs, device=False):
        f = lib.rt_render_aov_device if device else lib.rt_render_aov
        args = (s._h, C.byref(cam), C.byref(opts), C.byref(bufs)) + ((C.c_void_p(0),) if device else ())
        return f(*args)

    for device in (False, True):
        full, _keep = _buffers(w * h, **{c: True for c in abi.AOV_CHANNELS})
        assert call(abi.default_render_opts(w, h, 2), full, device) == abi.RT_ERR_NO_DEVICE
        assert call(abi.default_render_opts(w, h, 2), abi.AovBuffers(), device) == abi.RT_ERR_INVALID_ARGUMENT  # all NULL
        o = abi.default_render_opts(w, h, 2)
        o.output_layout = abi.RT_LAYOUT_SHARD
        assert call(o, full, device) == abi.RT_ERR_UNSUPPORTED
        o = abi.default_render_opts(w, h, 2)
        o.shard_count = 2
        assert call(o, full, device) == abi.RT_ERR_UNSUPPORTED
        assert call(abi.default_render_opts(1, h, 2), full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, h, 0), full, device) == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(hb.RtHipError) as e:
        s.render_aov(cam, abi.default_render_opts(w, h, 2))
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        s.render_aov(cam, abi.default_render_opts(w, h, 2), channels=("albedo", "colour"))


@pytest.mark.parametrize("sample_begin", [0, 7])
def test_checker_reproduces_the_oracle_render_jitter(O, sample_begin):
    """one pass of an all-Emit(1.0) scene: the oracle's image IS the texture colour of each primary ray, so the checker's
    albedo -- its own rays, hits and texture restatement -- must equal it bit for bit"""
    sc = K.emit_scene()
    cpu = O.Scene(sc)
    cam = O.camera_new(**K.EMIT_CAMERA)
    w, h = 40, 24
    opts = abi.default_render_opts(w, h, 1, method=abi.RT_METHOD_NAIVE, seed=5)
    opts.sample_begin = sample_begin
    opts.sample_split = 1
    img, _ = cpu.render(cam, opts)
    ref = K.aovs(sc, cpu, cam, w, h, 1, seed=5, sample_begin=sample_begin)
    assert np.array_equal(ref["albedo"].reshape(h, w, 3), img)
    # and the picture is not trivial: sky, Solid and Lerp primitives all appear
    assert len(np.unique(ref["material"])) >= 4


def test_direction_textures_match_the_emit_twin(O):
    """the checker's Lerp / Image restatement (and Solid, and the sky) against the oracle's own texture evaluation, through the
    Emit twin of scenes that hold every direction-only texture"""
    cases = [(scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA)] + [scenes.random_everything(seed) for seed in (1, 4, 9)]
    checked = 0
    for sc, cam_params in cases:
        cpu, twin = O.Scene(sc), O.Scene(K.emit_twin(sc))
        cam = O.camera_new(**cam_params)
        w, h = 32, 18
        pixels = np.arange(0, w * h, 3)
        o, d = K.primary_rays(cam, w, h, 2, pixels, 0)
        hits = cpu.check_hit(o, d)
        direction_only = np.array([sc.textures[int(sc.materials[int(m)].texture)].type in (abi.RT_TEX_LERP, abi.RT_TEX_IMAGE,
                                                                                             abi.RT_TEX_SOLID)
                                   for m in hits["material"]])
        sel = np.nonzero(direction_only)[0]
        wo = K.normalised(d[sel])
        mine = np.zeros((len(sel), 3), np.float32)
        for i, r in enumerate(sel):
            mat = sc.materials[int(hits["material"][r])]
            mine[i] = K.texture_colours(sc, int(mat.texture), wo[i:i + 1], hits["point"][r:r + 1])[0]
        ref = K.emit_twin_colours(twin, o[sel], d[sel])
        assert np.array_equal(mine, ref)
        checked += len(sel)
    assert checked > 500


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() { rt_hip::RenderOptions o; o.width = 64; o.height = 36; o.samples_per_pixel = 16;\n'
           'rt_hip::AovBuffers (*f)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, uint64_t, uint64_t)'
           ' = &rt_hip::render_aov; (void)f; (void)o; return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
