"""Anti-aliased ID mattes (rt_render_matte, rt_matte_extract) without a GPU: the CPU checker (tests/matte_checker.py) on pass-ID
arrays written by hand and over the first-hit checker, then the C-ABI boundary on a host-only scene: structs, defaults and the
status code of every check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_checker as K
import matte_checker as M
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32
SKY = 0xFFFFFFFF


def _one_pixel(passes, layers):
    ids, cov, res = M.layers_from_pass_ids(np.array(passes, dtype=np.uint32)[:, None], layers)
    return ids[:, 0].tolist(), cov[:, 0], res[0]


# ---- the checker on pass IDs written by hand ----
def test_ranking_by_count_then_id_with_the_sky_last():
    ids, cov, res = _one_pixel([7, SKY, 3, 7, SKY, 3, 9, 7], 8)
    assert ids == [7, 3, SKY, 9] + [SKY] * 4  # 3 and the sky tie on two passes: the smaller ID first, the sky last among equals
    assert cov.tobytes() == (np.array([3, 2, 2, 1, 0, 0, 0, 0], F32) / F32(8)).tobytes()
    assert not np.signbit(cov).any() and res == 0.0
    # an empty layer and a sky layer differ in coverage only
    assert ids[2] == ids[4] == SKY and cov[2] > 0 and cov[4] == 0


def test_a_ninth_id_is_overflow_and_goes_to_the_residual():
    ids, cov, res = _one_pixel(list(range(10, 19)) + [10], 8)  # nine distinct IDs, then the first again
    assert ids == list(range(10, 18))
    assert cov.tobytes() == (np.array([2, 1, 1, 1, 1, 1, 1, 1], F32) / F32(10)).tobytes()
    assert res == F32(1) / F32(10)


def test_an_id_that_arrives_after_the_table_is_full_is_never_counted():
    late = 99
    ids, cov, res = _one_pixel(list(range(8)) + [late] * 6 + [0, 0], 8)  # `late` would rank first by count
    assert late not in ids and ids == list(range(8))
    assert cov[0] == F32(3) / F32(16) and (cov[1:] == F32(1) / F32(16)).all()
    assert res == F32(6) / F32(16)


def test_fewer_layers_than_occupied_slots_leave_the_rest_to_the_residual():
    passes = [5] * 4 + [6] * 3 + [7] * 2 + [8]
    for k in range(1, 9):
        ids, cov, res = _one_pixel(passes, k)
        assert ids == [5, 6, 7, 8, SKY, SKY, SKY, SKY][:k]
        counts = [4, 3, 2, 1, 0, 0, 0, 0][:k]
        assert cov.tobytes() == (np.array(counts, F32) / F32(10)).tobytes()
        assert res == F32(10 - sum(counts)) / F32(10)


def test_counts_and_residual_add_up_to_the_passes():
    rng = np.random.default_rng(1)
    spp, n = 16, 200
    passes = rng.integers(0, 12, (spp, n)).astype(np.uint32)
    passes[rng.random((spp, n)) < 0.2] = SKY
    for k in (1, 3, 8):
        ids, cov, res = M.layers_from_pass_ids(passes, k)
        assert ids.shape == cov.shape == (k, n) and res.shape == (n,)
        counts = cov * F32(spp)  # a power-of-two spp: exact
        assert (counts == np.round(counts)).all()
        assert ((counts.sum(axis=0) + res * F32(spp)) == spp).all()
        assert ((cov.sum(axis=0, dtype=F32) + res) == F32(1.0)).all()
    assert (M.layers_from_pass_ids(passes, 8)[2] > 0).any()  # twelve IDs and the sky: some pixel overflows


def test_extract_on_hand_written_layers():
    ids = np.array([[4, SKY, 2], [SKY, SKY, SKY], [SKY, SKY, SKY]], dtype=np.uint32)
    cov = np.array([[0.75, 1.0, 0.5], [0.25, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=F32)
    assert M.extract(ids, cov, []).tolist() == [0.0, 0.0, 0.0]
    assert M.extract(ids, cov, [4]).tolist() == [0.75, 0.0, 0.0]
    assert M.extract(ids, cov, [SKY]).tolist() == [0.25, 1.0, 0.0]  # empty layers do not match the sky's ID
    assert M.extract(ids, cov, [2, 4, SKY, 4, 2]).tolist() == [1.0, 1.0, 0.5]
    assert M.extract(ids, np.full_like(cov, 0.75), [4, SKY, 2]).tolist() == [1.0, 1.0, 1.0]  # clamped


# ---- the checker over the oracle ----
@pytest.mark.parametrize("name", ["emit_scene", "all_materials"])
def test_layers_over_the_first_hit_checker(O, name):
    sc, cam_params = (K.emit_scene(), K.EMIT_CAMERA) if name == "emit_scene" else (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA)
    cpu, cam = O.Scene(sc), O.camera_new(**cam_params)
    w, h, spp = 16, 9, 8
    for kind in ("primitive", "material"):
        passes = M.pass_ids(sc, cpu, cam, w, h, spp, 5, 2, kind)
        assert passes.shape == (spp, w * h) and passes.dtype == np.uint32
        # one pass: layer 0 is the oracle's ID channel, fully covered
        first = K.aovs(sc, cpu, cam, w, h, 1, seed=5, sample_begin=2)[kind]
        ids1, cov1, res1 = M.layers_from_pass_ids(passes[:1], 8)
        assert ids1[0].tobytes() == first.tobytes() and (cov1[0] == 1.0).all() and (res1 == 0.0).all()
        assert (ids1[1:] == SKY).all() and (cov1[1:] == 0.0).all()
        # K layers are the first K of eight
        ids8, cov8, res8 = M.layers_from_pass_ids(passes, 8)
        for k in range(1, 8):
            ids, cov, res = M.layers_from_pass_ids(passes, k)
            assert ids.tobytes() == ids8[:k].tobytes() and cov.tobytes() == cov8[:k].tobytes()
            assert ((cov.sum(axis=0, dtype=F32) + res) == F32(1.0)).all()
        assert (cov8[1] > 0).any()  # some pixel sees two IDs: silhouettes exist at this size


# ---- the C ABI on a host-only scene ----
def _buffers(n, layers, residual=True):
    b = abi.MatteBuffers()
    keep = [np.zeros(layers * n, np.uint32), np.zeros(layers * n, F32), np.zeros(n, F32)]
    b.ids = keep[0].ctypes.data_as(C.POINTER(C.c_uint32))
    b.coverage = keep[1].ctypes.data_as(C.POINTER(C.c_float))
    if residual:
        b.residual = keep[2].ctypes.data_as(C.POINTER(C.c_float))
    return b, keep


def test_symbols_structs_and_defaults(hb):
    lib = hb.lib()
    for sym in ("rt_matte_opts_default", "rt_render_matte", "rt_render_matte_device", "rt_matte_extract", "rt_matte_extract_device"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.rt_abi_version() == abi.RT_ABI_VERSION == 2
    assert C.sizeof(abi.MatteOpts) == abi.EXPECTED_SIZES["rt_matte_opts"][1] == 32
    assert C.sizeof(abi.MatteBuffers) == abi.EXPECTED_SIZES["rt_matte_buffers"][1] == 24
    assert tuple(n for n, _ in abi.MatteBuffers._fields_) == abi.MATTE_BUFFERS
    assert abi.RT_MATTE_SLOTS == M.SLOTS == 8 and (abi.RT_MATTE_ID_PRIMITIVE, abi.RT_MATTE_ID_MATERIAL) == (0, 1)
    o = abi.MatteOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    assert lib.rt_matte_opts_default(C.byref(o)) == abi.RT_OK
    assert o.id_kind == abi.RT_MATTE_ID_MATERIAL and o.layers == 4 and list(o.reserved) == [0] * 6
    assert bytes(abi.default_matte_opts()) == bytes(o) == bytes(hb.matte_opts())
    assert lib.rt_matte_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT
    m = hb.matte_opts(id_kind="primitive", layers=7)
    assert (m.id_kind, m.layers) == (abi.RT_MATTE_ID_PRIMITIVE, 7)
    with pytest.raises(ValueError):
        hb.matte_opts(id_kind="mesh")
    with pytest.raises(ValueError):
        hb.matte_opts(slots=8)


def test_render_matte_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    cam = hb.camera_new(**ls.camera_params)
    lib = hb.lib()
    w, h = 16, 9
    n = w * h

    def call(opts, mopts, bufs, device=False, scene=s._h, camera=cam):
        f = lib.rt_render_matte_device if device else lib.rt_render_matte
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = (scene, ref(camera), ref(opts), ref(mopts), ref(bufs)) + ((C.c_void_p(0),) if device else ())
        return f(*args)

    ok, matte = abi.default_render_opts(w, h, 2), abi.default_matte_opts()
    for device in (False, True):
        full, _keep = _buffers(n, 8)
        for good in (matte, abi.default_matte_opts(abi.RT_MATTE_ID_PRIMITIVE, 1), abi.default_matte_opts(layers=8)):
            assert call(ok, good, full, device) == abi.RT_ERR_NO_DEVICE
        no_residual, _keep2 = _buffers(n, 8, residual=False)
        assert call(ok, matte, no_residual, device) == abi.RT_ERR_NO_DEVICE  # the residual is optional
        for args in ((None, matte, full), (ok, None, full), (ok, matte, None)):
            assert call(*args, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, matte, full, device, scene=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, matte, full, device, camera=None) == abi.RT_ERR_INVALID_ARGUMENT
        for missing in ("ids", "coverage"):
            b, _k = _buffers(n, 8)
            setattr(b, missing, None)
            assert call(ok, matte, b, device) == abi.RT_ERR_INVALID_ARGUMENT, missing
        for bad in (dict(layers=0), dict(layers=9), dict(id_kind=2), dict(id_kind=-1)):
            assert call(ok, abi.default_matte_opts(**bad), full, device) == abi.RT_ERR_INVALID_ARGUMENT, bad
        for word in range(6):
            m = abi.default_matte_opts()
            m.reserved[word] = 1
            assert call(ok, m, full, device) == abi.RT_ERR_INVALID_ARGUMENT, word
        # overlapping outputs: coverage inside ids, the residual on the last layer of the coverage
        b, keep = _buffers(n, 8)
        b.coverage = C.cast(C.c_void_p(keep[0].ctypes.data + 4 * (4 * n - 1)), C.POINTER(C.c_float))
        assert call(ok, abi.default_matte_opts(layers=4), b, device) == abi.RT_ERR_INVALID_ARGUMENT
        b, keep = _buffers(n, 8)
        b.residual = C.cast(C.c_void_p(keep[1].ctypes.data + 4 * 3 * n), C.POINTER(C.c_float))
        assert call(ok, abi.default_matte_opts(layers=4), b, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, abi.default_matte_opts(layers=3), b, device) == abi.RT_ERR_NO_DEVICE  # ... which three layers do not reach
        # the rules of rt_render_aov
        o = abi.default_render_opts(w, h, 2)
        o.output_layout = abi.RT_LAYOUT_SHARD
        assert call(o, matte, full, device) == abi.RT_ERR_UNSUPPORTED
        o = abi.default_render_opts(w, h, 2)
        o.shard_count = 2
        assert call(o, matte, full, device) == abi.RT_ERR_UNSUPPORTED
        assert call(abi.default_render_opts(1, h, 2), matte, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, 1, 2), matte, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, h, 0), matte, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(1 << 16, 1 << 15, 2), matte, full, device) == abi.RT_ERR_UNSUPPORTED  # 2^31 pixels
    with pytest.raises(hb.RtHipError) as e:
        s.render_matte(cam, ok, residual=True)
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(hb.RtHipError) as e:
        s.render_matte(cam, ok, layers=9)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        s.render_matte(cam, ok, id_kind="object")
    with pytest.raises(ValueError):
        s.render_matte_device(cam, ok, {"ids": 16, "coverage": 32, "overflow": 48})


def test_matte_extract_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    lib = hb.lib()
    w, h, k = 16, 9, 4
    n = w * h
    sel = np.array([3, 1, 3], dtype=np.uint32)
    big = np.zeros(abi.MATTE_MAX_IDS + 1, dtype=np.uint32)
    out = np.zeros(n, F32)

    def call(bufs, device=False, scene=s._h, width=w, height=h, layers=k, ids=sel.ctypes.data, n_ids=3, dst=out.ctypes.data):
        f = lib.rt_matte_extract_device if device else lib.rt_matte_extract
        args = (scene, None if bufs is None else C.byref(bufs), C.c_uint32(width), C.c_uint32(height), C.c_uint32(layers),
                C.cast(C.c_void_p(ids), C.POINTER(C.c_uint32)), C.c_uint64(n_ids), C.cast(C.c_void_p(dst), C.POINTER(C.c_float)))
        return f(*(args + ((C.c_void_p(0),) if device else ())))

    for device in (False, True):
        full, keep = _buffers(n, k, residual=False)  # the residual is not read
        assert call(full, device) == abi.RT_ERR_NO_DEVICE
        assert call(full, device, ids=None, n_ids=0) == abi.RT_ERR_NO_DEVICE  # an empty selection
        assert call(full, device, ids=big.ctypes.data, n_ids=abi.MATTE_MAX_IDS) == abi.RT_ERR_NO_DEVICE
        assert call(full, device, ids=big.ctypes.data, n_ids=abi.MATTE_MAX_IDS + 1) == abi.RT_ERR_UNSUPPORTED
        assert call(full, device, width=1, height=1, layers=1) == abi.RT_ERR_NO_DEVICE
        assert call(full, device, scene=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(None, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(full, device, dst=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(full, device, ids=None) == abi.RT_ERR_INVALID_ARGUMENT  # three IDs at NULL
        for missing in ("ids", "coverage"):
            b, _k = _buffers(n, k)
            setattr(b, missing, None)
            assert call(b, device) == abi.RT_ERR_INVALID_ARGUMENT, missing
        for bad in (dict(width=0), dict(height=0), dict(layers=0), dict(layers=9)):
            assert call(full, device, **bad) == abi.RT_ERR_INVALID_ARGUMENT, bad
        assert call(full, device, width=1 << 16, height=(1 << 15) + 1) == abi.RT_ERR_UNSUPPORTED  # more than 2^31 pixels
        # out must not overlap the layers or the selection
        assert call(full, device, dst=keep[0].ctypes.data + 4 * (k * n - 1)) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(full, device, dst=keep[1].ctypes.data) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(full, device, dst=sel.ctypes.data - 4 * (n - 1)) == abi.RT_ERR_INVALID_ARGUMENT
    ids, cov = np.zeros((k, h, w), np.uint32), np.zeros((k, h, w), F32)
    with pytest.raises(hb.RtHipError) as e:
        s.matte_extract(ids, cov, [1, 2])
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(hb.RtHipError) as e:
        s.matte_extract({"ids": ids, "coverage": cov}, None, np.zeros(abi.MATTE_MAX_IDS + 1, np.uint32))
    assert e.value.code == abi.RT_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        s.matte_extract(ids, cov[:2], [1])


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() { rt_hip::MatteOptions m; m.id_kind = RT_MATTE_ID_PRIMITIVE; m.layers = RT_MATTE_SLOTS;\n'
           'rt_hip::MatteLayers (*f)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, '
           'const rt_hip::MatteOptions &, uint64_t, uint64_t) = &rt_hip::render_matte; (void)f; (void)m;\n'
           'std::vector<float> (*g)(const rt_hip::Bvh &, const rt_hip::MatteLayers &, const std::vector<uint32_t> &) = '
           '&rt_hip::matte_extract; (void)g;\n'
           'rt_hip::MatteLayers l; return (int)(l.ids.size() + l.coverage.size() + l.residual.size()); }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
