"""rt_probe_sh and rt_probe_sh_eval on the GPU (csrc/rt_probe.hip), bit for bit: against the checker (tests/probe_checker.py: the
header's arithmetic in numpy f32, the oracle's fixed-ray integrator for every sample) and, with no oracle, against rt_radiance fed the
checker's directions.  test_probe.py shows on the CPU that the coefficients compared here differ where they should.  Where a sample's
value may be NaN (the MIS prologue returns ahead of the integrators' filter) any NaN equals any NaN; every other word compares as bits."""
import numpy as np
import pytest

import hard_tree_cases
import probe_cases as PB
import probe_checker as PC
import scenes
import sky_cases
import test_probe as TP
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture

pytestmark = pytest.mark.gpu
abi = scenes.abi
F32 = np.float32
NAIVE, MIS = abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS


def _gpu(hb, name):
    return hb.HipScene(PB.built(name)[0], device=0)


@pytest.mark.parametrize("name", sorted(PB.SCENES))
@pytest.mark.parametrize("method", PB.METHODS)
def test_coefficients_are_the_checkers(hb, name, method):
    """(K, S) = (4, 1), (4, 2), (7, 3), (13, 13) from sample_begin 5, five probes, both convolve values: coefficients and rays_shot"""
    gpu, pos = _gpu(hb, name), PB.positions(name)
    for k, split in PB.FOLDS:
        for convolve in (0, 1):
            ref, ref_rays = PB.reference(name, method, k, split, convolve)
            what = f"{name} method {method} K {k} S {split} convolve {convolve}"
            for _ in range(2):  # (twice: rays_shot is written, not added to)
                got, rays = gpu.probe_sh(pos, **PB.opts(method, k, split, convolve))
                assert_same_bits(got, ref, what, nan_equal=True)
                assert rays == ref_rays, what


@pytest.mark.parametrize("method", PB.METHODS)
def test_more_slots_than_a_workgroup(hb, method):
    """70 probes x S = 4: 280 slots on 256-lane workgroups, the last wave partly empty; under a cap of one workgroup (every lane
    refills) the same bytes"""
    ref, ref_rays = PB.many_reference(method)
    first = None
    for groups in (0, 1):
        gpu = _gpu(hb, "all_materials")
        gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, groups)
        got, rays = gpu.probe_sh(PB.many_positions(), **PB.opts(method, PB.MANY_K, PB.MANY_S))
        assert_same_bits(got, ref, f"70 probes, groups {groups}", nan_equal=True)
        assert rays == ref_rays
        first = first or got.tobytes()
        assert got.tobytes() == first


def _device_buffers(torch, hb, pos, o, off):
    n = len(pos)
    words = hb.probe_workspace_bytes(n, **o) // 4
    bufs = GuardedBuffers(torch, {"pos": ((n, 3), np.float32), "out": ((n, 9, 3), np.float32), "work": ((words,), np.float32),
                                  "rays": ((2,), np.uint32)}, off=off)
    lo = 4 + off
    bufs.buf["pos"][lo:lo + 3 * n] = torch.from_numpy(np.ascontiguousarray(pos, F32).view(np.int32).reshape(-1).copy()).to("cuda:0")
    return bufs


def _rays_value(bufs):
    r = bufs.read("rays")
    return int(r[0]) | (int(r[1]) << 32)


@pytest.mark.parametrize("method", PB.METHODS)
def test_device_entry_and_guards(hb, method):
    """device entry == host entry == checker; guard words around the outputs and the workspace at every alignment; a NULL rays_shot
    leaves the counter's words alone"""
    import torch
    name = "all_materials"
    gpu, pos = _gpu(hb, name), PB.positions(name)
    for k, split in ((4, 2), (7, 3)):
        o = PB.opts(method, k, split, 1)
        ref, ref_rays = PB.reference(name, method, k, split, 1)
        host, host_rays = gpu.probe_sh(pos, **o)
        for off in (3, 1, 2, 0):
            bufs = _device_buffers(torch, hb, pos, o, off)
            with_rays = off % 2 == 0  # (the counter is 8-byte aligned at even offsets)
            gpu.probe_sh_device(bufs.ptr("pos"), len(pos), bufs.ptr("out"), bufs.ptr("work"), bufs.ptr("rays") if with_rays else None, **o)
            torch.cuda.synchronize()
            got = bufs.read("out")
            assert_same_bits(got, ref, f"device K {k} S {split} off {off}", nan_equal=True)
            assert got.tobytes() == host.tobytes()
            bufs.read("work")  # (its guards)
            assert bufs.read("pos").tobytes() == pos.tobytes()
            if with_rays:
                assert _rays_value(bufs) == host_rays == ref_rays
            else:
                assert bufs.untouched("rays")


def _radiance_coefficients(gpu, pos, method, k, split, seed, begin, convolve=0):
    """the coefficients from rt_radiance: every pass's directions from the checker, streams = probe, one sample at sample_begin = the
    pass; projected in numpy"""
    n = len(pos)
    streams = np.arange(n, dtype=np.uint64)
    dirs = np.stack([PC.directions(seed, range(n), begin + j) for j in range(k)])
    values = np.stack([gpu.radiance(pos, dirs[j], streams=streams, method=method, samples=1, seed=seed, sample_begin=(begin + j) & PC.MASK64)
                       for j in range(k)])
    return PC.project(values, dirs, split, convolve), values


def _box_positions(gpu, n, seed):
    root = gpu.nodes()[0]
    lo, hi = np.array(root["min"], np.float64), np.array(root["max"], np.float64)
    return np.random.default_rng(seed).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (n, 3)).astype(F32)


@pytest.mark.parametrize("method", PB.METHODS)
def test_the_chain_tree_against_radiance_queries(hb, method):
    """the tree whose stacks need more than 64 KB of LDS (the lane's record lies behind them): GPU against GPU, 40 probes in and
    around the scene's box and one at the camera"""
    sc, cam_params, _, _ = hard_tree_cases.built("chain")
    gpu = hb.HipScene(sc, device=0)
    pos = np.concatenate([_box_positions(gpu, 40, 4), np.array([cam_params["origin"]], F32)])
    ref, values = _radiance_coefficients(gpu, pos, method, 8, 3, PB.SEED, PB.BEGIN)
    assert np.unique(values.reshape(-1, 3), axis=0).shape[0] > 20  # samples, not a constant
    got, _ = gpu.probe_sh(pos, **PB.opts(method, 8, 3))
    assert_same_bits(got, ref, f"chain method {method}", nan_equal=True)


@pytest.mark.parametrize("method", PB.METHODS)
def test_a_sky_over_the_lds_limit_against_radiance_queries(hb, method):
    """sky_cases `big_guided` (127 940 bytes of tables: they stay in global memory) over the floor: GPU against GPU"""
    sc, cam_params = sky_cases.RENDER_SCENES["floor"]()
    gpu = hb.HipScene(sky_cases.with_sky(sc, "big_guided"), device=0)
    pos = np.concatenate([np.array([cam_params["origin"], cam_params["lookat"]], F32) + F32(0.01), _box_positions(gpu, 30, 6)])
    ref, _ = _radiance_coefficients(gpu, pos, method, 8, 2, PB.SEED, PB.BEGIN, 1)
    got, _ = gpu.probe_sh(pos, **PB.opts(method, 8, 2, 1))
    assert_same_bits(got, ref, f"big sky method {method}", nan_equal=True)


@pytest.mark.parametrize("seed,begin", [((1 << 63) + 12345, (1 << 32) - 2), (0xFEDCBA9876543210, (1 << 64) - 2), (3, (1 << 63) + (1 << 32) - 2)])
def test_64_bit_seeds_and_first_samples(hb, seed, begin):
    """(K, S) = (4, 2): the chunk boundary is pass 2, where sample_begin + k carries into the high word, or wraps at 2^64"""
    name = "all_materials"
    gpu, pos, cpu = _gpu(hb, name), PB.positions(name), PB.built(name)[2]
    for method in PB.METHODS:
        values, dirs, rays = PC.samples(cpu, pos, method, seed, begin, 4)
        got, got_rays = gpu.probe_sh(pos, **PB.opts(method, 4, 2, 0, seed, begin))
        assert_same_bits(got, PC.project(values, dirs, 2), f"seed {seed:#x} begin {begin:#x} method {method}", nan_equal=True)
        assert got_rays == int(rays.sum())
    # the low words alone give other coefficients
    low, _ = gpu.probe_sh(pos, **PB.opts(MIS, 4, 2, 0, seed & 0xFFFFFFFF, begin & 0xFFFFFFFF))
    assert low.tobytes() != got.tobytes()


@pytest.mark.parametrize("method", PB.METHODS)
def test_schedules_change_no_byte(hb, method):
    """both traversal modes, both walks, a workgroup cap of one and none: the bytes and the ray count of the first"""
    name = "all_materials"
    ref, ref_rays = PB.many_reference(method, 1)
    for traversal in (0, 1):
        for walk in (0, 1):
            for groups in (1, 0):
                gpu = _gpu(hb, name)
                gpu.set_traversal(traversal)
                gpu.set_tuning(abi.RT_TUNE_WALK, walk)
                gpu.set_tuning(abi.RT_TUNE_RADIANCE_GROUPS, groups)
                got, rays = gpu.probe_sh(PB.many_positions(), **PB.opts(method, PB.MANY_K, PB.MANY_S, 1))
                assert_same_bits(got, ref, f"traversal {traversal} walk {walk} groups {groups}", nan_equal=True)
                assert rays == ref_rays


def test_graph_capture_as_a_fresh_scenes_first_call_and_two_streams(hb):
    import torch
    name = "all_materials"
    pos = PB.positions(name)
    oa, ob = PB.opts(MIS, 4, 2), PB.opts(NAIVE, 7, 3, 1)
    ref_a, ref_b = PB.reference(name, MIS, 4, 2)[0], PB.reference(name, NAIVE, 7, 3, 1)[0]
    gpu = _gpu(hb, name)  # fresh: nothing has run on it
    a, b = _device_buffers(torch, hb, pos, oa, 0), _device_buffers(torch, hb, pos, ob, 0)
    g = capture(torch, lambda s: gpu.probe_sh_device(a.ptr("pos"), len(pos), a.ptr("out"), a.ptr("work"), a.ptr("rays"), stream=s, **oa))
    assert a.untouched("out") and a.untouched("work") and a.untouched("rays")
    for _ in range(2):
        a.buf["out"].fill_(a.guard)
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(a.read("out"), ref_a, "replay", nan_equal=True)
        assert _rays_value(a) == PB.reference(name, MIS, 4, 2)[1]
    # two launches in flight on two streams, two workspaces
    a.buf["out"].fill_(a.guard)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.probe_sh_device(a.ptr("pos"), len(pos), a.ptr("out"), a.ptr("work"), None, stream=s1.cuda_stream, **oa)
    gpu.probe_sh_device(b.ptr("pos"), len(pos), b.ptr("out"), b.ptr("work"), b.ptr("rays"), stream=s2.cuda_stream, **ob)
    torch.cuda.synchronize()
    assert_same_bits(a.read("out"), ref_a, "stream one", nan_equal=True)
    assert_same_bits(b.read("out"), ref_b, "stream two", nan_equal=True)
    assert _rays_value(b) == PB.reference(name, NAIVE, 7, 3, 1)[1]


def test_render_before_and_after_returns_its_own_bytes(hb):
    ls = scenes.load_ssml("rtweekend1")
    gpu, cam = hb.HipScene(ls.scene, device=0), hb.camera_new(**ls.camera_params)
    pos = PB.positions("rtweekend1")

    def between(opts, image):
        coeffs, _ = gpu.probe_sh(pos, **PB.opts(MIS, 4, 2, 1))
        gpu.probe_sh_eval(coeffs, np.eye(3, dtype=F32), [0, 1, 2])
    assert_render_unaffected(gpu, cam, between)


def test_a_multi_device_scene_is_refused(hb):
    gpu = hb.HipScene(PB.built("rtweekend1")[0], devices=[0, 0])
    for call in (lambda: gpu.probe_sh(PB.positions("rtweekend1"), **PB.opts(MIS, 4, 1)),
                 lambda: gpu.probe_sh_eval(np.zeros((1, 9, 3), F32), np.zeros((1, 3), F32))):
        with pytest.raises(hb.RtHipError) as e:
            call()
        assert e.value.code == abi.RT_ERR_UNSUPPORTED


def test_an_empty_batch_writes_nothing(hb):
    gpu = _gpu(hb, "rtweekend1")
    got, rays = gpu.probe_sh(np.zeros((0, 3), F32), **PB.opts(MIS, 4, 2))
    assert got.shape == (0, 9, 3) and rays == 0
    assert gpu.probe_sh_eval(np.zeros((2, 9, 3), F32), np.zeros((0, 3), F32)).shape == (0, 3)


# ---- rt_probe_sh_eval ----
def _eval_inputs():
    rng = np.random.default_rng(5)
    nm = rng.normal(size=(100, 3))
    nm[50:] /= np.linalg.norm(nm[50:], axis=1, keepdims=True)  # half as given, half unit
    return nm.astype(F32), rng.integers(0, 5, 100).astype(np.uint32)


def test_evaluation_is_the_checkers(hb):
    """100 normals with an index list, and the first five without; host and device forms"""
    import torch
    gpu = _gpu(hb, "all_materials")
    coeffs = PB.reference("all_materials", NAIVE, 13, 13, 1)[0]
    nm, idx = _eval_inputs()
    assert_same_bits(gpu.probe_sh_eval(coeffs, nm, idx), PC.evaluate(coeffs, nm, idx), "indexed", nan_equal=False)
    assert_same_bits(gpu.probe_sh_eval(coeffs, nm[:5]), PC.evaluate(coeffs, nm[:5]), "in order", nan_equal=False)
    for off in (1, 0):
        bufs = GuardedBuffers(torch, {"out": ((100, 3), np.float32)}, off=off)
        d_c, d_n = torch.from_numpy(coeffs.copy()).to("cuda:0"), torch.from_numpy(nm.copy()).to("cuda:0")
        d_i = torch.from_numpy(idx.view(np.int32).copy()).to("cuda:0")
        gpu.probe_sh_eval_device(d_c.data_ptr(), 5, d_i.data_ptr(), d_n.data_ptr(), 100, bufs.ptr("out"))
        torch.cuda.synchronize()
        assert_same_bits(bufs.read("out"), PC.evaluate(coeffs, nm, idx), f"device off {off}", nan_equal=False)
        bufs.refill()
        gpu.probe_sh_eval_device(d_c.data_ptr(), 5, None, d_n.data_ptr(), 5, bufs.ptr("out"))
        torch.cuda.synchronize()
        assert_same_bits(bufs.read("out", used=15), PC.evaluate(coeffs, nm[:5]), "device in order", nan_equal=False)


def test_an_index_past_the_probes(hb):
    """the host form refuses the call and writes nothing; the device form writes the quiet NaN to that element alone"""
    import ctypes as C
    import torch
    gpu = _gpu(hb, "all_materials")
    coeffs = PB.reference("all_materials", NAIVE, 13, 13)[0]
    nm, idx = _eval_inputs()
    idx = idx.copy()
    idx[[7, 99]] = (5, 0xFFFFFFFF)
    out = np.full((100, 3), 7.0, F32)
    rc = hb.lib().rt_probe_sh_eval(gpu._h, coeffs.ctypes.data_as(C.c_void_p), C.c_uint64(5), idx.ctypes.data_as(C.c_void_p),
                                   nm.ctypes.data_as(C.c_void_p), C.c_uint64(100), out.ctypes.data_as(C.c_void_p))
    assert rc == abi.RT_ERR_INVALID_ARGUMENT and (out == 7.0).all()
    with pytest.raises(hb.RtHipError) as e:
        gpu.probe_sh_eval(coeffs, nm[:6])  # six normals, five probes, no list
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    bufs = GuardedBuffers(torch, {"out": ((100, 3), np.float32)})
    d_c, d_n = torch.from_numpy(coeffs.copy()).to("cuda:0"), torch.from_numpy(nm.copy()).to("cuda:0")
    d_i = torch.from_numpy(idx.view(np.int32).copy()).to("cuda:0")
    gpu.probe_sh_eval_device(d_c.data_ptr(), 5, d_i.data_ptr(), d_n.data_ptr(), 100, bufs.ptr("out"))
    torch.cuda.synchronize()
    got = bufs.read("out")
    bad = np.zeros(100, bool)
    bad[[7, 99]] = True
    assert (got[bad].view(np.uint32) == 0x7FC00000).all()
    ok = idx.copy()
    ok[bad] = 0
    assert_same_bits(got[~bad], PC.evaluate(coeffs, nm, ok)[~bad], "the other elements", nan_equal=False)


def test_a_uniform_sphere_of_radiance_one(hb):
    """a scene that is nothing but a sky of radiance 1 (one far, tiny, black sphere: a scene needs a primitive): every sample is 1,
    coefficient 0 is 2 sqrt(pi), the others vanish within the estimator's six sigma, and at convolve = 1 every normal sees pi"""
    sc = scenes.SceneDescription()
    sc.sphere((1e6, 1e6, 1e6), 1e-3, sc.lambertian(sc.solid((0.0, 0.0, 0.0)), 0.0))
    sc.set_sky(sc.solid((1.0, 1.0, 1.0)), (0, 0))
    gpu = hb.HipScene(sc, device=0)
    pos = np.zeros((3, 3), F32)
    o = dict(render_method=NAIVE, samples_per_probe=TP.UNIFORM_K, sample_split=64, seed=PB.SEED)
    c, rays = gpu.probe_sh(pos, **o)
    assert rays == 3 * TP.UNIFORM_K  # one ray a sample: every one left into the sky
    assert_same_bits(c, TP.uniform_coefficients(0), "uniform", nan_equal=False)
    assert np.abs(c[:, 0] / (2.0 * np.sqrt(np.pi)) - 1.0).max() <= 1e-5 and np.abs(c[:, 1:]).max() <= TP.UNIFORM_BOUND
    e, _ = gpu.probe_sh(pos, convolve=1, **o)
    rng = np.random.default_rng(3)
    nm = rng.normal(size=(100, 3))
    nm = (nm / np.linalg.norm(nm, axis=1, keepdims=True)).astype(F32)
    got = gpu.probe_sh_eval(e, nm, rng.integers(0, 3, 100))
    assert np.abs(got - np.pi).max() <= TP.eval_bound()
