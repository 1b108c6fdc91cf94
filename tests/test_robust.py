"""Firefly-robust frames (rt_render_robust, rt_robust_combine, rt_render_denoised_robust) without a GPU: the C-ABI boundary on a
host-only scene -- structs, defaults, the status code of every check of the five entry points -- then the numpy checker
(tests/robust_checker.py) held to hand-computed cases and to rt_render's bytes on an oracle frame."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import noise_checker as N
import robust_checker as R
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32
INVALID, UNSUPPORTED, NO_DEVICE = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED, abi.RT_ERR_NO_DEVICE


# ---- the C-ABI boundary ----
def test_struct_sizes_against_a_compiled_sizeof(tmp_path):
    names = {"rt_robust_opts": abi.RobustOpts, "rt_robust_buffers": abi.RobustBuffers}
    src = '#include <stdio.h>\n#include "rt_hip.h"\nint main(void){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + 'printf("abi %u\\n", RT_ABI_VERSION); return 0;}'
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    sizes = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in names.items():
        assert int(sizes[n]) == C.sizeof(cls) == abi.EXPECTED_SIZES[n][1], (n, sizes[n], C.sizeof(cls))
        assert abi.EXPECTED_SIZES[n][0] is cls
    assert C.sizeof(abi.RobustOpts) == 32 and int(sizes["abi"]) == 2


def test_defaults(hb):
    lib = hb.lib()
    o = abi.RobustOpts()
    o.mode, o.trim, o.gini_gain = 7, 9, 3.0
    o.reserved[4] = 9
    assert lib.rt_robust_opts_default(C.byref(o)) == abi.RT_OK
    assert (o.mode, o.trim, o.gini_gain) == (abi.RT_ROBUST_GINI, 1, 1.0) and list(o.reserved) == [0] * 5
    assert bytes(abi.default_robust_opts()) == bytes(o) == bytes(hb.robust_opts())
    assert lib.rt_robust_opts_default(None) == INVALID
    r = hb.robust_opts(mode="median", trim=3)
    assert (r.mode, r.trim, r.gini_gain) == (abi.RT_ROBUST_MEDIAN, 3, 1.0)
    assert (abi.RT_ROBUST_TRIM, abi.RT_ROBUST_MEDIAN, abi.RT_ROBUST_GINI) == (R.TRIM, R.MEDIAN, R.GINI)
    with pytest.raises(ValueError):
        hb.robust_opts(gain=1.0)
    with pytest.raises(ValueError):
        hb.robust_opts(mode="mean")
    for name in abi.EXPORTED_SYMBOLS:
        if "robust" in name:
            assert hasattr(lib, name), name
    assert sum("robust" in name for name in abi.EXPORTED_SYMBOLS) == 6


def _arrays(w, h, split=2):
    n = w * h
    keep = {"out": np.zeros(3 * n, F32), "mean": np.zeros(3 * n, F32), "gini": np.zeros(n, F32), "trimmed": np.zeros(n, np.uint8),
            "dropped": np.zeros(n, np.uint8), "albedo": np.zeros(3 * n, F32), "sums": np.zeros(3 * n * split, F32)}
    b = abi.RobustBuffers()
    for name in ("out", "mean", "gini"):
        setattr(b, name, keep[name].ctypes.data_as(C.POINTER(C.c_float)))
    for name in ("trimmed", "dropped"):
        setattr(b, name, keep[name].ctypes.data_as(C.POINTER(C.c_uint8)))
    return b, keep


def _at(array, index, ctype=C.c_float):
    return C.cast(C.c_void_p(array.ctypes.data + array.itemsize * index), C.POINTER(ctype))


def _opts(w, h, spp, split):
    o = abi.default_render_opts(w, h, spp)
    o.sample_split = split
    return o


def _bad_options():
    bad = [abi.default_robust_opts(mode=3), abi.default_robust_opts(mode=-1)]
    bad += [abi.default_robust_opts(gini_gain=g) for g in (0.0, -1.0, np.nan, np.inf, -np.inf)]
    bad += [abi.default_robust_opts(mode=abi.RT_ROBUST_TRIM, gini_gain=0.0)]  # checked in every mode
    for word in range(5):
        r = abi.default_robust_opts()
        r.reserved[word] = 1
        bad.append(r)
    return bad


def _overlaps(w, h, make):
    """buffer sets in which one written buffer ends on the last value of another buffer: every pair of the five outputs"""
    n = w * h
    last = {"out": 3 * n - 1, "mean": 3 * n - 1, "gini": n - 1, "trimmed": n - 1, "dropped": n - 1}
    ctype = {"out": C.c_float, "mean": C.c_float, "gini": C.c_float, "trimmed": C.c_uint8, "dropped": C.c_uint8}
    for moved in last:
        for onto in last:
            if moved != onto:
                b, keep = make()
                setattr(b, moved, _at(keep[onto], last[onto], ctype[moved]))
                yield f"{moved} on {onto}", b, keep


@pytest.fixture(scope="module")
def host_only(hb):
    ls = scenes.load_ssml("rtweekend1")
    return hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE), hb.camera_new(**ls.camera_params)


def test_render_robust_status_codes_and_the_split_rule_without_a_device(hb, host_only):
    s, cam = host_only
    lib = hb.lib()
    w, h = 16, 9
    n_px = w * h
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731

    def call(opts, ropts, bufs, device, albedo=None, scene=s._h, camera=cam):
        if device:
            return lib.rt_render_robust_device(scene, ref(camera), ref(opts), ref(ropts), albedo, ref(bufs), None, C.c_void_p(0))
        return lib.rt_render_robust(scene, ref(camera), ref(opts), ref(ropts), albedo, ref(bufs), None)

    ro = abi.default_robust_opts()
    for device in (False, True):
        full, keep = _arrays(w, h)
        ok = _opts(w, h, 8, 2)
        assert call(ok, ro, full, device) == NO_DEVICE
        assert call(ok, ro, full, device, albedo=_at(keep["albedo"], 0)) == NO_DEVICE
        for mode in (abi.RT_ROBUST_TRIM, abi.RT_ROBUST_MEDIAN, abi.RT_ROBUST_GINI):
            assert call(ok, abi.default_robust_opts(mode=mode, trim=1000, gini_gain=1e30), full, device) == NO_DEVICE
        only_out = abi.RobustBuffers()
        only_out.out = full.out
        assert call(ok, ro, only_out, device) == NO_DEVICE  # any field but out may be NULL
        no_out, _ = _arrays(w, h)
        no_out.out = None
        assert call(ok, ro, no_out, device) == INVALID
        for args in ((None, ro, full), (ok, None, full), (ok, ro, None)):
            assert call(*args, device) == INVALID
        assert call(ok, ro, full, device, scene=None) == INVALID
        assert call(ok, ro, full, device, camera=None) == INVALID
        # the split rule of the noise estimates
        for spp, split in ((8, 2), (8, 4), (8, 8), (64, 64), (6, 3), (1024, 0), (32, 0), (100, 0), (102, 0)):
            assert call(_opts(w, h, spp, split), ro, full, device) == NO_DEVICE, (spp, split)
        for spp, split in ((8, 3), (8, 1), (7, 0), (1, 0), (33, 0), (8, 0), (8, 16), (128, 128), (130, 65), (8, 5), (0, 2), (1 << 32, 2)):
            assert call(_opts(w, h, spp, split), ro, full, device) == INVALID, (spp, split)
        for bad in _bad_options():
            assert call(ok, bad, full, device) == INVALID, bytes(bad)
        assert call(ok, abi.default_robust_opts(gini_gain=1e-30), full, device) == NO_DEVICE
        # overlap: an output on the last value of another output or of the albedo; just behind it is fine
        for what, b, keep in _overlaps(w, h, lambda: _arrays(w, h)):
            assert call(ok, ro, b, device) == INVALID, what
        for name, last in (("out", 3 * n_px - 1), ("mean", 3 * n_px - 1), ("gini", n_px - 1), ("trimmed", n_px - 1), ("dropped", n_px - 1)):
            b, keep = _arrays(w, h)
            assert call(ok, ro, b, device, albedo=_at(keep[name], last)) == INVALID, name
        big = np.zeros(7 * n_px + 2, F32)
        b, keep = _arrays(w, h)
        b.out, b.mean, b.gini = _at(big, 0), _at(big, 3 * n_px), _at(big, 6 * n_px)
        b.trimmed = C.cast(C.c_void_p(big.ctypes.data + 28 * n_px), C.POINTER(C.c_uint8))
        b.dropped = C.cast(C.c_void_p(big.ctypes.data + 29 * n_px), C.POINTER(C.c_uint8))
        assert call(ok, ro, b, device) == NO_DEVICE
        # the frame
        o = _opts(w, h, 8, 2)
        o.output_layout = abi.RT_LAYOUT_SHARD
        assert call(o, ro, full, device) == UNSUPPORTED
        o = _opts(w, h, 8, 2)
        o.shard_count = 2
        assert call(o, ro, full, device) == UNSUPPORTED
        assert call(_opts(1, h, 8, 2), ro, full, device) == INVALID
        assert call(_opts(w, 1, 8, 2), ro, full, device) == INVALID
        o = _opts(w, h, 8, 2)
        o.render_method = 7
        assert call(o, ro, full, device) == INVALID
    # the Python binding
    for opts, code in ((_opts(w, h, 8, 2), NO_DEVICE), (_opts(w, h, 8, 3), INVALID), (_opts(w, h, 7, 0), INVALID), (_opts(w, h, 8, 1), INVALID)):
        with pytest.raises(hb.RtHipError) as e:
            s.render_robust(cam, opts)
        assert e.value.code == code
    with pytest.raises(hb.RtHipError) as e:
        s.render_robust(cam, _opts(w, h, 8, 2), mode="gini", gini_gain=0.0)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        s.render_robust(cam, _opts(w, h, 8, 2), channels=("variance",))


def test_robust_combine_status_codes_without_a_device(hb, host_only):
    s, _ = host_only
    lib = hb.lib()
    w, h, split = 13, 11, 4
    n_px = w * h
    ro = abi.default_robust_opts()

    def call(device, bufs, keep, sums="default", split=split, chunk_passes=2, width=w, height=h, albedo=None, ropts=ro, scene=s._h):
        f = lib.rt_robust_combine_device if device else lib.rt_robust_combine
        args = (scene, _at(keep["sums"], 0) if isinstance(sums, str) else sums, C.c_uint32(split), C.c_uint64(chunk_passes), C.c_uint32(width),
                C.c_uint32(height), albedo, C.byref(ropts) if ropts is not None else None, C.byref(bufs) if bufs is not None else None)
        return f(*args, C.c_void_p(0)) if device else f(*args)

    for device in (False, True):
        full, keep = _arrays(w, h, split)
        assert call(device, full, keep) == NO_DEVICE
        assert call(device, full, keep, albedo=_at(keep["albedo"], 0)) == NO_DEVICE
        only_out = abi.RobustBuffers()
        only_out.out = full.out
        assert call(device, only_out, keep) == NO_DEVICE
        one, keep1 = _arrays(1, 1, 2)
        assert call(device, one, keep1, split=2, width=1, height=1) == NO_DEVICE  # a frame of one pixel is a frame
        big, keepb = _arrays(w, h, 64)
        assert call(device, big, keepb, split=64, chunk_passes=(1 << 26) - 1) == NO_DEVICE
        assert call(device, big, keepb, split=64, chunk_passes=1 << 26) == INVALID  # split * chunk_passes = 2^32
        assert call(device, full, keep, split=2, chunk_passes=(1 << 31) - 1) == NO_DEVICE
        assert call(device, full, keep, split=2, chunk_passes=1 << 31) == INVALID
        assert call(device, full, keep, chunk_passes=1 << 32) == INVALID and call(device, full, keep, chunk_passes=(1 << 62)) == INVALID
        assert call(device, full, keep, chunk_passes=0) == INVALID
        assert call(device, full, keep, split=1) == INVALID and call(device, full, keep, split=0) == INVALID
        assert call(device, big, keepb, split=65) == INVALID
        assert call(device, full, keep, split=3) == NO_DEVICE  # nothing divides here: any 2..64
        assert call(device, full, keep, width=0) == INVALID and call(device, full, keep, height=0) == INVALID
        assert call(device, full, keep, width=1 << 16, height=(1 << 15) + 1) == UNSUPPORTED
        assert call(device, full, keep, sums=None) == INVALID and call(device, None, keep) == INVALID
        assert call(device, full, keep, ropts=None) == INVALID and call(device, full, keep, scene=None) == INVALID
        no_out, keep2 = _arrays(w, h, split)
        no_out.out = None
        assert call(device, no_out, keep2) == INVALID
        for bad in _bad_options():
            assert call(device, full, keep, ropts=bad) == INVALID, bytes(bad)
        for what, b, k in _overlaps(w, h, lambda: _arrays(w, h, split)):
            assert call(device, b, k) == INVALID, what
        # an output on the last value of the chunk sums or of the albedo
        for name, ctype in (("out", C.c_float), ("mean", C.c_float), ("gini", C.c_float), ("trimmed", C.c_uint8), ("dropped", C.c_uint8)):
            b, k = _arrays(w, h, split)
            setattr(b, name, _at(k["sums"], 3 * n_px * split - 1, ctype))
            assert call(device, b, k) == INVALID, name
            b, k = _arrays(w, h, split)
            setattr(b, name, _at(k["albedo"], 3 * n_px - 1, ctype))
            assert call(device, b, k, albedo=_at(k["albedo"], 0)) == INVALID, name
        assert call(device, full, keep, albedo=_at(keep["sums"], 0)) == NO_DEVICE  # two buffers that are only read may share memory
    with pytest.raises(hb.RtHipError) as e:
        s.robust_combine(np.zeros((4, 3, 5, 3), F32), 2)
    assert e.value.code == NO_DEVICE
    with pytest.raises(hb.RtHipError) as e:
        s.robust_combine(np.zeros((1, 3, 5, 3), F32), 2)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        s.robust_combine(np.zeros((4, 3, 5), F32), 2)


def test_denoised_robust_status_codes_without_a_device(hb, host_only):
    s, cam = host_only
    lib = hb.lib()
    w, h = 16, 9
    n_px = w * h
    clean, robust = np.zeros(3 * n_px, F32), np.zeros(3 * n_px, F32)
    d, ro = abi.default_denoise_opts(), abi.default_robust_opts()

    def den(opts, ropts=ro, dopts=d, clean_p=_at(clean, 0), robust_p=_at(robust, 0), camera=cam):
        return lib.rt_render_denoised_robust(s._h, C.byref(camera) if camera is not None else None, C.byref(opts),
                                             C.byref(ropts) if ropts is not None else None, C.byref(dopts) if dopts is not None else None,
                                             clean_p, robust_p, None)

    ok = _opts(w, h, 8, 4)
    assert den(ok) == NO_DEVICE and den(ok, robust_p=None) == NO_DEVICE
    assert den(ok, clean_p=None) == INVALID and den(ok, dopts=None) == INVALID and den(ok, ropts=None) == INVALID and den(ok, camera=None) == INVALID
    assert den(_opts(w, h, 8, 3)) == INVALID and den(_opts(w, h, 7, 0)) == INVALID and den(_opts(w, h, 8, 1)) == INVALID
    assert den(ok, dopts=abi.default_denoise_opts(iterations=11)) == INVALID
    for bad in _bad_options():
        assert den(ok, ropts=bad) == INVALID, bytes(bad)
    assert den(ok, robust_p=_at(clean, 3 * n_px - 1)) == INVALID
    o = _opts(w, h, 8, 4)
    o.output_layout = abi.RT_LAYOUT_SHARD
    assert den(o) == UNSUPPORTED
    o = _opts(w, h, 8, 4)
    o.shard_count = 2
    assert den(o) == UNSUPPORTED
    with pytest.raises(hb.RtHipError) as e:
        s.render_denoised_robust(cam, ok, mode="trim")
    assert e.value.code == NO_DEVICE


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() { rt_hip::RobustOptions r; r.mode = RT_ROBUST_MEDIAN; r.trim = 2; r.gini_gain = 0.5f;\n'
           'rt_hip::RobustFrame (*f)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, uint32_t, '
           'const rt_hip::RobustOptions &, uint64_t, uint64_t) = &rt_hip::render_robust; (void)f;\n'
           'rt_hip::RobustFrame (*g)(const rt_hip::Bvh &, const std::vector<float> &, uint32_t, uint64_t, uint32_t, uint32_t, '
           'const rt_hip::RobustOptions &) = &rt_hip::robust_combine; (void)g;\n'
           'rt_hip::RobustFrame e; return (int)(e.out.size() + e.mean.size() + e.gini.size() + e.trimmed.size() + e.dropped.size() + e.rays_shot); }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)


# ---- the checker against hand-computed cases ----
def _pixel(values, n=1):
    """S chunk sums of ONE grey pixel whose chunk luminances are `values` (lum of a grey v is not v exactly: the weights do not sum
    to 1 in f32 -- the tests below compare luminances through R.luminances, never to `values`)"""
    v = np.asarray(values, F32)
    return np.repeat(v[:, None, None, None], 3, axis=3) * F32(n)


def _random_sums(split, seed=0, shape=(5, 7)):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 4.0, (split,) + shape + (3,)).astype(F32)


def test_no_trim_gives_the_bits_of_the_plain_combine():
    for split, n in ((2, 4), (3, 1), (8, 2), (16, 1), (64, 1)):
        sums = _random_sums(split, seed=split)
        for kw in (dict(mode=R.TRIM, trim=0), dict(mode=R.GINI, gini_gain=1e-30)):
            got = R.robust(sums, n, **kw)
            assert got["out"].tobytes() == N.combine(sums, split * n).tobytes() == got["mean"].tobytes(), (split, kw)
            assert not got["trimmed"].any() and not got["dropped"].any()
            assert got["out"].dtype == got["mean"].dtype == got["gini"].dtype == F32
            assert got["trimmed"].dtype == got["dropped"].dtype == np.uint8


def test_three_chunks_under_median_give_the_middle_chunk():
    sums = _random_sums(3, seed=1)
    l = R.luminances(sums, 4)
    middle = np.argsort(l, axis=0, kind="stable")[1]
    got = R.robust(sums, 4, mode=R.MEDIAN)
    expected = np.take_along_axis(sums, middle[None, ..., None], axis=0)[0] / F32(4)
    assert got["out"].tobytes() == expected.tobytes() and (got["trimmed"] == 1).all()


def test_equal_chunks_rank_by_index_and_keep_the_central_indices():
    for split in (4, 5, 8, 16):
        sums = _pixel([0.5] * split)
        got = R.robust(sums, 1, mode=R.MEDIAN)
        assert got["ranks"][:, 0, 0].tolist() == list(range(split))
        t = (split - 1) // 2
        assert got["trimmed"][0, 0] == t and np.flatnonzero(got["kept"][:, 0, 0]).tolist() == list(range(t, split - t))
        assert (got["out"] == F32(0.5)).all() and got["gini"][0, 0] <= 1e-6  # (the coefficients cancel up to rounding)
        one = R.robust(sums, 1, mode=R.TRIM, trim=1)
        assert np.flatnonzero(one["kept"][:, 0, 0]).tolist() == list(range(1, split - 1))


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_non_finite_chunk_is_dropped_and_counted(poison):
    sums = _random_sums(8, seed=2, shape=(3, 4))
    clean = R.robust(sums, 2, mode=R.TRIM, trim=0)
    bad = sums.copy()
    bad[5, 1, 2, 1] = poison  # one channel of one chunk of pixel (1, 2)
    got = R.robust(bad, 2, mode=R.TRIM, trim=0)
    assert got["dropped"][1, 2] == 1 and got["dropped"].sum() == 1 and got["ranks"][5, 1, 2] == 7
    others = [c for c in range(8) if c != 5]
    acc = np.zeros(3, F32)
    for c in others:
        acc = acc + sums[c, 1, 2]
    assert got["out"][1, 2].tobytes() == (acc / F32(14)).tobytes() and np.isfinite(got["out"]).all()
    assert not np.isfinite(got["mean"][1, 2]).all()  # the plain combine carries the poison
    untouched = np.ones((3, 4), bool)
    untouched[1, 2] = False
    for k in ("out", "mean", "gini", "trimmed", "dropped"):
        assert got[k][untouched].tobytes() == clean[k][untouched].tobytes(), k  # the neighbours are left alone
    # tmax follows S_f = 7: the median keeps one chunk
    med = R.robust(bad, 2, mode=R.MEDIAN)
    assert med["trimmed"][1, 2] == 3 and med["kept"][:, 1, 2].sum() == 1 and med["trimmed"][0, 0] == 3 and med["kept"][:, 0, 0].sum() == 2


def test_all_chunks_non_finite_give_the_plain_combine():
    sums = _random_sums(4, seed=3, shape=(2, 2))
    sums[:, 0, 1, 0] = [np.nan, np.inf, -np.inf, np.inf]
    for mode in (R.TRIM, R.MEDIAN, R.GINI):
        got = R.robust(sums, 2, mode=mode)
        assert got["dropped"][0, 1] == 4 and got["trimmed"][0, 1] == 0 and got["gini"][0, 1] == 0.0
        assert np.isnan(got["out"][0, 1, 0]) and got["out"][0, 1].tobytes() == N.combine(sums, 8)[0, 1].tobytes()
        assert got["ranks"][:, 0, 1].tolist() == [0, 1, 2, 3]  # all keys equal: by index


def test_minus_zero_ranks_below_plus_zero():
    sums = _pixel([0.0, -0.0, 0.0, -0.0])
    l = R.luminances(sums, 1)[:, 0, 0]
    assert np.signbit(l).tolist() == [False, True, False, True]
    k = R.keys(l)
    assert k.tolist() == [0x80000000, 0x7FFFFFFF, 0x80000000, 0x7FFFFFFF]
    assert R.robust(sums, 1)["ranks"][:, 0, 0].tolist() == [2, 0, 3, 1]
    # and the keys order as the values do
    v = np.array([-np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.5, 3.4e38, np.inf, np.nan], F32)
    k = R.keys(v)
    assert (np.diff(k[1:8].astype(np.int64)) > 0).all() and (k[[0, 8, 9]] == 0xFFFFFFFF).all()


def test_the_gini_coefficient_and_trim_count_of_one_outlier():
    """seven zero chunks and one of luminance l: ranks 0 .. 6 by index and 7; A = 7 l, B = l, G = 7 l / (8 l) = 7/8 -- up to the
    rounding of 7 l and of the quotient, one ulp of 7/8 each at the most; tmax = 3, t = floor(7/8 * 3) = floor(2.625) = 2.
    The same shape at S = 4: G = 3/4, tmax = 1, t = floor(3/4) = 0."""
    ulp = 2.0 ** -24  # of a value in [0.5, 1)
    for x in (1.0, 1024.0, 2.0 ** -20):
        got = R.robust(_pixel([0, 0, x, 0, 0, 0, 0, 0]), 1)
        assert abs(float(got["G"][0, 0]) - 0.875) <= 2 * ulp and got["G"][0, 0] == got["gini"][0, 0] and got["trimmed"][0, 0] == 2
        assert got["ranks"][:, 0, 0].tolist() == [0, 1, 7, 2, 3, 4, 5, 6]
        assert np.flatnonzero(got["kept"][:, 0, 0]).tolist() == [3, 4, 5, 6] and (got["out"] == 0.0).all()
        assert got["mean"][0, 0, 0] == F32(x) / F32(8)
        four = R.robust(_pixel([0, x, 0, 0]), 1)
        assert abs(float(four["G"][0, 0]) - 0.75) <= 2 * ulp and four["trimmed"][0, 0] == 0
        assert four["out"].tobytes() == four["mean"].tobytes()
        # the gain scales the trim count, capped at tmax
        assert R.robust(_pixel([0, 0, x, 0, 0, 0, 0, 0]), 1, gini_gain=100.0)["trimmed"][0, 0] == 3
        assert R.robust(_pixel([0, 0, x, 0, 0, 0, 0, 0]), 1, gini_gain=0.5)["trimmed"][0, 0] == 1
        assert R.robust(_pixel([0, x, 0, 0]), 1, gini_gain=2.0)["trimmed"][0, 0] == 1


def test_an_all_black_pixel_has_no_inequality():
    for split in (2, 4, 8):
        got = R.robust(_pixel([0.0] * split), 3)
        assert np.isnan(got["G"][0, 0]) and got["gini"][0, 0] == 0.0 and not np.signbit(got["gini"][0, 0])
        assert got["trimmed"][0, 0] == 0 and (got["out"] == 0.0).all()
    neg = R.robust(_pixel([-1.0, -2.0, -3.0, -4.0]), 1)  # negative luminances: G < 0 clamps to 0
    assert neg["G"][0, 0] < 0 and neg["gini"][0, 0] == 0.0 and neg["ranks"][:, 0, 0].tolist() == [3, 2, 1, 0]


@pytest.mark.parametrize("kw", [dict(mode=R.TRIM, trim=1), dict(mode=R.MEDIAN)])
def test_raising_the_top_chunk_leaves_the_output_bit_identical(kw):
    for split in (4, 7, 16):
        sums = _random_sums(split, seed=10 + split)
        base = R.robust(sums, 2, **kw)
        top = np.argmax(base["ranks"], axis=0)
        for factor in (1.5, 1e6, 1e30):
            raised = sums.copy()
            idx = np.indices(top.shape)
            raised[top, idx[0], idx[1]] = sums[top, idx[0], idx[1]] * F32(factor)
            assert np.isfinite(R.luminances(raised, 2)).all()
            got = R.robust(raised, 2, **kw)
            assert got["out"].tobytes() == base["out"].tobytes(), (split, factor)
            assert got["mean"].tobytes() != base["mean"].tobytes()


def test_two_chunks_equal_the_plain_combine_in_every_mode():
    sums = _random_sums(2, seed=4)
    sums[1, 0, 0] = sums[0, 0, 0] * F32(1e6)
    for kw in (dict(mode=R.TRIM, trim=5), dict(mode=R.MEDIAN), dict(mode=R.GINI, gini_gain=1e9)):
        got = R.robust(sums, 16, **kw)
        assert got["out"].tobytes() == N.combine(sums, 32).tobytes() and not got["trimmed"].any()


def test_an_albedo_changes_the_ranking_not_the_sums():
    sums = np.zeros((3, 1, 1, 3), F32)
    sums[0, 0, 0], sums[1, 0, 0], sums[2, 0, 0] = (3, 0, 0), (0, 1, 0), (0, 0, 8)  # lum 0.64, 0.72, 0.58
    assert R.robust(sums, 1, mode=R.MEDIAN)["out"][0, 0].tolist() == [3, 0, 0]
    albedo = np.array([[[1.0, 1.0, 0.0]]], F32)  # blue floored at 1e-3: chunk 2 is now the brightest, chunk 1 the median
    assert R.robust(sums, 1, albedo, mode=R.MEDIAN)["out"][0, 0].tolist() == [0, 1, 0]


# ---- on the oracle's frame ----
@pytest.mark.parametrize("method", [abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS])
def test_untrimmed_pixels_of_an_oracle_frame_have_rt_renders_bits(O, method):
    w, h, spp = 24, 20, 32
    cpu = O.Scene(scenes.all_materials())
    cam = O.camera_new(**scenes.ALL_MATERIALS_CAMERA)
    o = abi.default_render_opts(w, h, spp, method=method, seed=3)
    passes = N.passes(cpu, cam, o, spp)
    for split in (8, 16):
        sums = N.chunk_sums(passes, split)
        o.sample_split = split
        image = cpu.render(cam, o, n_threads=1)[0]  # the oracle's own render at that split
        got = R.robust(sums, spp // split)
        assert got["mean"].tobytes() == image.tobytes()
        untrimmed = (got["trimmed"] == 0) & (got["dropped"] == 0)
        n_trimmed = int((got["trimmed"] > 0).sum())
        print(f"method {method} S={split}: {n_trimmed} of {w * h} pixels trimmed, {int(got['dropped'].astype(bool).sum())} with dropped chunks")
        assert got["out"][untrimmed].tobytes() == image[untrimmed].tobytes()
        assert n_trimmed >= 1 and untrimmed.any()
