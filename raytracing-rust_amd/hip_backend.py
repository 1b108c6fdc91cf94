"""Host-side binding of librt_hip.so (the HIP back end) -- the Python twin of the Rust
`extern "C"` block in INTEGRATION.md.

`HipScene` stands where the reference's `Bvh` + `Scene` stand (crates/implementations/src/
acceleration/mod.rs:44-93, src/scene.rs:7-42); `RandomSampler.sample_image` keeps the
reference's trait-method shape (samplers/mod.rs:7-20) including the per-pass callback.

There is no CPU fallback: if the shared library is missing, or no HIP device is present,
every call raises.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(_HERE, "librt_hip.so")  # RT_HIP_LIB: A/B builds
_LIB = None


class RtHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"rt_hip error {code}: {message}")
        self.code = code


def lib():
    """Load librt_hip.so (built by __graft_entry__.build() / csrc/Makefile).  Raises if absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RtHipError(abi.RT_ERR_NO_DEVICE, f"{LIB_PATH} not built (run `make -C raytracing-rust_amd/csrc`); "
                             "the HIP back end has no CPU fallback")
        # PyTorch-ROCm ships its own HIP/HSA runtime.  A process that uses both (bench.py, the RCCL gather,
        # the HIP-graph test) must have torch's copy loaded BEFORE librt_hip.so pulls in /opt/rocm's: in the
        # reverse order torch later finds "No HIP GPUs".  So if torch is installed, import it first.
        if "torch" not in sys.modules and os.environ.get("RT_HIP_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        _LIB = C.CDLL(LIB_PATH)
        _LIB.rt_last_error.restype = C.c_char_p
        _LIB.rt_abi_version.restype = C.c_uint32
    return _LIB


def _check(rc):
    if rc != 0:
        raise RtHipError(rc, lib().rt_last_error().decode())


def _p(a, t):
    """a numpy array (None = not given) as a typed ctypes pointer"""
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _ref(s):
    """byref of a ctypes struct (None = not given)"""
    return None if s is None else C.byref(s)


def _vp(ptr):
    """a device address (an int, 0 / None = not given) as a void pointer"""
    return C.c_void_p(int(ptr)) if ptr else None


def _dp(ptr, ctype=C.c_float):
    """a device address (an int, 0 / None = not given) as a typed ctypes pointer"""
    return C.cast(_vp(ptr), C.POINTER(ctype)) if ptr else None


def _known(key, allowed, what):
    if key not in allowed:
        raise ValueError(f"unknown {what} {key!r}: one of {sorted(allowed)}")


def _f32(a, shape, name):
    """`a` (None = not given) as a contiguous f32 array, which must have exactly `shape`"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != shape:
        raise ValueError(f"{name} must be {shape}, got {a.shape}")
    return a


def _image(image, name="image"):
    """(the frame as a contiguous f32 array, h, w) of an (H, W, 3) frame"""
    a = np.ascontiguousarray(image, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{name} must be (H, W, 3), got {a.shape}")
    return a, a.shape[0], a.shape[1]


def _guides(color, albedo, **named):
    """(color, {guide: array or None}) of denoise / denoise_temporal, whose guides may come by name or as the dict render_aov
    returns, either in place of `albedo` or, with the image under "color", in place of `color`"""
    guides = {}
    if isinstance(color, dict):  # denoise({"color": ..., **scene.render_aov(...)})
        guides, color = color, color["color"]
    elif isinstance(albedo, dict):  # denoise(color, scene.render_aov(...))
        guides, albedo = albedo, None
    return color, {k: guides.get(k, v) for k, v in dict(albedo=albedo, **named).items()}


def _shape(kind, h, w, layers=0):
    """the array shape an abi channel table names, for an h x w frame"""
    return {"hw": (h, w), "hw3": (h, w, 3), "lhw": (layers, h, w), "tiles": ((h + 7) // 8, (w + 7) // 8)}[kind]


def _host_buffers(table, bufs, channels, h, w, layers=0):
    """{channel: zeroed array} for the `channels` (repeats count once) of an abi channel table at h x w, with the pointers of
    the struct `bufs` set to them; a "summary" channel is its struct, for _summary_dict once the library has filled it"""
    known = abi.channels(table, bufs)
    out = {}
    for name in channels:
        _known(name, known, "channel")
        holder, ctype, kind = known[name]
        if name in out:
            continue
        if kind == "summary":
            out[name] = ctype()
            setattr(holder, name, C.pointer(out[name]))
        else:
            out[name] = np.zeros(_shape(kind, h, w, layers), dtype=np.dtype(ctype))
            setattr(holder, name, _p(out[name], ctype))
    return out


def _host_inputs(table, ins, arrays, h, w):
    """the pointers of the struct `ins` set to `arrays` ({input: array or None}) as contiguous f32 of the shapes the abi channel
    table gives them at h x w; `ins` keeps the arrays alive"""
    known = abi.channels(table, ins)
    ins._arrays = getattr(ins, "_arrays", [])
    for name, a in arrays.items():
        holder, ctype, kind = known[name]
        ins._arrays.append(_f32(a, _shape(kind, h, w), name))
        setattr(holder, name, _p(ins._arrays[-1], ctype))


def _device_buffers(table, bufs, d_ptrs):
    """`bufs` with the pointers of d_ptrs ({channel: device address}) set, each typed as the struct's field"""
    known = abi.channels(table, bufs)
    for name, ptr in d_ptrs.items():
        _known(name, known, "channel")
        holder, ctype, _ = known[name]
        setattr(holder, name, _dp(ptr, ctype))
    return bufs


def _u64(symbol, opts):
    """the uint64 a query `symbol(const opts *, uint64_t *)` of the library answers"""
    n = C.c_uint64()
    _check(getattr(lib(), symbol)(C.byref(opts), C.byref(n)))
    return n.value


def _f3(v):
    return (C.c_float * 3)(*[float(np.float32(x)) for x in v])


def _in_use(names, mask):
    """the names (an abi *_FORM_NAMES table) whose bit a self-test's `in_use` word has set"""
    return [n for k, n in enumerate(names) if mask >> k & 1]


def _selftest_cases(test, cases, device, *lead):
    """{count name: value} of the self-test `test` of abi.SELFTEST_CASE_TABLES on `cases` (n, width); `lead`: what the entry point
    takes between the device and the cases; "in_use" comes back as the names of its bits"""
    symbol, ctype, width, what, names, forms = abi.SELFTEST_CASE_TABLES[test]
    cases = np.ascontiguousarray(cases, dtype=np.dtype(ctype))
    if cases.ndim != 2 or cases.shape[1] != width:
        raise ValueError(f"{what} must be (n, {width}), got {cases.shape}")
    out = (C.c_uint64 * len(names))()
    _check(getattr(lib(), symbol)(C.c_int(device), *lead, _p(cases, ctype), C.c_uint64(cases.shape[0]), out))
    res = dict(zip(names, (int(x) for x in out)))
    if forms is not None:
        res["in_use"] = _in_use(forms, res["in_use"])
    return res


def rccl_probe():
    """(usable, note): which RCCL a multi-device scene would bind (rt_rccl_probe; touches no GPU)"""
    usable, note = C.c_int(), C.create_string_buffer(512)
    _check(lib().rt_rccl_probe(C.byref(usable), note, C.c_uint64(512)))
    return bool(usable.value), note.value.decode()


def device_count():
    return int(lib().rt_device_count())


def selftest_lean(device=0, n_per_thread=64, seed=1):
    """rt_selftest_lean: mismatch counts per operand class between the kernels' short arithmetic forms
    (csrc/rt_lean.h) and the plain IEEE operators / rt_detmath.h, evaluated on the GPU.  All must be zero."""
    out = (C.c_uint64 * 9)()
    _check(lib().rt_selftest_lean(C.c_int(device), C.c_uint64(n_per_thread), C.c_uint64(seed), out))
    return [int(x) for x in out]


def selftest_short_forms(device=0, operands=None):
    """rt_selftest_short_forms.  operands None: the enumeration of every short form of csrc/rt_lean.h that rests on gfx950's
    v_rcp_f32 / v_sqrt_f32 against the plain operators -- {"forms": {name: (tested, mismatches, first mismatching input's bits or
    None)}, "sqrt_raw": {"exact", "high", "low", "other"}, "in_use": names of the forms the render kernels use}.  With operands
    (f32 values): {"sites": {name: mismatches}, "tested": n} of the guarded call sites on directions built from them."""
    res = abi.ShortFormsResult()
    if operands is None:
        _check(lib().rt_selftest_short_forms(C.c_int(device), None, C.c_uint64(0), C.byref(res)))
        forms = {name: (int(f.tested), int(f.mismatches), int(f.first_mismatch) if f.mismatches else None)
                 for name, f in zip(abi.SHORT_FORM_NAMES, res.form)}
        raw = {k: int(getattr(res, "sqrt_raw_" + k)) for k in ("exact", "high", "low", "other")}
        return {"forms": forms, "sqrt_raw": raw, "in_use": _in_use(abi.SHORT_FORM_NAMES, res.in_use)}
    ops = np.ascontiguousarray(operands, dtype=np.float32).ravel()
    _check(lib().rt_selftest_short_forms(C.c_int(device), _p(ops, C.c_float), C.c_uint64(ops.size), C.byref(res)))
    return {"sites": dict(zip(abi.SHORT_SITE_NAMES, (int(x) for x in res.site_mismatches))), "tested": int(res.site_tested)}


def selftest_div_forms(denominators=None, exponents=((0, 0),), first_denominator=0, n_denominators=None, operands=None, device=0):
    """rt_selftest_div_forms.  Without operands, the enumeration of the quotient forms of csrc/rt_lean.h against `n / d`: every
    denominator significand of the list `denominators` (or of the range first_denominator + [0, n_denominators)) x all 2^23
    numerator significands x every (numerator exponent, denominator exponent) of `exponents` -- {"tested", "forms": {name:
    (mismatches, (numerator bits, denominator bits) of the first one or None)}, "in_use": names of the forms the render kernels'
    guarded divisions use}.  With operands ((n, 2) f32 pairs (n, d)): {"tested", "in_domain", "sites": {name: mismatches}} of the
    wrappers and the guarded call sites on them."""
    res = abi.DivFormsResult()
    if operands is not None:
        ops = np.ascontiguousarray(operands, dtype=np.float32)
        if ops.ndim != 2 or ops.shape[1] != 2:
            raise ValueError(f"operands must be (n, 2), got {ops.shape}")
        _check(lib().rt_selftest_div_forms(C.c_int(device), None, _p(ops, C.c_float), C.c_uint64(ops.shape[0]), C.byref(res)))
        return {"tested": int(res.site_tested), "in_domain": int(res.site_in_domain),
                "sites": dict(zip(abi.DIV_SITE_NAMES, (int(x) for x in res.site_mismatches)))}
    exps = np.ascontiguousarray(exponents, dtype=np.int32).reshape(-1, 2)
    sl = abi.DivFormsSlice()
    sl.exponents, sl.n_exponent_pairs = _p(exps, C.c_int32), exps.shape[0]
    if denominators is not None:
        dens = np.ascontiguousarray(denominators, dtype=np.uint32).ravel()
        sl.denominators, sl.n_denominators = _p(dens, C.c_uint32), dens.size
    else:
        sl.denominators, sl.n_denominators, sl.first_denominator = None, int(n_denominators), int(first_denominator)
    _check(lib().rt_selftest_div_forms(C.c_int(device), C.byref(sl), None, C.c_uint64(0), C.byref(res)))
    forms = {name: (int(res.mismatches[k]), (int(res.first_numerator[k]), int(res.first_denominator[k])) if res.mismatches[k] else None)
             for k, name in enumerate(abi.DIV_FORM_NAMES)}
    return {"tested": int(res.tested), "forms": forms, "in_use": _in_use(abi.DIV_FORM_NAMES, res.in_use)}


def selftest_sky_pdf_forms(scene, dirs):
    """rt_selftest_sky_pdf_forms: (pdf as the two-sphere kernels instantiate sky_pdf, pdf of the default instantiation) at dirs (m, 3)"""
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError(f"dirs must be (m, 3), got {dirs.shape}")
    a, b = np.empty(dirs.shape[0], dtype=np.float32), np.empty(dirs.shape[0], dtype=np.float32)
    _check(lib().rt_selftest_sky_pdf_forms(scene._h, _p(dirs, C.c_float), C.c_uint64(dirs.shape[0]), _p(a, C.c_float), _p(b, C.c_float)))
    return a, b


SKY_CELL_COUNT_NAMES = ("guarded_disagree", "unguarded", "unguarded_agree", "pdf_mismatches", "tested")


def sky_cell_guard(scene):
    """the guard of the carried sky cell for this scene's sky, as rt_selftest_sky_cell reports it without a launch (any scene, a sky
    without sampler included): {"proven", "enabled", "delta_u", "delta_v", "row_lo", "row_hi", "in_use"}"""
    guard = np.zeros(8, dtype=np.uint32)
    _check(lib().rt_selftest_sky_cell(scene._h, None, C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), None, None, _p(guard, C.c_uint32)))
    return _sky_cell_guard_dict(guard)


def _sky_cell_guard_dict(guard):
    return {"proven": bool(guard[0]), "enabled": bool(guard[1]), "delta_u": float(guard[2:3].view(np.float32)[0]), "delta_v": float(guard[3:4].view(np.float32)[0]),
            "row_lo": int(guard[4]), "row_hi": int(guard[5]), "in_use": bool(guard[6])}


def selftest_sky_cell(scene, cases=None, *, axis=0, su=0, sv=0):
    """rt_selftest_sky_cell on the scene's sky table.  cases (n, 4) uint32 (su, sv, bits of r_u, bits of r_v; consecutive cases are
    consecutive lanes of a wave): (out (n, 4) uint32 -- bits of the carried pdf, bits of the default pdf, carried cell | guard bit << 31,
    default cell --, counts, guard).  cases None: the enumeration of all 2^24 jitters of `axis` at cell (su, sv): (None, counts, guard).
    counts: {"guarded_disagree", "unguarded", "unguarded_agree", "pdf_mismatches", "tested"}; guard: {"proven", "enabled", "delta_u",
    "delta_v", "row_lo", "row_hi", "in_use"}."""
    counts, guard = (C.c_uint64 * 5)(), np.zeros(8, dtype=np.uint32)
    out = None
    if cases is not None:
        cases = np.ascontiguousarray(cases, dtype=np.uint32)
        if cases.ndim != 2 or cases.shape[1] != 4:
            raise ValueError(f"cases must be (n, 4), got {cases.shape}")
        out = np.zeros((cases.shape[0], 4), dtype=np.uint32)
        _check(lib().rt_selftest_sky_cell(scene._h, _p(cases, C.c_uint32), C.c_uint64(cases.shape[0]), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0),
                                          _p(out, C.c_uint32), counts, _p(guard, C.c_uint32)))
    else:
        _check(lib().rt_selftest_sky_cell(scene._h, None, C.c_uint64(0), C.c_uint32(axis), C.c_uint32(su), C.c_uint32(sv), None, counts, _p(guard, C.c_uint32)))
    return out, dict(zip(SKY_CELL_COUNT_NAMES, (int(x) for x in counts))), _sky_cell_guard_dict(guard)


def selftest_frame_forms(vectors, device=0):
    """rt_selftest_frame_forms: vectors (n, 3) f32, each both as a normal -- the scatter frame as the two-sphere kernels form it next
    to the plain coord_from_z -- and as a ray direction -- ray_new<FeatPair>'s direction and reciprocals next to the plain operators --
    on the GPU: {"tested", "frame_mismatches", "frame_short", "frame_plain", "ray_mismatches", "ray_short", "ray_plain"} (short / plain:
    vectors that passed / failed the site's guard) and "in_use": names of the short forms the kernels' switches select.  Both
    mismatch counts must be zero."""
    return _selftest_cases("frame_forms", vectors, device)


def philox_round_keys(seed):
    """rt_philox_round_keys: (10, 2) uint32, row r = the key words round r of rt_philox4x32_10 xors in for `seed` (host only)"""
    keys = np.zeros((10, 2), dtype=np.uint32)
    lib().rt_philox_round_keys.restype = None
    lib().rt_philox_round_keys(C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), _p(keys, C.c_uint32))
    return keys


def selftest_gen_keys(seed, cases, device=0):
    """rt_selftest_gen_keys: cases (n, 4) uint32 -- pixel index, sample index, sample_begin low word, high word -- seeded on the GPU
    from the host's key table of `seed`, without and with the pixel's product formed ahead, next to rt_rng_seed: {"tested",
    "state_mismatches", "draw_mismatches", "item_state_mismatches", "item_draw_mismatches", "zero_blocks"} and "in_use": names of
    the forms the render kernels' switches select.  The four mismatch counts must be zero."""
    return _selftest_cases("gen_keys", cases, device, C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF))


def selftest_pair_shadow(cases, device=0):
    """rt_selftest_pair_shadow: cases (n, 10) f32 -- centre, radius, ray origin, ray direction (as given) -- through the two-sphere
    kernels' occlusion predicate for a ray without a limit and through Sphere::get_int's `hit && t > 0`, on the GPU:
    {"tested", "mismatches", "asked_mismatches", "asked"}.  Both mismatch counts must be zero."""
    return _selftest_cases("pair_shadow", cases, device)


def selftest_pair_shadow_walk(cases, device=0):
    """rt_selftest_pair_shadow_walk: cases (n, 16) f32 -- first sphere (centre, radius), second sphere, ray origin, ray direction,
    skip (0 none, 1 first, 2 second), one unused -- through the two-sphere kernels' whole shadow arm and through the same arm with
    the full test of every candidate, on the GPU: {"tested", "mismatches", "asked", "asked_both", "asked_with_occluded"}."""
    return _selftest_cases("pair_shadow_walk", cases, device)


def selftest_pair_primary(scene, origin):
    """rt_selftest_pair_primary: (valid, mismatches) -- whether a render from `origin` would use the host's block of
    origin-only terms (csrc/rt_types.h DevPairPrimary), and how many of its words differ from the device's own arithmetic."""
    valid, bad = C.c_uint32(), C.c_uint64()
    _check(lib().rt_selftest_pair_primary(scene._h, _f3(origin), C.byref(valid), C.byref(bad)))
    return bool(valid.value), int(bad.value)


def selftest_sky_tiles(scene, camera, opts):
    """rt_selftest_sky_tiles: (tiles_y, tiles_x) uint8 -- 1 where a render of `camera` under `opts` would flag the tile as seeing
    only sky (csrc/rt_sky_tiles.h), by the kernels' own test on the GPU; zeros for scenes the two-sphere kernels do not take."""
    tw, th = int(opts.tile_width) or 8, int(opts.tile_height) or 8
    tiles_x, tiles_y = (int(opts.width) + tw - 1) // tw, (int(opts.height) + th - 1) // th
    out = np.zeros(tiles_x * tiles_y, dtype=np.uint8)
    _check(lib().rt_selftest_sky_tiles(scene._h, C.byref(camera), C.byref(opts), _p(out, C.c_uint8), C.c_uint64(out.size)))
    return out.reshape(tiles_y, tiles_x)


def camera_new(origin, lookat, vup, fov, aspect_ratio, aperture, focus_dist):
    """SimpleCamera::new (camera.rs:20-54)."""
    cam = abi.Camera()
    _check(lib().rt_camera_new(C.byref(cam), _f3(origin), _f3(lookat), _f3(vup), C.c_float(fov),
                               C.c_float(aspect_ratio), C.c_float(aperture), C.c_float(focus_dist)))
    return cam


def lens_camera_new(origin, lookat, vup, fov, aspect_ratio, aperture, focus_dist, projection="perspective"):
    """rt_lens_camera_new: SimpleCamera::new with the fields get_ray never reads (u, v, lens_radius) kept, -w, the fisheye's
    half angle (fov / 2, radians) and a projection: a name of abi.PROJECTIONS or an rt_projection value."""
    if isinstance(projection, str):
        _known(projection, abi.PROJECTIONS, "projection")
        projection = abi.PROJECTIONS[projection]
    cam = abi.LensCamera()
    _check(lib().rt_lens_camera_new(C.byref(cam), _f3(origin), _f3(lookat), _f3(vup), C.c_float(fov), C.c_float(aspect_ratio),
                                    C.c_float(aperture), C.c_float(focus_dist), C.c_int32(projection)))
    return cam


HIT_DTYPE = np.dtype([("t", "<f4"), ("point", "<f4", 3), ("error", "<f4", 3), ("normal", "<f4", 3), ("uv", "<f4", 2),
                      ("has_uv", "<i4"), ("out", "<i4"), ("material", "<u4"), ("found", "<u4"), ("index", "<u8")])
NODE_DTYPE = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("children", "<i8", 2), ("primitive_offset", "<u8"),
                       ("number_primitives", "<u8")])


WIDE_NODE_DTYPE = np.dtype([("origin", "<f4", 3), ("exps", "<u4"), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("child", "<u4", 4),
                            ("pad", "<u4", 2)])


def _pack_rays(origins, directions):
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


class HipScene:
    """Bvh::new(primitives, sky, split_type) + upload to the HBM of `device`
    (device=abi.RT_DEVICE_NONE: the host-side tree only; rendering then raises RT_ERR_NO_DEVICE)."""

    def __init__(self, scene_description, device=0, devices=None):
        """devices=[d0, d1, ...]: ONE scene replicated over several GPUs (rt_scene_create_multi): every render call shards the
        frame's tiles over them and gathers into d0's HBM."""
        self._desc = scene_description.desc()
        self._h = C.c_void_p()
        if devices is not None:
            devices = [int(d) for d in devices]
            self.device = devices[0]
            self.devices = devices
            arr = (C.c_int * len(devices))(*devices)
            _check(lib().rt_scene_create_multi(C.byref(self._desc), arr, C.c_uint32(len(devices)), C.byref(self._h)))
        else:
            self.device = device
            self.devices = [device]
            _check(lib().rt_scene_create(C.byref(self._desc), C.c_int(device), C.byref(self._h)))

    def device_count(self):
        n = C.c_uint32()
        _check(lib().rt_scene_device_count(self._h, C.byref(n)))
        return n.value

    def close(self):
        if self._h:
            lib().rt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- what Bvh::new produced ----
    def counts(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().rt_scene_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def nodes(self):
        n = self.counts()[0]
        out = np.zeros(max(1, n), dtype=NODE_DTYPE)
        _check(lib().rt_scene_get_nodes(self._h, out.ctypes.data_as(C.POINTER(abi.BvhNode)), C.c_uint64(n)))
        return out[:n]

    def primitive_order(self):
        n = self.counts()[1]
        out = np.zeros(max(1, n), dtype=np.uint64)
        _check(lib().rt_scene_get_primitive_order(self._h, _p(out, C.c_uint64), C.c_uint64(n)))
        return out[:n]

    def lights(self):
        n = self.counts()[2]
        out = np.zeros(max(1, n), dtype=np.uint64)
        _check(lib().rt_scene_get_lights(self._h, _p(out, C.c_uint64), C.c_uint64(n)))
        return out[:n]

    def wide_tree(self):
        """(wide nodes as a structured array, root ref, stack depth, leaf boxes [n_slots, 8]) -- what pruned walks descend"""
        n, root, depth = C.c_uint64(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_scene_wide_info(self._h, C.byref(n), C.byref(root), C.byref(depth)))
        nodes = np.zeros(max(1, n.value), dtype=WIDE_NODE_DTYPE)
        boxes = np.zeros((max(1, self.counts()[1]), 8), dtype=np.float32)
        if n.value:
            _check(lib().rt_scene_get_wide_nodes(self._h, nodes.ctypes.data_as(C.c_void_p), C.c_uint64(n.value)))
            _check(lib().rt_scene_get_leaf_boxes(self._h, _p(boxes, C.c_float), C.c_uint64(boxes.shape[0])))
        return nodes[:n.value], root.value, depth.value, boxes

    def wide_tree_compact(self):
        """(compact wide nodes -- the bytes the kernels fetch --, leaf boxes by leaf index [n_leaves, 8])"""
        n, root, depth = C.c_uint64(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_scene_wide_info(self._h, C.byref(n), C.byref(root), C.byref(depth)))
        nodes = np.zeros(max(1, n.value), dtype=WIDE_NODE_DTYPE)
        n_leaves = C.c_uint64()
        _check(lib().rt_scene_get_leaf_boxes_compact(self._h, None, C.c_uint64(0), C.byref(n_leaves)))
        boxes = np.zeros((max(1, n_leaves.value), 8), dtype=np.float32)
        if n.value:
            _check(lib().rt_scene_get_wide_nodes_compact(self._h, nodes.ctypes.data_as(C.c_void_p), C.c_uint64(n.value)))
            _check(lib().rt_scene_get_leaf_boxes_compact(self._h, _p(boxes, C.c_float), C.c_uint64(boxes.shape[0]), C.byref(n_leaves)))
        return nodes[:n.value], boxes[:n_leaves.value]

    def sky_info(self):
        """rt_scene_sky_info as a dict: res_x, res_y, guide_k, inv_res_ok, the two reciprocals (f32) and table_bytes"""
        si = abi.SkyInfo()
        _check(lib().rt_scene_sky_info(self._h, C.byref(si)))
        d = {name: getattr(si, name) for name, _ in abi.SkyInfo._fields_}
        d["inv_res_x"], d["inv_res_y"] = np.float32(si.inv_res_x), np.float32(si.inv_res_y)
        return d

    def sky_tables(self):
        """(row CDFs [res_y, res_x + 1], marginal CDF [res_y + 1], guide bytes [res_y + 1, guide_k] or None) as the host built them"""
        si = self.sky_info()
        rows = np.zeros((si["res_y"], si["res_x"] + 1), dtype=np.float32)
        marg = np.zeros(si["res_y"] + 1, dtype=np.float32)
        guide = np.zeros((si["res_y"] + 1, si["guide_k"]), dtype=np.uint8) if si["guide_k"] else None
        _check(lib().rt_scene_get_sky_tables(self._h, _p(rows, C.c_float), C.c_uint64(rows.size), _p(marg, C.c_float), C.c_uint64(marg.size),
                                             _p(guide, C.c_uint8), C.c_uint64(0 if guide is None else guide.size)))
        return rows, marg, guide

    def selftest_sky(self, tables_in_lds, n, seed=1, dirs=None):
        """rt_selftest_sky: (directions [n, 3] of sky_sample on streams 0..n-1 of `seed`, sky_pdf at each of them [n], sky_pdf at
        each row of `dirs` [m]) computed by the kernels' own sky code, with the tables in global memory (0) or staged in LDS (1)"""
        dirs = np.zeros((0, 3), np.float32) if dirs is None else np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        m = dirs.shape[0]
        out_dirs = np.zeros((max(1, n), 3), dtype=np.float32)
        out_pdf_s = np.zeros(max(1, n), dtype=np.float32)
        out_pdf = np.zeros(max(1, m), dtype=np.float32)
        _check(lib().rt_selftest_sky(self._h, C.c_int(int(tables_in_lds)), C.c_uint64(seed), C.c_uint64(n), _p(out_dirs, C.c_float),
                                     _p(out_pdf_s, C.c_float), _p(dirs, C.c_float) if m else None, C.c_uint64(m), _p(out_pdf, C.c_float)))
        return out_dirs[:n], out_pdf_s[:n], out_pdf[:m]

    def set_traversal(self, mode):
        """-1 auto, 0 exhaustive (reference amount of work), 1 pruned."""
        _check(lib().rt_scene_set_traversal(self._h, C.c_int(mode)))

    def set_tuning(self, key, value):
        """abi.RT_TUNE_*: knobs that change how the kernels run, never what they return."""
        _check(lib().rt_scene_set_tuning(self._h, C.c_int(key), C.c_int(value)))

    # ---- Sampler::sample_image: mean over opts.samples_per_pixel passes ----
    def render(self, camera, opts):
        out = np.zeros(output_floats(opts), dtype=np.float32)
        rays = C.c_uint64()
        _check(lib().rt_render(self._h, C.byref(camera), C.byref(opts), _p(out, C.c_float), C.byref(rays)))
        if opts.output_layout == abi.RT_LAYOUT_FRAME:
            out = out.reshape(opts.height, opts.width, 3)
        else:
            out = out.reshape(-1, 3)
        return out, rays.value

    def render_rgb8(self, camera, opts, gamma=2.2):
        """rt_render + the output stage on the device: the 8-bit image save_data_to_image would write (lib.rs:89-97)."""
        out = np.zeros(output_floats(opts), dtype=np.uint8)
        rays = C.c_uint64()
        _check(lib().rt_render_rgb8(self._h, C.byref(camera), C.byref(opts), C.c_float(gamma), _p(out, C.c_uint8), C.byref(rays)))
        return (out.reshape(opts.height, opts.width, 3) if opts.output_layout == abi.RT_LAYOUT_FRAME else out.reshape(-1, 3)), rays.value

    def output_rgb8_device(self, d_rgb_ptr, n_values, d_out_ptr, gamma=2.2, stream=0):
        _check(lib().rt_output_rgb8_device(self._h, C.c_void_p(d_rgb_ptr), C.c_uint64(n_values), C.c_float(gamma), C.c_void_p(d_out_ptr),
                                           C.c_void_p(stream)))

    def render_device(self, camera, opts, d_out_ptr, d_rays_ptr=None, stream=0):
        """Asynchronous render into device memory (raw pointers, e.g. torch.Tensor.data_ptr())."""
        _check(lib().rt_render_device(self._h, C.byref(camera), C.byref(opts), C.c_void_p(d_out_ptr), _vp(d_rays_ptr), C.c_void_p(stream)))

    def gather_info(self):
        """(rt_gather_mode, why): how a multi-device scene moves its members' shards into devices[0] (rt_scene_gather_info)"""
        mode, note = C.c_int(), C.create_string_buffer(512)
        _check(lib().rt_scene_gather_info(self._h, C.byref(mode), note, C.c_uint64(512)))
        return mode.value, note.value.decode()

    def auto_sample_split(self, opts):
        """what opts.sample_split = 0 resolves to on this scene (rt_scene_auto_sample_split: the library's one rule)"""
        v = C.c_uint32()
        _check(lib().rt_scene_auto_sample_split(self._h, C.byref(opts), C.byref(v)))
        return v.value

    def last_kernel_ms(self):
        ms, n = C.c_float(), C.c_uint32()
        _check(lib().rt_last_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_launch_info(self):
        """What the most recent render launched (rt_launch_info) as a dict."""
        li = abi.LaunchInfo()
        _check(lib().rt_last_launch_info(self._h, C.byref(li)))
        d = {name: getattr(li, name) for name, _ in abi.LaunchInfo._fields_ if name not in ("kernel", "reserved")}
        d["kernel"] = li.kernel.decode()
        return d

    # ---- first-hit AOV buffers (rt_render_aov): albedo, normal, depth, coverage, primitive / material IDs ----
    def render_aov(self, camera, opts, channels=abi.AOV_CHANNELS):
        """The auxiliary buffers of the primary hits of passes [sample_begin, sample_begin + samples_per_pixel) -- the camera rays
        rt_render traces -- as {channel: numpy array}: albedo / normal (H, W, 3) f32, depth / coverage (H, W) f32, primitive /
        material (H, W) u32 (abi.AOV_NO_ID where pass sample_begin missed).  Semantics: include/rt_hip.h rt_aov_buffers."""
        bufs = abi.AovBuffers()
        out = _host_buffers(abi.AOV_SHAPES, bufs, channels, int(opts.height), int(opts.width))
        _check(lib().rt_render_aov(self._h, C.byref(camera), C.byref(opts), C.byref(bufs)))
        return out

    def render_aov_device(self, camera, opts, d_ptrs, stream=0):
        """rt_render_aov_device: asynchronous, into DEVICE buffers of the scene's GPU.  d_ptrs = {channel: device pointer}
        (e.g. torch.Tensor.data_ptr()); channels left out are not produced."""
        bufs = _device_buffers(abi.AOV_SHAPES, abi.AovBuffers(), d_ptrs)
        _check(lib().rt_render_aov_device(self._h, C.byref(camera), C.byref(opts), C.byref(bufs), C.c_void_p(stream)))

    # ---- specular-chain AOV buffers (rt_render_aov_chain): the same channels seen through perfect mirrors and glass ----
    def render_aov_chain(self, camera, opts, channels=abi.AOV_CHAIN_CHANNELS, max_chain=8, fuzz_limit=0.0):
        """The channels of render_aov taken at the first vertex of each camera path that is not a followed Reflect / Refract
        surface, plus "bounces" (H, W) f32, the mean number of surfaces followed; as {channel: numpy array}.  albedo / normal /
        depth are drop-in guides for denoise and upscale (not for denoise_temporal: the depth is a path length).  Semantics:
        include/rt_hip.h rt_aov_chain_opts."""
        bufs = abi.AovChainBuffers()
        out = _host_buffers(abi.AOV_CHAIN_SHAPES, bufs, channels, int(opts.height), int(opts.width))
        copts = abi.default_aov_chain_opts(max_chain, fuzz_limit)
        _check(lib().rt_render_aov_chain(self._h, C.byref(camera), C.byref(opts), C.byref(copts), C.byref(bufs)))
        return out

    def render_aov_chain_device(self, camera, opts, d_ptrs, stream=0, max_chain=8, fuzz_limit=0.0):
        """rt_render_aov_chain_device: asynchronous, into DEVICE buffers of the scene's GPU.  d_ptrs = {channel: device pointer}
        over abi.AOV_CHAIN_CHANNELS; channels left out are not produced.  Allocates nothing: capturable from the first call."""
        bufs = _device_buffers(abi.AOV_CHAIN_SHAPES, abi.AovChainBuffers(), d_ptrs)
        copts = abi.default_aov_chain_opts(max_chain, fuzz_limit)
        _check(lib().rt_render_aov_chain_device(self._h, C.byref(camera), C.byref(opts), C.byref(copts), C.byref(bufs),
                                                C.c_void_p(stream)))

    # ---- anti-aliased ID mattes (rt_render_matte, rt_matte_extract): ranked ID / coverage layers over all passes ----
    def render_matte(self, camera, opts, id_kind="material", layers=4, residual=False):
        """The `layers` most-covering primitive or material IDs of every pixel over passes [sample_begin, sample_begin +
        samples_per_pixel) with their coverage fractions, as {"ids": (K, H, W) u32, "coverage": (K, H, W) f32} plus "residual"
        (H, W) f32 -- the share the layers leave out -- when asked for.  A sky layer has ID abi.AOV_NO_ID and a positive coverage,
        an empty layer the same ID and coverage 0.  id_kind: "material" / "primitive" or abi.RT_MATTE_ID_*.  Semantics:
        include/rt_hip.h rt_matte_opts."""
        m = matte_opts(id_kind=id_kind, layers=layers)
        bufs = abi.MatteBuffers()
        k = max(0, min(int(layers), abi.RT_MATTE_SLOTS))  # enough to allocate; a layer count out of range is the library's to refuse
        out = _host_buffers(abi.MATTE_SHAPES, bufs, abi.MATTE_BUFFERS if residual else ("ids", "coverage"), int(opts.height), int(opts.width), k)
        _check(lib().rt_render_matte(self._h, C.byref(camera), C.byref(opts), C.byref(m), C.byref(bufs)))
        return out

    def render_matte_device(self, camera, opts, d_ptrs, id_kind="material", layers=4, stream=0):
        """rt_render_matte_device: asynchronous, into DEVICE buffers of the scene's GPU.  d_ptrs = {"ids": ..., "coverage": ...,
        "residual": ...} device pointers (the residual may be left out).  Allocates nothing: capturable from the first call."""
        bufs = _device_buffers(abi.MATTE_SHAPES, abi.MatteBuffers(), d_ptrs)
        m = matte_opts(id_kind=id_kind, layers=layers)
        _check(lib().rt_render_matte_device(self._h, C.byref(camera), C.byref(opts), C.byref(m), C.byref(bufs), C.c_void_p(stream)))

    def matte_extract(self, ids, coverage, selection):
        """rt_matte_extract: the (H, W) f32 matte of the IDs in `selection` (any order, duplicates allowed; abi.AOV_NO_ID selects
        the sky) from the (K, H, W) layers render_matte returns -- which may also come as that dict, in place of `ids` with
        coverage=None."""
        if isinstance(ids, dict):
            ids, coverage = ids["ids"], ids["coverage"]
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        coverage = np.ascontiguousarray(coverage, dtype=np.float32)
        if ids.ndim != 3 or coverage.shape != ids.shape:
            raise ValueError(f"ids and coverage must both be (K, H, W), got {ids.shape} and {coverage.shape}")
        k, h, w = ids.shape
        sel = np.ascontiguousarray(np.asarray(selection, dtype=np.uint32).reshape(-1))
        bufs = abi.MatteBuffers()
        bufs.ids, bufs.coverage = _p(ids, C.c_uint32), _p(coverage, C.c_float)
        out = np.zeros((h, w), dtype=np.float32)
        _check(lib().rt_matte_extract(self._h, C.byref(bufs), C.c_uint32(w), C.c_uint32(h), C.c_uint32(k),
                                      _p(sel, C.c_uint32) if sel.size else None, C.c_uint64(sel.size), _p(out, C.c_float)))
        return out

    def matte_extract_device(self, d_ids, d_coverage, width, height, layers, d_sorted_ids, n_ids, d_out, stream=0):
        """rt_matte_extract_device: asynchronous, DEVICE buffers of the scene's GPU, no state.  d_sorted_ids: n_ids u32 in ASCENDING
        order (not verified; 0 / None with n_ids = 0)."""
        bufs = _device_buffers(abi.MATTE_SHAPES, abi.MatteBuffers(), {"ids": d_ids, "coverage": d_coverage})
        _check(lib().rt_matte_extract_device(self._h, C.byref(bufs), C.c_uint32(width), C.c_uint32(height), C.c_uint32(layers),
                                             _dp(d_sorted_ids, C.c_uint32), C.c_uint64(n_ids), _dp(d_out), C.c_void_p(stream)))

    # ---- ambient occlusion (rt_render_ao): visibility and bent normal at the first hit ----
    def render_ao(self, camera, opts, rays_per_pass=4, radius=0.0, channels=abi.AO_CHANNELS):
        """The share of `rays_per_pass` cosine-weighted rays per pass from the first hit that reach nothing within `radius` (0: no
        limit) and the mean direction of those rays, over passes [sample_begin, sample_begin + samples_per_pixel), as
        {"visibility": (H, W) f32, "bent_normal": (H, W, 3) f32}; only `channels` are produced.  A pixel no pass hit has visibility
        1 and bent normal 0.  Semantics: include/rt_hip.h rt_ao_opts."""
        a = ao_opts(rays_per_pass=rays_per_pass, radius=radius)
        bufs = abi.AoBuffers()
        out = _host_buffers(abi.AO_SHAPES, bufs, channels, int(opts.height), int(opts.width))
        _check(lib().rt_render_ao(self._h, C.byref(camera), C.byref(opts), C.byref(a), C.byref(bufs)))
        return out

    def render_ao_device(self, camera, opts, d_ptrs, rays_per_pass=4, radius=0.0, stream=0):
        """rt_render_ao_device: asynchronous, into DEVICE buffers of the scene's GPU.  d_ptrs = {"visibility": ..., "bent_normal":
        ...} device pointers (either may be left out).  Allocates nothing: capturable from the first call."""
        bufs = _device_buffers(abi.AO_SHAPES, abi.AoBuffers(), d_ptrs)
        a = ao_opts(rays_per_pass=rays_per_pass, radius=radius)
        _check(lib().rt_render_ao_device(self._h, C.byref(camera), C.byref(opts), C.byref(a), C.byref(bufs), C.c_void_p(stream)))

    # ---- AOV-guided A-Trous denoiser (rt_denoise) ----
    def denoise(self, color, albedo=None, normal=None, depth=None, variance=None, **opts):
        """rt_denoise: filter an (H, W, 3) f32 radiance image guided by the optional albedo / normal (H, W, 3), depth and variance
        (H, W); returns (H, W, 3) f32.  The guides may also come as the dict render_aov returns, in place of `albedo` (its
        other channels are ignored), or with the image under "color" in place of `color`.  Keyword options: iterations,
        sigma_luminance, sigma_normal, sigma_depth.  Semantics: include/rt_hip.h rt_denoise_opts."""
        color, guides = _guides(color, albedo, normal=normal, depth=depth, variance=variance)
        color, h, w = _image(color, "color")
        ins = abi.DenoiseInputs()
        _host_inputs(abi.DENOISE_SHAPES, ins, {"color": color, **guides}, h, w)
        o = denoise_opts(w, h, **opts)
        out = np.zeros((h, w, 3), dtype=np.float32)
        _check(lib().rt_denoise(self._h, C.byref(ins), C.byref(o), _p(out, C.c_float)))
        return out

    def denoise_device(self, d_ptrs, d_workspace, d_out, opts, stream=0):
        """rt_denoise_device: asynchronous, DEVICE buffers of the scene's GPU.  d_ptrs = {input: device pointer} over
        abi.DENOISE_INPUTS ("color" required); d_workspace: denoise_workspace_bytes(opts) bytes, 16-byte aligned;
        opts: abi.DenoiseOpts with the frame size set."""
        ins = _device_buffers(abi.DENOISE_SHAPES, abi.DenoiseInputs(), d_ptrs)
        _check(lib().rt_denoise_device(self._h, C.byref(ins), C.byref(opts), C.c_void_p(int(d_workspace)),
                                       _dp(d_out), C.c_void_p(stream)))

    def render_denoised(self, camera, opts, dopts=None):
        """rt_render_denoised: two half renders, the AOVs of all passes and the filter in one call.  Returns (clean, noisy,
        rays_shot) with clean / noisy (H, W, 3) f32.  dopts: abi.DenoiseOpts (its width / height are ignored) or None for the
        defaults."""
        h, w = int(opts.height), int(opts.width)
        if dopts is None:
            dopts = denoise_opts(w, h)
        return self._frames_and_rays("rt_render_denoised", (C.byref(camera), C.byref(opts), C.byref(dopts)), (h, w, 3), (h, w, 3))

    def _frames_and_rays(self, symbol, args, *shapes):
        """a composite call symbol(scene, args..., one zeroed f32 frame per shape..., rays_shot *): (the frames..., rays_shot)"""
        frames = [np.zeros(shape, dtype=np.float32) for shape in shapes]
        rays = C.c_uint64()
        _check(getattr(lib(), symbol)(self._h, *args, *(_p(a, C.c_float) for a in frames), C.byref(rays)))
        return (*frames, rays.value)

    # ---- noise estimates (rt_render_noise, rt_noise_tiles, rt_render_converged, rt_render_denoised_split) ----
    def render_noise(self, camera, opts, albedo=None, channels=abi.NOISE_CHANNELS, **nopts):
        """rt_render_noise: ONE render at opts.sample_split (2..64 dividing the passes; 0 = automatic) and, from its chunk sums,
        {"mean": (H, W, 3), "variance": (H, W), "lum_mean": (H, W), "tile_error": (ceil(H/8), ceil(W/8)) f32, "summary": dict,
        "rays_shot": int}; only `channels` (always the mean) are produced.  albedo (H, W, 3): demodulate as rt_denoise does.
        Keyword options: luminance_floor, threshold.  Semantics: include/rt_hip.h rt_noise_opts."""
        n = noise_opts(**nopts)
        h, w = int(opts.height), int(opts.width)
        bufs = abi.NoiseBuffers()
        out = _host_buffers(abi.NOISE_SHAPES, bufs, ("mean", *channels), h, w)
        albedo = _f32(albedo, (h, w, 3), "albedo")
        rays = C.c_uint64()
        _check(lib().rt_render_noise(self._h, C.byref(camera), C.byref(opts), C.byref(n), _p(albedo, C.c_float), C.byref(bufs), C.byref(rays)))
        if "summary" in out:
            out["summary"] = _summary_dict(out["summary"])
        out["rays_shot"] = rays.value
        return out

    def render_noise_device(self, camera, opts, d_ptrs, d_albedo=None, d_rays_ptr=None, stream=0, **nopts):
        """rt_render_noise_device: asynchronous, DEVICE buffers of the scene's GPU.  d_ptrs = {channel: device pointer} over
        abi.NOISE_CHANNELS ("mean" required; "summary": 16 bytes)."""
        bufs = _device_buffers(abi.NOISE_SHAPES, abi.NoiseBuffers(), d_ptrs)
        n = noise_opts(**nopts)
        _check(lib().rt_render_noise_device(self._h, C.byref(camera), C.byref(opts), C.byref(n), _dp(d_albedo), C.byref(bufs),
                                            _vp(d_rays_ptr), C.c_void_p(stream)))

    def noise_tiles(self, lum_mean, variance, **nopts):
        """rt_noise_tiles: the tile stage alone on (H, W) f32 planes; returns (tile_error (ceil(H/8), ceil(W/8)), summary dict)."""
        lum_mean = np.ascontiguousarray(lum_mean, dtype=np.float32)
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        if lum_mean.ndim != 2 or lum_mean.shape != variance.shape:
            raise ValueError(f"lum_mean and variance must be (H, W) alike, got {lum_mean.shape} and {variance.shape}")
        h, w = lum_mean.shape
        n = noise_opts(**nopts)
        tiles = np.zeros(_shape("tiles", h, w), dtype=np.float32)
        summary = abi.NoiseSummary()
        _check(lib().rt_noise_tiles(self._h, _p(lum_mean, C.c_float), _p(variance, C.c_float), C.c_uint32(w), C.c_uint32(h), C.byref(n),
                                    _p(tiles, C.c_float), C.byref(summary)))
        return tiles, _summary_dict(summary)

    def noise_tiles_device(self, d_lum_mean, d_variance, width, height, d_tile_error=None, d_summary=None, stream=0, **nopts):
        """rt_noise_tiles_device: asynchronous, DEVICE planes; allocates nothing."""
        n = noise_opts(**nopts)
        _check(lib().rt_noise_tiles_device(self._h, _dp(d_lum_mean), _dp(d_variance), C.c_uint32(width), C.c_uint32(height), C.byref(n),
                                           _dp(d_tile_error), _dp(d_summary, abi.NoiseSummary), C.c_void_p(stream)))

    def render_converged(self, camera, opts, batch, min_batches=1, max_passes=None, **nopts):
        """rt_render_converged: render windows of `batch` passes from opts.sample_begin on until every tile's error is at most the
        threshold (after at least min_batches windows) or another window would exceed max_passes (default: 64 windows).  Returns
        {"mean", "variance", "tile_error", "passes", "batches", "converged", "rays_shot", "summary"}; the mean is a mean of batch
        means, not the bytes of one render of all the passes."""
        n = noise_opts(**nopts)
        h, w = int(opts.height), int(opts.width)
        bufs = abi.NoiseBuffers()
        out = _host_buffers(abi.NOISE_SHAPES, bufs, ("mean", "variance", "tile_error"), h, w)
        res = abi.NoiseResult()
        _check(lib().rt_render_converged(self._h, C.byref(camera), C.byref(opts), C.byref(n), C.c_uint64(batch), C.c_uint32(min_batches),
                                         C.c_uint64(64 * batch if max_passes is None else max_passes), bufs.mean, bufs.variance,
                                         bufs.tile_error, C.byref(res)))
        out.update(passes=res.passes, batches=res.batches, converged=bool(res.converged), rays_shot=res.rays_shot,
                   summary=_summary_dict(res.summary))
        return out

    def render_denoised_split(self, camera, opts, dopts=None):
        """rt_render_denoised_split: render_denoised from ONE render at opts.sample_split, the variance taken from its chunk sums.
        Returns (clean, noisy, variance, rays_shot); noisy is the bytes render() gives at that split."""
        h, w = int(opts.height), int(opts.width)
        if dopts is None:
            dopts = denoise_opts(w, h)
        return self._frames_and_rays("rt_render_denoised_split", (C.byref(camera), C.byref(opts), C.byref(dopts)), (h, w, 3), (h, w, 3), (h, w))

    # ---- the render on a list of tiles, and the list of the noisy ones (rt_render_tiles, rt_noise_select_tiles) ----
    def render_tiles(self, camera, opts, tiles, frame, chunk_sums=False):
        """rt_render_tiles: the pixels of the listed 8 x 8 tiles (indices into the grid of noise_tiles, distinct) of `frame`
        ((H, W, 3) f32, contiguous, changed in place) receive the bytes render() gives them under the same opts; every other
        pixel keeps its value.  Returns (rays_shot, sums): sums is None, or with chunk_sums=True and a resolved split S > 1 the
        (S, len(tiles), 8, 8, 3) chunk sums, padding lanes of edge tiles +0."""
        h, w = int(opts.height), int(opts.width)
        if not (isinstance(frame, np.ndarray) and frame.dtype == np.float32 and frame.shape == (h, w, 3) and frame.flags.c_contiguous):
            raise ValueError(f"frame must be a contiguous float32 array of shape {(h, w, 3)}")
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32).reshape(-1)
        sums = None
        if chunk_sums:
            split = int(opts.sample_split) or self.auto_sample_split(opts)
            if split > 1:
                sums = np.zeros((split, len(tiles), 8, 8, 3), dtype=np.float32)
        rays = C.c_uint64()
        _check(lib().rt_render_tiles(self._h, C.byref(camera), C.byref(opts), _p(tiles, C.c_uint32) if len(tiles) else None,
                                     C.c_uint32(len(tiles)), _p(frame, C.c_float), _p(sums, C.c_float), C.byref(rays)))
        return rays.value, sums

    def render_adaptive(self, camera, opts, batch, min_batches=1, max_passes=None, albedo=None, **nopts):
        """rt_render_adaptive: render_converged that renders, after min_batches whole-frame windows, only the tiles whose error is
        still above the threshold.  Returns {"mean", "variance", "tile_error", "passes" ((H, W) uint32: passes rendered per pixel),
        "batches", "converged", "pixel_passes", "rays_shot", "summary"}.  The mean of a stopped tile is a mean of fewer batches
        than its neighbour's: tile borders can show at loose thresholds."""
        n = noise_opts(**nopts)
        h, w = int(opts.height), int(opts.width)
        bufs = abi.NoiseBuffers()
        out = _host_buffers(abi.NOISE_SHAPES, bufs, ("mean", "variance", "tile_error"), h, w)
        passes = np.zeros((h, w), dtype=np.uint32)
        albedo = _f32(albedo, (h, w, 3), "albedo")
        res = abi.AdaptiveResult()
        _check(lib().rt_render_adaptive(self._h, C.byref(camera), C.byref(opts), C.byref(n), _p(albedo, C.c_float), C.c_uint64(batch),
                                        C.c_uint32(min_batches), C.c_uint64(64 * batch if max_passes is None else max_passes),
                                        bufs.mean, bufs.variance, bufs.tile_error, _p(passes, C.c_uint32), C.byref(res)))
        out.update(passes=passes, batches=res.batches, converged=bool(res.converged), pixel_passes=res.pixel_passes,
                   rays_shot=res.rays_shot, summary=_summary_dict(res.summary))
        return out

    def render_tiles_device(self, camera, opts, d_tiles, n_tiles, d_frame, d_chunk_sums=None, d_rays_ptr=None, stream=0):
        """rt_render_tiles_device: asynchronous, DEVICE buffers of the scene's GPU; allocates nothing, keeps no state."""
        _check(lib().rt_render_tiles_device(self._h, C.byref(camera), C.byref(opts), _dp(d_tiles, C.c_uint32), C.c_uint32(n_tiles),
                                            _dp(d_frame), _dp(d_chunk_sums), _vp(d_rays_ptr), C.c_void_p(stream)))

    # ---- lens cameras (rt_render_lens): whole frames through a thin lens, a fisheye, a panorama or an orthographic camera ----
    def render_lens(self, camera, opts, chunk_sums=False):
        """rt_render_lens: the frame of an abi.LensCamera (lens_camera_new) under `opts`.  Returns (frame (H, W, 3) f32, rays_shot,
        sums): sums is None, or with chunk_sums=True and a resolved split S > 1 the (S, ceil(H/8) * ceil(W/8), 8, 8, 3) chunk
        sums, padding lanes of edge tiles +0.  A perspective frame at aperture 0 is NOT render()'s bytes: the camera draws on a
        stream of its own."""
        h, w = int(opts.height), int(opts.width)
        frame = np.zeros((h, w, 3), dtype=np.float32)
        sums = None
        if chunk_sums:
            split = int(opts.sample_split) or self.auto_sample_split(opts)
            if split > 1:
                sums = np.zeros((split, ((h + 7) // 8) * ((w + 7) // 8), 8, 8, 3), dtype=np.float32)
        rays = C.c_uint64()
        _check(lib().rt_render_lens(self._h, C.byref(camera), C.byref(opts), _p(frame, C.c_float), _p(sums, C.c_float), C.byref(rays)))
        return frame, rays.value, sums

    def render_lens_device(self, camera, opts, d_frame, d_chunk_sums=None, d_rays_ptr=None, stream=0):
        """rt_render_lens_device: asynchronous, DEVICE buffers of the scene's GPU; allocates nothing, keeps no state."""
        _check(lib().rt_render_lens_device(self._h, C.byref(camera), C.byref(opts), _dp(d_frame), _dp(d_chunk_sums), _vp(d_rays_ptr),
                                           C.c_void_p(stream)))

    # ---- light probes (rt_probe_sh): L2 spherical-harmonic radiance at positions, projected on the device ----
    def probe_sh(self, positions, **opts):
        """rt_probe_sh: the 9 x RGB spherical-harmonic coefficients of the radiance arriving at each of the (n, 3) `positions`, under
        probe_opts(**opts).  Returns (coeffs (n, 9, 3) f32, rays_shot).  convolve=1: irradiance coefficients."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        n = pos.shape[0]
        out = np.zeros((n, 9, 3), dtype=np.float32)
        rays = C.c_uint64()
        _check(lib().rt_probe_sh(self._h, _p(pos, C.c_float), C.c_uint64(n), C.byref(probe_opts(**opts)), _p(out, C.c_float), C.byref(rays)))
        return out, rays.value

    def probe_sh_device(self, d_positions, n_probes, d_out, d_workspace, d_rays_ptr=None, stream=0, **opts):
        """rt_probe_sh_device: asynchronous, DEVICE buffers of the scene's GPU -- d_positions 3 n f32, d_out 27 n f32, d_workspace
        probe_workspace_bytes(n, **opts) bytes; allocates nothing, keeps no state."""
        _check(lib().rt_probe_sh_device(self._h, _dp(d_positions), C.c_uint64(n_probes), C.byref(probe_opts(**opts)), _dp(d_out),
                                        _vp(d_workspace), _vp(d_rays_ptr), C.c_void_p(stream)))

    @staticmethod
    def probe_workspace_bytes(n_probes, **opts):
        """rt_probe_workspace_bytes (the module's probe_workspace_bytes)."""
        return probe_workspace_bytes(n_probes, **opts)

    def probe_sh_eval(self, coeffs, normals, probe_index=None):
        """rt_probe_sh_eval: the colour each of the (m, 3) `normals` sees in the (n, 9, 3) `coeffs` -- of probe probe_index[i], or of
        probe i without an index list -- as an (m, 3) f32 array."""
        co = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1, 9, 3)
        nm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        idx = None if probe_index is None else np.ascontiguousarray(probe_index, dtype=np.uint32)
        if idx is not None and idx.shape != (nm.shape[0],):
            raise ValueError(f"probe_index must be one per normal: {idx.shape} for {nm.shape[0]} normals")
        out = np.zeros((nm.shape[0], 3), dtype=np.float32)
        _check(lib().rt_probe_sh_eval(self._h, _p(co, C.c_float), C.c_uint64(co.shape[0]), _p(idx, C.c_uint32), _p(nm, C.c_float),
                                      C.c_uint64(nm.shape[0]), _p(out, C.c_float)))
        return out

    def probe_sh_eval_device(self, d_coeffs, n_probes, d_probe_index, d_normals, m, d_out, stream=0):
        """rt_probe_sh_eval_device: asynchronous, DEVICE buffers; d_probe_index 0 / None: element i reads probe i.  An index past
        the probes gives a quiet NaN in that element."""
        _check(lib().rt_probe_sh_eval_device(self._h, _dp(d_coeffs), C.c_uint64(n_probes), _dp(d_probe_index, C.c_uint32), _dp(d_normals),
                                             C.c_uint64(m), _dp(d_out), C.c_void_p(stream)))

    # ---- guides through a lens camera (rt_render_lens_aov) and the denoised lens frame (rt_render_lens_denoised) ----
    def render_lens_aov(self, camera, opts, channels=abi.AOV_CHAIN_CHANNELS, max_chain=None, fuzz_limit=0.0):
        """rt_render_lens_aov: the seven channels of render_aov_chain for the frame render_lens makes of an abi.LensCamera -- every
        pass starts with that pass's lens ray (same camera stream, same draws) -- as {channel: numpy array}.  max_chain None: no
        chain options are passed, which is the first hit (max_chain 0).  A black fisheye sample adds to no sum; a pixel whose
        first pass is black has the IDs abi.AOV_NO_ID.  Semantics: include/rt_hip.h rt_render_lens_aov."""
        bufs = abi.AovChainBuffers()
        out = _host_buffers(abi.AOV_CHAIN_SHAPES, bufs, channels, int(opts.height), int(opts.width))
        copts = None if max_chain is None else abi.default_aov_chain_opts(max_chain, fuzz_limit)
        _check(lib().rt_render_lens_aov(self._h, C.byref(camera), C.byref(opts), _ref(copts), C.byref(bufs)))
        return out

    def render_lens_aov_device(self, camera, opts, d_ptrs, stream=0, max_chain=None, fuzz_limit=0.0):
        """rt_render_lens_aov_device: asynchronous, into DEVICE buffers of the scene's GPU.  d_ptrs = {channel: device pointer} over
        abi.AOV_CHAIN_CHANNELS; channels left out are not produced.  Allocates nothing: capturable from the first call."""
        bufs = _device_buffers(abi.AOV_CHAIN_SHAPES, abi.AovChainBuffers(), d_ptrs)
        copts = None if max_chain is None else abi.default_aov_chain_opts(max_chain, fuzz_limit)
        _check(lib().rt_render_lens_aov_device(self._h, C.byref(camera), C.byref(opts), _ref(copts), C.byref(bufs), C.c_void_p(stream)))

    def render_lens_denoised(self, camera, opts, dopts=None, max_chain=None, fuzz_limit=0.0, noisy=True):
        """rt_render_lens_denoised: render_denoised for an abi.LensCamera -- two half render_lens frames, the render_lens_aov guides of
        all passes (max_chain as there) and the filter in one call.  Returns (clean, noisy, rays_shot) with clean / noisy (H, W, 3)
        f32; noisy=False: the noisy frame is not asked for and None is returned in its place."""
        h, w = int(opts.height), int(opts.width)
        if dopts is None:
            dopts = denoise_opts(w, h)
        copts = None if max_chain is None else abi.default_aov_chain_opts(max_chain, fuzz_limit)
        clean = np.zeros((h, w, 3), dtype=np.float32)
        mean = np.zeros((h, w, 3), dtype=np.float32) if noisy else None
        rays = C.c_uint64()
        _check(lib().rt_render_lens_denoised(self._h, C.byref(camera), C.byref(opts), _ref(copts), C.byref(dopts), _p(clean, C.c_float),
                                             _p(mean, C.c_float), C.byref(rays)))
        return clean, mean, rays.value

    def noise_select_tiles(self, tile_error, threshold):
        """rt_noise_select_tiles: the indices (uint32, ascending) of the tiles of a (ceil(H/8), ceil(W/8)) f32 error map whose
        error is > threshold (NaN is not)."""
        tile_error = np.ascontiguousarray(tile_error, dtype=np.float32)
        if tile_error.ndim != 2:
            raise ValueError(f"tile_error must be (tiles_y, tiles_x), got {tile_error.shape}")
        ty, tx = tile_error.shape
        tiles = np.zeros(ty * tx, dtype=np.uint32)
        count = C.c_uint32()
        _check(lib().rt_noise_select_tiles(self._h, _p(tile_error, C.c_float), C.c_uint32(8 * tx), C.c_uint32(8 * ty), C.c_float(threshold),
                                           _p(tiles, C.c_uint32), C.byref(count)))
        return tiles[:count.value].copy()

    def noise_select_tiles_device(self, d_tile_error, width, height, threshold, d_tiles, d_count, stream=0):
        """rt_noise_select_tiles_device: asynchronous, DEVICE buffers (d_tiles: capacity the tile count; d_count: one u32)."""
        _check(lib().rt_noise_select_tiles_device(self._h, _dp(d_tile_error), C.c_uint32(width), C.c_uint32(height), C.c_float(threshold),
                                                  _dp(d_tiles, C.c_uint32), _dp(d_count, C.c_uint32), C.c_void_p(stream)))

    # ---- firefly-robust frames (rt_render_robust, rt_robust_combine, rt_render_denoised_robust) ----
    def render_robust(self, camera, opts, albedo=None, channels=abi.ROBUST_CHANNELS, **ropts):
        """rt_render_robust: ONE render at opts.sample_split (2..64 dividing the passes; 0 = automatic) and the rank-trimmed mean
        of its chunk sums: {"out": (H, W, 3) f32, "mean": (H, W, 3) f32 -- the bytes render() gives at that split --, "gini":
        (H, W) f32, "trimmed", "dropped": (H, W) uint8, "rays_shot": int}; only `channels` (always "out") are produced.
        albedo (H, W, 3): rank the demodulated luminances.  Keyword options: mode (abi.RT_ROBUST_* or "trim" / "median" /
        "gini"), trim, gini_gain.  Semantics: include/rt_hip.h rt_robust_opts."""
        r = robust_opts(**ropts)
        h, w = int(opts.height), int(opts.width)
        bufs = abi.RobustBuffers()
        out = _host_buffers(abi.ROBUST_SHAPES, bufs, ("out", *channels), h, w)
        albedo = _f32(albedo, (h, w, 3), "albedo")
        rays = C.c_uint64()
        _check(lib().rt_render_robust(self._h, C.byref(camera), C.byref(opts), C.byref(r), _p(albedo, C.c_float), C.byref(bufs), C.byref(rays)))
        out["rays_shot"] = rays.value
        return out

    def render_robust_device(self, camera, opts, d_ptrs, d_albedo=None, d_rays_ptr=None, stream=0, **ropts):
        """rt_render_robust_device: asynchronous, DEVICE buffers of the scene's GPU.  d_ptrs = {channel: device pointer} over
        abi.ROBUST_CHANNELS ("out" required)."""
        r = robust_opts(**ropts)
        bufs = _device_buffers(abi.ROBUST_SHAPES, abi.RobustBuffers(), d_ptrs)
        _check(lib().rt_render_robust_device(self._h, C.byref(camera), C.byref(opts), C.byref(r), _dp(d_albedo), C.byref(bufs),
                                             _vp(d_rays_ptr), C.c_void_p(stream)))

    def robust_combine(self, chunk_sums, chunk_passes, albedo=None, channels=abi.ROBUST_CHANNELS, **ropts):
        """rt_robust_combine: the rank-trimmed mean of the caller's chunk sums (S, H, W, 3) f32, each the sum of chunk_passes
        passes.  Returns the dict of render_robust without "rays_shot"; "mean" is the plain combine."""
        sums = np.ascontiguousarray(chunk_sums, dtype=np.float32)
        if sums.ndim != 4 or sums.shape[3] != 3:
            raise ValueError(f"chunk_sums must be (S, H, W, 3), got {sums.shape}")
        split, h, w = sums.shape[:3]
        r = robust_opts(**ropts)
        bufs = abi.RobustBuffers()
        out = _host_buffers(abi.ROBUST_SHAPES, bufs, ("out", *channels), h, w)
        albedo = _f32(albedo, (h, w, 3), "albedo")
        _check(lib().rt_robust_combine(self._h, _p(sums, C.c_float), C.c_uint32(split), C.c_uint64(chunk_passes), C.c_uint32(w), C.c_uint32(h),
                                       _p(albedo, C.c_float), C.byref(r), C.byref(bufs)))
        return out

    def robust_combine_device(self, d_chunk_sums, split, chunk_passes, width, height, d_ptrs, d_albedo=None, stream=0, **ropts):
        """rt_robust_combine_device: asynchronous, DEVICE planes [S][h][w][3]; allocates nothing."""
        r = robust_opts(**ropts)
        bufs = _device_buffers(abi.ROBUST_SHAPES, abi.RobustBuffers(), d_ptrs)
        _check(lib().rt_robust_combine_device(self._h, _dp(d_chunk_sums), C.c_uint32(split), C.c_uint64(chunk_passes), C.c_uint32(width),
                                              C.c_uint32(height), _dp(d_albedo), C.byref(r), C.byref(bufs), C.c_void_p(stream)))

    def render_denoised_robust(self, camera, opts, dopts=None, **ropts):
        """rt_render_denoised_robust: the AOVs, render_robust with their albedo and the filter on the robust frame (no variance
        plane).  Returns (clean, robust, rays_shot)."""
        h, w = int(opts.height), int(opts.width)
        if dopts is None:
            dopts = denoise_opts(w, h)
        r = robust_opts(**ropts)
        return self._frames_and_rays("rt_render_denoised_robust", (C.byref(camera), C.byref(opts), C.byref(r), C.byref(dopts)),
                                     (h, w, 3), (h, w, 3))

    # ---- temporal accumulation with camera reprojection (rt_denoise_temporal) ----
    def denoise_temporal(self, color, camera, albedo=None, normal=None, depth=None, motion=False, **opts):
        """rt_denoise_temporal: one frame of a camera path.  color (H, W, 3) f32 -- or the dict render_aov returns with the image
        under "color" -- with the optional albedo / normal (H, W, 3) and the REQUIRED depth (H, W); camera: this frame's
        abi.Camera.  The scene keeps the history between calls (temporal_reset forgets it; a new frame size starts over).
        Returns out (H, W, 3) f32, or (out, motion (H, W, 2) f32) with motion=True.  Keyword options: those of denoise_opts and
        of abi.TEMPORAL_OPTIONS.  Semantics: include/rt_hip.h rt_temporal_opts."""
        color, guides = _guides(color, albedo, normal=normal, depth=depth)
        if guides["depth"] is None:
            raise ValueError("denoise_temporal needs depth")
        color, h, w = _image(color, "color")
        ins = abi.TemporalInputs()
        _host_inputs(abi.TEMPORAL_SHAPES, ins, {"color": color, **guides}, h, w)
        o = temporal_opts(w, h, **opts)
        out = np.zeros((h, w, 3), dtype=np.float32)
        mv = np.zeros((h, w, 2), dtype=np.float32) if motion else None
        _check(lib().rt_denoise_temporal(self._h, C.byref(ins), C.byref(camera), C.byref(o), _p(out, C.c_float), _p(mv, C.c_float)))
        return (out, mv) if motion else out

    def temporal_reset(self):
        """rt_denoise_temporal_reset: the next denoise_temporal call has no history."""
        _check(lib().rt_denoise_temporal_reset(self._h))

    def denoise_temporal_device(self, d_ptrs, camera, prev_camera, d_history_in, d_history_out, d_workspace, d_out, opts,
                                d_motion=0, stream=0):
        """rt_denoise_temporal_device: asynchronous, DEVICE buffers of the scene's GPU, no state.  d_ptrs = {input: device
        pointer} over abi.TEMPORAL_INPUTS ("color" and "depth" required); d_history_in 0 = no history (prev_camera may then be
        None); the histories temporal_history_bytes(opts) and the workspace temporal_workspace_bytes(opts) bytes, 16-byte
        aligned; d_motion 0 = not written; opts: abi.TemporalOpts with the frame size set."""
        ins = _device_buffers(abi.TEMPORAL_SHAPES, abi.TemporalInputs(), d_ptrs)
        _check(lib().rt_denoise_temporal_device(self._h, C.byref(ins), C.byref(camera), _ref(prev_camera), _vp(d_history_in), _vp(d_history_out),
                                                C.byref(opts), _vp(d_workspace), _dp(d_out), _dp(d_motion), C.c_void_p(stream)))

    # ---- display stage: auto-exposure, tone curve, transfer, 8-bit output (rt_display) ----
    def display(self, image, histogram=False, **opts):
        """rt_display: an (H, W, 3) f32 frame to (H, W, 4) uint8 (RGBA8 / BGRA8) or (H, W, 3) (RGB8).  The scene keeps the exposure
        state between calls (display_reset forgets it; a new frame size starts over); display_state() is the state after the last
        call.  histogram=True returns (pixels, the 256 uint32 counts).  Keyword options: display_opts'.  Semantics: include/rt_hip.h
        rt_display_opts."""
        a, h, w = _image(image)
        o = display_opts(w, h, **opts)
        out = np.zeros((h, w, 3 if o.pixel_format == abi.RT_PIXEL_RGB8 else 4), dtype=np.uint8)
        hist = np.zeros(abi.DISPLAY_HISTOGRAM_BINS, dtype=np.uint32)
        state = abi.DisplayState()
        _check(lib().rt_display(self._h, _p(a, C.c_float), C.byref(o), out.ctypes.data_as(C.c_void_p), C.byref(state),
                                _p(hist, C.c_uint32)))
        self._display_state = state
        return (out, hist) if histogram else out

    def display_state(self):
        """the abi.DisplayState the last display call left (zero before the first call and after display_reset)"""
        st = abi.DisplayState()
        if getattr(self, "_display_state", None) is not None:
            C.memmove(C.byref(st), C.byref(self._display_state), C.sizeof(st))
        return st

    def display_reset(self):
        """rt_display_reset: the next display call starts from a zero state."""
        _check(lib().rt_display_reset(self._h))
        self._display_state = None

    def display_device(self, d_rgb, opts, d_state, d_workspace, d_out, d_histogram=0, stream=0):
        """rt_display_device: asynchronous, DEVICE buffers of the scene's GPU, no state of its own.  d_rgb: W*H*3 f32; d_state: an
        rt_display_state (16 bytes, read and written on the device; 0 = none); d_workspace: display_workspace_bytes(opts) bytes,
        16-byte aligned; d_out: display_output_bytes(opts) bytes; d_histogram: 256 uint32 or 0; opts: abi.DisplayOpts."""
        _check(lib().rt_display_device(self._h, _dp(d_rgb), C.byref(opts), _vp(d_state), _vp(d_workspace), _vp(d_out),
                                       _dp(d_histogram, C.c_uint32), C.c_void_p(stream)))

    # ---- bloom stage: glare around over-range pixels, ahead of the display stage (rt_bloom) ----
    def bloom(self, image, state=None, **opts):
        """rt_bloom: an (H, W, 3) f32 frame to an (H, W, 3) f32 frame, the input plus `intensity` times a wide blur of its
        over-threshold part.  state: an abi.DisplayState (display_state()) whose ev is added to exposure_ev, or None.  Keyword
        options: bloom_opts'.  Semantics: include/rt_hip.h rt_bloom_opts."""
        a, h, w = _image(image)
        o = bloom_opts(w, h, **opts)
        out = np.zeros((h, w, 3), dtype=np.float32)
        _check(lib().rt_bloom(self._h, _p(a, C.c_float), C.byref(o), _ref(state), _p(out, C.c_float)))
        return out

    def bloom_device(self, d_rgb, opts, d_state, d_workspace, d_out, stream=0):
        """rt_bloom_device: asynchronous, DEVICE buffers of the scene's GPU, no state.  d_rgb, d_out: W*H*3 f32 (d_out may be
        d_rgb); d_state: an rt_display_state read on the device, or 0; d_workspace: bloom_workspace_bytes(opts) bytes, 16-byte
        aligned; opts: abi.BloomOpts."""
        _check(lib().rt_bloom_device(self._h, _dp(d_rgb), C.byref(opts), _vp(d_state), _vp(d_workspace), _dp(d_out), C.c_void_p(stream)))

    # ---- depth-of-field stage: depth-driven disc blur, ahead of the bloom stage (rt_dof) ----
    def dof(self, image, depth, camera=None, coc=False, **opts):
        """rt_dof: an (H, W, 3) f32 frame and its (H, W) depth plane (render_aov's "depth") to the defocused (H, W, 3) frame.
        camera: the abi.Camera the depth was rendered with, or None (then planar_depth must be 0).  coc=True returns (out, the
        (H, W) signed circle-of-confusion radii).  Keyword options: dof_opts'.  Semantics: include/rt_hip.h rt_dof_opts."""
        a, h, w = _image(image)
        z = _f32(depth, (h, w), "depth")
        o = dof_opts(w, h, **opts)
        out = np.zeros((h, w, 3), dtype=np.float32)
        radii = np.zeros((h, w), dtype=np.float32) if coc else None
        _check(lib().rt_dof(self._h, _p(a, C.c_float), _p(z, C.c_float), _ref(camera), C.byref(o), _p(out, C.c_float), _p(radii, C.c_float)))
        return (out, radii) if coc else out

    def dof_device(self, d_rgb, d_depth, camera, opts, d_workspace, d_out, d_coc=0, stream=0):
        """rt_dof_device: asynchronous, DEVICE buffers of the scene's GPU, no state.  d_rgb, d_out: W*H*3 f32 (disjoint); d_depth:
        W*H f32; d_coc: W*H f32 or 0; d_workspace: dof_workspace_bytes(opts) bytes, 16-byte aligned; camera: abi.Camera or None;
        opts: abi.DofOpts."""
        _check(lib().rt_dof_device(self._h, _dp(d_rgb), _dp(d_depth), _ref(camera), C.byref(opts), _vp(d_workspace), _dp(d_out), _dp(d_coc),
                                   C.c_void_p(stream)))

    def render_dof(self, camera, opts, dopts):
        """rt_render_dof: rt_render, the depth of the same passes and rt_dof in one call; dopts: abi.DofOpts (its sizes are
        ignored), e.g. dof_opts_from_camera's.  Returns the defocused (H, W, 3) frame."""
        out = np.zeros((int(opts.height), int(opts.width), 3), dtype=np.float32)
        _check(lib().rt_render_dof(self._h, C.byref(camera), C.byref(opts), C.byref(dopts), _p(out, C.c_float)))
        return out

    # ---- AOV-guided upscaling (rt_upscale): a source-size frame to the destination size ----
    def upscale(self, color, src=None, dst=None, stage=False, **opts):
        """rt_upscale: an (h, w, 3) f32 frame to (H, W, 3), guided by the albedo / normal (.., 3) and depth of `src` (at h x w) and
        `dst` (at H x W): dicts as render_aov returns them (other channels are ignored); a guide is used when both hold it, and
        both must then hold it.  Without guides `dst` is the destination size (H, W): plain bilinear interpolation.
        stage=True returns (out, the (H, W) uint8 stage map).  Keyword options: abi.UPSCALE_OPTIONS.  Semantics: include/rt_hip.h
        rt_upscale_opts."""
        src = src or {}
        if isinstance(dst, dict):
            shapes = [np.shape(dst[k])[:2] for k in abi.UPSCALE_GUIDES if dst.get(k) is not None]
            if not shapes:
                raise ValueError("upscale: dst holds no guide; pass the destination size (H, W) instead")
            H, W = shapes[0]
        elif dst is not None:
            (H, W), dst = dst, {}
        else:
            raise ValueError("upscale needs dst: the destination guides, or the destination size (H, W)")
        color, h, w = _image(color, "color")
        ins = abi.UpscaleInputs()
        _host_inputs(abi.UPSCALE_SHAPES, ins, {"color": color, **{"src_" + k: src.get(k) for k in abi.UPSCALE_GUIDES}}, h, w)
        _host_inputs(abi.UPSCALE_SHAPES, ins, {"dst_" + k: dst.get(k) for k in abi.UPSCALE_GUIDES}, H, W)
        o = upscale_opts(w, h, W, H, **opts)
        out = np.zeros((H, W, 3), dtype=np.float32)
        smap = np.zeros((H, W), dtype=np.uint8) if stage else None
        _check(lib().rt_upscale(self._h, C.byref(ins), C.byref(o), _p(out, C.c_float), _p(smap, C.c_uint8)))
        return (out, smap) if stage else out

    def upscale_device(self, d_ptrs, d_out, opts, d_stage=0, stream=0):
        """rt_upscale_device: asynchronous, DEVICE buffers of the scene's GPU, no state, no workspace.  d_ptrs = {input: device
        pointer} over abi.UPSCALE_INPUTS ("color" required; each guide at both sizes or not at all); d_out: W*H*3 f32; d_stage:
        W*H bytes or 0; opts: abi.UpscaleOpts with both frame sizes set."""
        ins = _device_buffers(abi.UPSCALE_SHAPES, abi.UpscaleInputs(), d_ptrs)
        _check(lib().rt_upscale_device(self._h, C.byref(ins), C.byref(opts), _dp(d_out), _dp(d_stage, C.c_uint8), C.c_void_p(stream)))

    def render_upscaled(self, camera, opts, src_width, src_height, dopts=None, uopts=None):
        """rt_render_upscaled: trace and filter at src_width x src_height, reconstruct opts.width x opts.height.  Returns (out
        (H, W, 3), out_src (h, w, 3): the filtered source frame, rays_shot).  dopts / uopts: abi.DenoiseOpts / abi.UpscaleOpts
        (their sizes are ignored) or None for the defaults."""
        H, W, h, w = int(opts.height), int(opts.width), int(src_height), int(src_width)
        if dopts is None:
            dopts = denoise_opts(w, h)
        if uopts is None:
            uopts = upscale_opts(w, h, W, H)
        return self._frames_and_rays("rt_render_upscaled", (C.byref(camera), C.byref(opts), C.c_uint32(w), C.c_uint32(h), C.byref(dopts),
                                                            C.byref(uopts)), (H, W, 3), (h, w, 3))

    # ---- AccelerationStructure::check_hit / check_hit_index for batches ----
    def check_hit(self, origins, directions):
        rays = _pack_rays(origins, directions)
        out = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        _check(lib().rt_check_hit(self._h, rays.ctypes.data_as(C.POINTER(abi.RayDesc)), C.c_uint64(rays.shape[0]),
                                  out.ctypes.data_as(C.POINTER(abi.HitRecord))))
        return out

    def check_hit_index(self, origins, directions, indices):
        rays = _pack_rays(origins, directions)
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        out = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        _check(lib().rt_check_hit_index(self._h, rays.ctypes.data_as(C.POINTER(abi.RayDesc)), _p(idx, C.c_uint64),
                                        C.c_uint64(rays.shape[0]), out.ctypes.data_as(C.POINTER(abi.HitRecord))))
        return out

    # ---- radiance queries (rt_radiance): the integrator on caller-supplied rays ----
    def radiance(self, origins, directions, *, streams=None, method=abi.RT_METHOD_MIS, samples=1, seed=0, sample_begin=0,
                 max_depth=50, rr_threshold=3):
        """The mean of `samples` samples of Naive / MisIntegrator::get_colour along each ray, as an (n, 3) f32 array.  Sample k of
        ray i runs on the stream (seed, streams[i] or i, sample_begin + k) with no draw ahead of the integrator (no jitter: a query
        of a camera's rays does not reproduce a frame's bytes).  Semantics: include/rt_hip.h rt_radiance_opts."""
        rays = _pack_rays(origins, directions)
        n = rays.shape[0]
        out = np.zeros((n, 3), dtype=np.float32)
        st = None
        if streams is not None:
            st = np.ascontiguousarray(streams, dtype=np.uint64)
            if st.shape != (n,):
                raise ValueError(f"streams must be one per ray: {st.shape} for {n} rays")
        o = radiance_opts(render_method=method, samples_per_ray=samples, seed=seed, sample_begin=sample_begin, max_depth=max_depth,
                          rr_threshold=rr_threshold)
        _check(lib().rt_radiance(self._h, rays.ctypes.data_as(C.POINTER(abi.RayDesc)), _p(st, C.c_uint64), C.c_uint64(n), C.byref(o),
                                 _p(out, C.c_float)))
        return out

    def radiance_device(self, d_rays, d_streams, n_rays, d_out, *, method=abi.RT_METHOD_MIS, samples=1, seed=0, sample_begin=0,
                        max_depth=50, rr_threshold=3, stream=0):
        """rt_radiance_device: asynchronous, DEVICE pointers on the scene's GPU -- d_rays n x rt_ray_desc, d_streams n x u64 or
        0 / None (stream i = i), d_out 3 n f32.  Allocates nothing and keeps no state: capturable from the first call, and safe
        on several streams at once."""
        o = radiance_opts(render_method=method, samples_per_ray=samples, seed=seed, sample_begin=sample_begin, max_depth=max_depth,
                          rr_threshold=rr_threshold)
        _check(lib().rt_radiance_device(self._h, C.c_void_p(d_rays), _vp(d_streams), C.c_uint64(n_rays), C.byref(o),
                                        _dp(d_out, C.c_float), C.c_void_p(stream)))


def output_floats(opts):
    return _u64("rt_render_output_floats", opts)


def plan_work_items(opts, split, share, resident_waves=0):
    """(whole_claims, n_items) of a render under `opts` at an explicit split and whole-pixel share (rt_plan_work_items, host-side);
    share -1 is the library's own choice for a device that holds `resident_waves` waves at once"""
    whole, n = C.c_uint32(), C.c_uint64()
    _check(lib().rt_plan_work_items(C.byref(opts), C.c_uint32(split), C.c_int(share), C.c_uint64(resident_waves), C.byref(whole), C.byref(n)))
    return whole.value, n.value


def shard_pixel_order(opts):
    n = output_floats(_with_layout(opts, abi.RT_LAYOUT_SHARD)) // 3
    out = np.zeros(max(1, n), dtype=np.uint64)
    _check(lib().rt_shard_pixel_order(C.byref(opts), _p(out, C.c_uint64), C.c_uint64(n)))
    return out[:n]


def _with_layout(opts, layout):
    o = abi.RenderOpts()
    C.memmove(C.byref(o), C.byref(opts), C.sizeof(o))
    o.output_layout = layout
    return o


class SamplerProgress:
    """samplers/mod.rs:49-63."""

    def __init__(self, pixel_num, channels=3):
        self.samples_completed = 0
        self.rays_shot = 0
        self.current_image = np.zeros(pixel_num * channels, dtype=np.float32)


class RandomSampler:
    """`impl Sampler` backed by the HIP kernels (samplers/random_sampler.rs:10-99).

    The reference hands its callback ONE image per pass; shipping 24.9 MB over PCIe per pass is
    what the batch ABI avoids, so passes are rendered `batch` at a time and the callback receives
    each batch's mean together with the number of passes it stands for.  With batch=1 the callback
    contract is exactly the reference's: f(data, progress, i) for i = 1..=spp, True cancels.
    """

    def __init__(self, batch=None):
        self.batch = batch

    def sample_image(self, render_options, camera, scene, presentation_update=None):
        """rt_sample_image: batch j+1 renders while batch j is copied out and handed to the callback."""
        opts = _with_layout(render_options, abi.RT_LAYOUT_FRAME)
        state = {"error": None}

        def trampoline(_data, p, done):
            try:
                progress = SamplerProgress(0)
                progress.samples_completed = int(p.contents.samples_completed)
                progress.rays_shot = int(p.contents.rays_shot)
                # a view of the sampler's pinned buffer: valid during the callback only
                progress.current_image = np.ctypeslib.as_array(p.contents.current_image, shape=(int(p.contents.n_floats),))
                if presentation_update is None:
                    return 0
                data, f = presentation_update
                return 1 if f(data, progress, int(done)) else 0
            except BaseException as e:  # an exception must not unwind through the C frames
                state["error"] = e
                return 1

        cb = abi.PresentationUpdate(trampoline)
        _check(lib().rt_sample_image(scene._h, C.byref(camera), C.byref(opts), C.c_uint64(self.batch or 0), cb, None))
        if state["error"] is not None:
            raise state["error"]


def running_mean_update(image, progress, i):
    """The TUI callback (src/main.rs:175-191) generalised to a batch of `progress.samples_completed`
    passes: image += (batch_mean - image) * n / i."""
    n = progress.samples_completed
    image += (progress.current_image - image) * (np.float32(n) / np.float32(i))
    return False


def output_rgb8(image, gamma=2.2):
    """save_data_to_image's pixel conversion (crates/output/src/lib.rs:92-95): (v.powf(1/gamma) * 255.999) as u8."""
    a = np.ascontiguousarray(image, dtype=np.float32)
    out = np.zeros(a.shape, dtype=np.uint8)
    _check(lib().rt_output_rgb8(_p(a, C.c_float), C.c_uint64(a.size), C.c_float(gamma), _p(out, C.c_uint8)))
    return out


def save_image(filename, image, gamma=2.2):
    """save_data_to_image (crates/output/src/lib.rs:74-113): .png .ppm .bmp .tiff (RGB8 after gamma) or .exr (floats) by extension."""
    a = np.ascontiguousarray(image, dtype=np.float32)
    h, w, _ = a.shape
    _check(lib().rt_output_save(filename.encode(), _p(a, C.c_float), C.c_uint32(w), C.c_uint32(h), C.c_float(gamma)))


def _set_opts(o, what, kw, allowed, enums=None, nested=None):
    """the keywords of every *_opts builder set on the struct `o`: a key must be in `allowed`, or in `nested` ({key: the struct
    inside `o` that holds it}).  With `enums` ({key: {name: value}}) a string stands for the value of that name, in either case."""
    for k, v in kw.items():
        _known(k, (*allowed, *(nested or ())), f"{what} option")
        if enums and isinstance(v, str):
            names = enums.get(k, {})
            _known(v.lower(), names, k)
            v = names[v.lower()]
        setattr((nested or {}).get(k, o), k, v)
    return o


def _opts(struct, what, kw, allowed, enums=None, **size):
    """rt_<what>_opts_default's `struct` with the frame-size fields `size`, then the keywords `kw` (see _set_opts), set"""
    o = struct()
    _check(getattr(lib(), f"rt_{what}_opts_default")(C.byref(o)))
    for k, v in size.items():
        setattr(o, k, int(v))
    return _set_opts(o, what, kw, allowed, enums)


_DENOISE_OPTIONS = ("iterations", "sigma_luminance", "sigma_normal", "sigma_depth")


def denoise_opts(width, height, **kw):
    """rt_denoise_opts_default with the frame size and any of iterations / sigma_luminance / sigma_normal / sigma_depth set."""
    return _opts(abi.DenoiseOpts, "denoise", kw, _DENOISE_OPTIONS, width=width, height=height)


def matte_opts(**kw):
    """rt_matte_opts_default with id_kind (abi.RT_MATTE_ID_* or its name, "primitive" / "material") and / or layers set."""
    return _opts(abi.MatteOpts, "matte", kw, ("id_kind", "layers"), {"id_kind": abi.MATTE_ID_KINDS})


def ao_opts(**kw):
    """rt_ao_opts_default with rays_per_pass and / or radius set."""
    return _opts(abi.AoOpts, "ao", kw, ("rays_per_pass", "radius"))


def radiance_opts(**kw):
    """rt_radiance_opts_default with any of seed, sample_begin, samples_per_ray, render_method, max_depth, rr_threshold set."""
    return _opts(abi.RadianceOpts, "radiance", kw, abi.RADIANCE_OPTIONS)


def probe_opts(**kw):
    """rt_probe_opts_default with any of seed, sample_begin, samples_per_probe, sample_split, render_method, max_depth,
    rr_threshold, convolve set."""
    return _opts(abi.ProbeOpts, "probe", kw, abi.PROBE_OPTIONS)


def probe_workspace_bytes(n_probes, **kw):
    """rt_probe_workspace_bytes: the bytes probe_sh_device's workspace must hold for n_probes under probe_opts(**kw)."""
    n = C.c_uint64()
    _check(lib().rt_probe_workspace_bytes(C.c_uint64(n_probes), C.byref(probe_opts(**kw)), C.byref(n)))
    return n.value


def noise_opts(**kw):
    """rt_noise_opts_default with luminance_floor and / or threshold set."""
    return _opts(abi.NoiseOpts, "noise", kw, ("luminance_floor", "threshold"))


def robust_opts(**kw):
    """rt_robust_opts_default with mode (abi.RT_ROBUST_* or its name, "trim" / "median" / "gini"), trim and / or gini_gain set."""
    return _opts(abi.RobustOpts, "robust", kw, ("mode", "trim", "gini_gain"), {"mode": abi.ROBUST_MODES})


def _summary_dict(s):
    return {"max_tile_error": np.float32(s.max_tile_error), "tiles_above": int(s.tiles_above), "n_tiles": int(s.n_tiles)}


def denoise_workspace_bytes(opts):
    """rt_denoise_workspace_bytes: the workspace rt_denoise_device needs for opts' frame size."""
    return _u64("rt_denoise_workspace_bytes", opts)


def temporal_opts(width, height, **kw):
    """rt_temporal_opts_default with the frame size and any of the denoise_opts keywords (iterations, sigma_*) or
    abi.TEMPORAL_OPTIONS set."""
    o = _opts(abi.TemporalOpts, "temporal", {}, ())
    o.denoise.width, o.denoise.height = int(width), int(height)
    return _set_opts(o, "temporal", kw, abi.TEMPORAL_OPTIONS, nested=dict.fromkeys(_DENOISE_OPTIONS, o.denoise))


def temporal_history_bytes(opts):
    """rt_temporal_history_bytes: the size of one history buffer for opts' frame size."""
    return _u64("rt_temporal_history_bytes", opts)


def temporal_workspace_bytes(opts):
    """rt_temporal_workspace_bytes: the workspace rt_denoise_temporal_device needs for opts' frame size."""
    return _u64("rt_temporal_workspace_bytes", opts)


def display_opts(width, height, **kw):
    """rt_display_opts_default with the frame size and any of abi.DISPLAY_OPTIONS set; the enum options also take their names
    (tonemap="hable", pixel_format="rgb8", ...)."""
    return _opts(abi.DisplayOpts, "display", kw, abi.DISPLAY_OPTIONS, abi.DISPLAY_ENUMS, width=width, height=height)


def display_workspace_bytes(opts):
    """rt_display_workspace_bytes: the workspace rt_display_device needs for opts' frame size."""
    return _u64("rt_display_workspace_bytes", opts)


def display_output_bytes(opts):
    """rt_display_output_bytes: W*H*4 (RGBA8, BGRA8) or W*H*3 (RGB8)."""
    return _u64("rt_display_output_bytes", opts)


def bloom_opts(width, height, **kw):
    """rt_bloom_opts_default with the frame size and any of abi.BLOOM_OPTIONS set."""
    return _opts(abi.BloomOpts, "bloom", kw, abi.BLOOM_OPTIONS, width=width, height=height)


def bloom_workspace_bytes(opts):
    """rt_bloom_workspace_bytes: the workspace rt_bloom_device needs for opts' frame size and levels."""
    return _u64("rt_bloom_workspace_bytes", opts)


def dof_opts(width, height, **kw):
    """rt_dof_opts_default with the frame size and any of abi.DOF_OPTIONS set."""
    return _opts(abi.DofOpts, "dof", kw, abi.DOF_OPTIONS, width=width, height=height)


def dof_opts_from_camera(camera, aperture, focus_dist, width, height, **kw):
    """rt_dof_opts_from_camera: a scene file's aperture and focus_dis as the blur of `camera` (made with that focus_dist) at
    width x height; then any of abi.DOF_OPTIONS set (max_radius, say)."""
    o = abi.DofOpts()
    _check(lib().rt_dof_opts_from_camera(C.byref(o), C.byref(camera), C.c_float(aperture), C.c_float(focus_dist),
                                         C.c_uint32(int(width)), C.c_uint32(int(height))))
    return _set_opts(o, "dof", kw, abi.DOF_OPTIONS)


def dof_workspace_bytes(opts):
    """rt_dof_workspace_bytes: the workspace rt_dof_device needs for opts' frame size."""
    return _u64("rt_dof_workspace_bytes", opts)


def upscale_opts(src_width, src_height, dst_width, dst_height, **kw):
    """rt_upscale_opts_default with the two frame sizes and any of abi.UPSCALE_OPTIONS set."""
    return _opts(abi.UpscaleOpts, "upscale", kw, abi.UPSCALE_OPTIONS, src_width=src_width, src_height=src_height, dst_width=dst_width,
                 dst_height=dst_height)


def save_aov(prefix, aovs):
    """Write the albedo and normal buffers of HipScene.render_aov as `<prefix>_albedo.exr` / `<prefix>_normal.exr` (float
    channels, through rt_output_save; the denoiser inputs).  Returns the paths written."""
    paths = []
    for name in ("albedo", "normal"):
        if name in aovs:
            path = f"{prefix}_{name}.exr"
            save_image(path, aovs[name])
            paths.append(path)
    return paths


def get_readable_duration(seconds):
    """output::get_readable_duration (crates/output/src/lib.rs:33-63), whole seconds as Duration::as_secs."""
    total = int(seconds)
    days, hours, minutes, secs = total // 86400, (total % 86400) // 3600, (total % 3600) // 60, total % 60

    def part(n, unit):
        return "" if n == 0 else (f"{n} {unit}, " if n == 1 else f"{n} {unit}s, ")

    tail = "~0 seconds" if secs == 0 else (f"{secs} second" if secs == 1 else f"{secs} seconds")
    return part(days, "day") + part(hours, "hour") + part(minutes, "minute") + tail


def final_statistics(seconds, ray_count, samples):
    """The message of output::print_final_statistics (crates/output/src/lib.rs:115-124)."""
    return (f"Finished rendering:\n\tSamples:\t{samples}\n\tTime taken:\t{get_readable_duration(seconds)}\n"
            f"\tRays shot:\t{ray_count} @ {ray_count / seconds / 1000000.0:.2f} Mray/s")
