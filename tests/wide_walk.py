"""The walk of the COMPACT wide-node bytes (what the kernels fetch: HipScene.wide_tree_compact of a host-only scene) in numpy f32,
the way rt_intersect.h descend4 steps through them, and the two-child walk of the reference nodes beside it.  A support module:
test_host_bvh.py shows with it that no walk enters an absent child, render_variant_cases.py measures with it how many stack
entries the walks of a frame's camera rays leave pending -- what a forced RT_TUNE_STACK_CAP has to lie below to reach the global
overflow area.  Neither walk prunes and neither looks at a primitive (limit_valid = false): see pending_entries for why that is
what the pruned device walk does as well, up to a point that is known.  torch is never imported here."""
import numpy as np

LEAF = 0x80000000
NONE = 0x7FFFFFFE
SLOT_MASK = 0x03FFFFFF


def f32(x):
    return np.float32(x)


def fma(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def descend4_children(node, o, inv, use_present_mask):
    """child slots descend4 would visit (nearest first), emulated in f32; no pruning (limit_valid = false)"""
    exps = int(node["exps"])
    s = [np.uint32(((exps >> (8 * a)) & 0xFF) << 23).view(np.float32) for a in range(3)]
    a_ = [f32(s[k] * inv[k]) for k in range(3)]
    b_ = [f32(f32(node["origin"][k] - o[k]) * inv[k]) for k in range(3)]
    near = [int(node["qhi"][k]) if inv[k] < 0 else int(node["qlo"][k]) for k in range(3)]
    far = [int(node["qlo"][k]) if inv[k] < 0 else int(node["qhi"][k]) for k in range(3)]
    big = f32(max(abs(b_[0]), abs(b_[1]), abs(b_[2])) + f32(255.0) * max(abs(a_[0]), abs(a_[1]), abs(a_[2])))
    pad = f32(f32(1.0e-5) * big)
    present = int(node["child"][1]) >> 26
    out = []
    for c in range(4):
        tn = max(fma(f32((near[k] >> (8 * c)) & 0xFF), a_[k], b_[k]) for k in range(3))
        tf = min(fma(f32((far[k] >> (8 * c)) & 0xFF), a_[k], b_[k]) for k in range(3))
        te = max(f32(tn - pad), f32(0.0))
        h = (f32(tf - tn) >= f32(-2.0) * pad) and (tf >= -pad)
        if use_present_mask and c >= 2:
            h = h and ((present >> c) & 1) != 0
        if h:
            # the kernel sorts by the bits of te with the slot in the two low bits
            out.append((int(np.float32(te).view(np.uint32)) & ~3 | c, c))
    return [c for _, c in sorted(out)]


def compact_ref(node, c):
    delta = (int(node["exps"]) >> (24 + 2 * c)) & 3
    if (int(node["child"][0]) >> (26 + c)) & 1:
        return LEAF | ((int(node["child"][1]) & SLOT_MASK) + delta)
    return (int(node["child"][0]) & SLOT_MASK) + delta


def ray_inverse(d):
    """(normalised direction, its reciprocal) as Ray::new forms them"""
    with np.errstate(all="ignore"):
        d = np.asarray(d, np.float32)
        d = (d / np.sqrt((d * d).sum(dtype=np.float32))).astype(np.float32)
        return d, (np.float32(1.0) / d).astype(np.float32)


def walk_compact_pending(nodes, root, o, d, use_present_mask, max_steps):
    """the unpruned wide walk of one ray: (leaf indices reached, absent slots visited, node steps, the largest number of pending
    stack entries, the largest number up to the moment the walk reaches its first leaf, absent children of the nodes visited);
    gives up after max_steps node steps"""
    with np.errstate(all="ignore"):
        _, inv = ray_inverse(d)
        stack, leaves, phantoms, steps, most, most_to_first_leaf, absent_seen = [root], [], 0, 0, 0, 0, 0
        while stack and steps < max_steps:
            ref = stack.pop()
            if ref & LEAF:
                leaves.append(ref & SLOT_MASK)
                continue
            steps += 1
            node = nodes[ref]
            kids = descend4_children(node, o, inv, use_present_mask)
            present = int(node["child"][1]) >> 26
            absent_seen += 4 - bin(present & 0xF).count("1")
            phantoms += sum(1 for c in kids if not (present >> c) & 1)
            for c in reversed(kids):
                stack.append(compact_ref(node, c))
            # descend4 keeps the nearest child in a register: what it has pushed is every other one
            pending = len(stack) - 1 if kids else len(stack)
            most = max(most, pending)
            if not leaves:
                most_to_first_leaf = max(most_to_first_leaf, pending)
    return leaves, phantoms, steps, most, most_to_first_leaf, absent_seen


def walk_compact(nodes, root, o, d, use_present_mask, max_steps):
    """(leaf indices reached, absent slots visited, node steps); gives up after max_steps node steps"""
    return walk_compact_pending(nodes, root, o, d, use_present_mask, max_steps)[:3]


def _slabs(lo, hi, o, inv):
    """AABB::does_int as the oracle and the kernels state it (aabb.rs: t1 = (min - o) * inv, t2 = (max - o) * inv, tmax widened by
    1 + 2 gamma(3); Rust's min / max ignore a NaN operand), f32"""
    with np.errstate(all="ignore"):
        t1 = ((lo - o) * inv).astype(np.float32)
        t2 = ((hi - o) * inv).astype(np.float32)
        tmin = np.fmin(t1, t2)
        tmax = np.fmax(t1, t2)
        widen = np.float32(1.0 + 2.0 * (3 * 2.0 ** -24) / (1.0 - 3 * 2.0 ** -24))
        near = np.fmax.reduce(tmin)
        far = np.fmin.reduce((tmax * widen).astype(np.float32))
        return bool(near <= far) and bool(far > 0)


def walk_two_child_pending(ref_nodes, o, d):
    """the unpruned two-child walk (rt_intersect.h descend_view, PRUNE = false) over the reference nodes (HipScene.nodes()): the
    largest number of pending stack entries.  A stand-in for the slab test's last ulp is enough here: the result is compared with
    stack_depth_narrow, a bound that holds for ANY set of boxes hit."""
    _, inv = ray_inverse(d)
    o = np.asarray(o, np.float32)
    if int(ref_nodes[0]["children"][0]) < 0:
        return 0
    stack, most = [0], 0
    while stack:
        n = ref_nodes[stack.pop()]
        if int(n["children"][0]) < 0:
            continue
        kids = [int(c) for c in n["children"]]
        hit = [c for c in kids if _slabs(ref_nodes[c]["min"][:3], ref_nodes[c]["max"][:3], o, inv)]
        for c in reversed(hit):
            stack.append(c)
        most = max(most, len(stack) - 1 if hit else len(stack))
    return most


def pixel_centre_rays(camera, width, height):
    """(origin [3], un-normalised directions [width * height, 3]) through the pixel centres, with the sampler's own expression
    u = (0.5 + x) / (W - 1), v = 1 - (0.5 + y) / (H - 1) (random_sampler.rs:50-61 with the jitter at its mean)"""
    pixels = np.arange(width * height)
    x, y = (pixels % width).astype(np.float32), (pixels // width).astype(np.float32)
    u = (np.float32(0.5) + x) / np.float32(width - 1)
    v = np.float32(1.0) - (np.float32(0.5) + y) / np.float32(height - 1)
    o = np.array(camera.origin[:], dtype=np.float32)
    ll, hz, vt = (np.array(getattr(camera, k)[:], dtype=np.float32) for k in ("lower_left", "horizontal", "vertical"))
    d = ((ll[None, :] + hz[None, :] * u[:, None]) + vt[None, :] * v[:, None]) - o[None, :]
    return o, d.astype(np.float32)


def pending_entries(host_scene, camera, width, height, misses=None):
    """Over the pixel-centre rays of a width x height frame, on the compact wide tree of a host-only scene:
      "unpruned"  the largest number of pending entries of the walk that prunes nothing (an upper bound for any pruned walk);
      "reached"   the largest number the PRUNED device walk provably reaches: descend4 prunes only once the walk holds a hit
                  (limit_valid = best_prim != kNoPrim), so it IS the unpruned walk until the first leaf it reaches, and for a ray
                  that hits nothing (`misses`: a mask over the pixels, from the oracle's check_hit) to its end;
      "absent"    absent children of the nodes those walks visit; "rays": the rays that met one.
    The kernel's `sp` after its pushes is what is counted: a store at index i goes to the overflow area when i >= cap, so a cap
    is exceeded when it lies below the number reached."""
    nodes, _ = host_scene.wide_tree_compact()
    explicit, root, depth, _ = host_scene.wide_tree()
    out = {"unpruned": 0, "reached": 0, "absent": 0, "rays": 0, "depth": int(depth), "nodes": int(len(nodes))}
    if len(nodes) == 0:
        return out
    o, dirs = pixel_centre_rays(camera, width, height)
    for i, d in enumerate(dirs):
        leaves, phantoms, steps, most, to_first, absent = walk_compact_pending(nodes, root, o, d, True, 50 * len(nodes) + 50)
        assert phantoms == 0 and steps <= len(nodes), (i, phantoms, steps)
        out["unpruned"] = max(out["unpruned"], most)
        out["reached"] = max(out["reached"], most if (misses is not None and misses[i]) else to_first)
        out["absent"] += absent
        out["rays"] += 1 if absent else 0
    return out


def two_child_pending(host_scene, camera, width, height, stride=1):
    """the largest number of pending entries of the unpruned two-child walk over every stride-th pixel-centre ray"""
    ref_nodes = host_scene.nodes()
    o, dirs = pixel_centre_rays(camera, width, height)
    return max(walk_two_child_pending(ref_nodes, o, d) for d in dirs[::stride])
