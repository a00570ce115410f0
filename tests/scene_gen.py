"""Seeded scene descriptions for the parity tests: rt_scene_desc values nobody wrote by hand.

generate(recipe, seed) returns a GenScene with HostScene's surface (.desc, .frame(), .nodes(), .spheres(), ...), so that
DeviceScene, OracleScene.from_desc / from_host, plan_walk_array and regroup_leaves take it unchanged.  Plain numpy; the
product's host library is not involved, so nothing here shares code with what it is compared against.

Rules every recipe follows:
  * values are written as the ABI states them (include/rt_abi.h): a quad carries Q, u, v and the derived n, D, w, computed
    here in float64 and rounded once; an instance carries sin and cos of its angle; a medium -1 / density;
  * a leaf's box contains its object: computed in float64 over the whole shutter [0, 1] and rounded outward, a quad's box
    padded by 1e-3 on every side (the reference's rule for its flat boxes); an interior box is the exact union of its
    children's boxes.  Parity never depends on the box rule: both sides read the description's boxes;
  * the tree is a binary split of the leaves in list order at a point drawn from the seed -- not the median, and not
    sorted along any axis;
  * lights are solid-coloured (the reference's diffuse_light is never textured).
"""
from __future__ import annotations

import math

import numpy as np

import accelerated_ray_tracer_amd as art

TEXTURE_DTYPE = np.dtype([("kind", "<i4"), ("a", "<i4"), ("b", "<i4"), ("scale", "<f4"), ("color", "<f4", 3), ("c", "<i4"), ("p", "<f4", 8)])
BOX_DTYPE = np.dtype([("first_quad", "<i4")])
assert TEXTURE_DTYPE.itemsize == 64

SPHERE, QUAD, BOX, INSTANCE, MEDIUM = range(5)
LAMBERTIAN, METAL, DIELECTRIC, LIGHT, ISOTROPIC = range(5)
T_SOLID, T_CHECKER, T_IMAGE, T_NOISE, T_NOODLE, T_FELT, T_UVOFF = range(7)
ROTATE_Y, TRANSLATE = 1, 2

RECIPES = ["spheres_plain", "spheres_checker", "spheres_tex", "general_plain", "general_tex", "media_many", "limits"]
LIMIT_COUNTS = [1, 2, 12, 13, 24, 25, 63, 64, 65]     # `limits`: seed k -> LIMIT_COUNTS[k % 9] leaves, k >= 9: one of them a quad
LIMIT_SEEDS = list(range(2 * len(LIMIT_COUNTS)))

# the product's documented limits for tier data (rt_abi.hip, build_tier_data): at most 64 x 64 leaves, at most two media leaves
TIER_MAX_LEAVES, TIER_MAX_MEDIA = 64 * 64, 2


def ref(kind: int, index: int) -> int:
    return (kind << 28) | index


def _down(x):
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def _up(x):
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


class GenScene:
    """A generated description and the arrays behind it (kept alive here; the description points into them)."""

    def __init__(self, name, arrays, camera, nx, ny, ns, gamma, background, gradient, contents):
        self.name = name
        self._a = arrays
        self.nx, self.ny, self.ns, self.gamma = nx, ny, ns, gamma
        self.background, self.use_gradient_bg = [float(x) for x in background], int(gradient)
        self.contents = set(contents)      # the oracle counters this scene's contents imply (tests/test_desc_oracle.py)
        d = art.RtSceneDesc()
        for field, count in (("nodes", "n_nodes"), ("spheres", "n_spheres"), ("quads", "n_quads"), ("boxes", "n_boxes"),
                             ("instances", "n_instances"), ("media", "n_media"), ("materials", "n_materials"), ("textures", "n_textures")):
            arr = arrays[field]
            setattr(d, field, arr.ctypes.data if len(arr) else None)
            setattr(d, count, len(arr))
        img = arrays["images"]
        d.images = img.ctypes.data if len(img) else None
        d.image_bytes = len(img)
        d.camera = camera
        self.desc = d

    def _copy(self, k):
        return self._a[k].copy()

    def nodes(self): return self._copy("nodes")
    def spheres(self): return self._copy("spheres")
    def quads(self): return self._copy("quads")
    def boxes(self): return self._copy("boxes")
    def instances(self): return self._copy("instances")
    def media(self): return self._copy("media")
    def materials(self): return self._copy("materials")
    def textures(self): return self._copy("textures")

    def leaf_order(self):
        n = self._a["nodes"]
        out = np.full(len(n), -1, np.int32)
        out[n["prim"] >= 0] = np.arange(int((n["prim"] >= 0).sum()))
        return out

    frame = art.HostScene.frame

    @property
    def n_leaves(self):
        return int((self._a["nodes"]["prim"] >= 0).sum())

    @property
    def has_tier_data(self):
        """Whether rt_scene_create builds tier data for this scene, from the documented limits alone."""
        prim = self._a["nodes"]["prim"]
        media_leaves = int(((prim >= 0) & ((prim >> 28) == MEDIUM)).sum())
        return 0 < self.n_leaves <= TIER_MAX_LEAVES and media_leaves <= TIER_MAX_MEDIA

    def emptied(self):
        """The same camera and frame with no objects (n_nodes = 0)."""
        a = dict(self._a, nodes=np.zeros(0, art.NODE_DTYPE))
        return GenScene(self.name + "/empty", a, self.desc.camera, self.nx, self.ny, self.ns, self.gamma, self.background,
                        self.use_gradient_bg, ())

    def close(self):
        pass


def make_camera(lookfrom, lookat, vfov, aspect, aperture, focus_dist, t0, t1):
    """camera.cuh:59-78 in float64, rounded once per field."""
    lookfrom, lookat = np.asarray(lookfrom, np.float64), np.asarray(lookat, np.float64)
    hh = math.tan(math.radians(vfov) / 2)
    hw = aspect * hh
    w = lookfrom - lookat
    w /= np.linalg.norm(w)
    u = np.cross([0.0, 1.0, 0.0], w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    c = art.RtCamera()
    c.origin[:] = lookfrom.astype(np.float32)
    c.lower_left_corner[:] = (lookfrom - hw * focus_dist * u - hh * focus_dist * v - focus_dist * w).astype(np.float32)
    c.horizontal[:] = (2 * hw * focus_dist * u).astype(np.float32)
    c.vertical[:] = (2 * hh * focus_dist * v).astype(np.float32)
    c.u[:] = u.astype(np.float32)
    c.v[:] = v.astype(np.float32)
    c.lens_radius = aperture / 2
    c.time0, c.time1 = t0, t1
    return c


class Builder:
    def __init__(self, rng):
        self.rng = rng
        self.sph, self.qd, self.bx, self.ins, self.med, self.mat, self.tex = [], [], [], [], [], [], []
        self.images = np.zeros(0, np.uint8)
        self.leaves = []          # (prim ref, lo float32[3], hi float32[3])
        self.contents = set()

    # ---- textures
    def _tex(self, kind, a=0, b=0, scale=0.0, color=(0, 0, 0), c=0, p=()):
        t = np.zeros((), TEXTURE_DTYPE)
        t["kind"], t["a"], t["b"], t["scale"], t["color"], t["c"] = kind, a, b, scale, color, c
        t["p"][: len(p)] = p
        self.tex.append(t)
        return len(self.tex) - 1

    def colour(self, lo=0.1, hi=0.9):
        return self.rng.uniform(lo, hi, 3)

    def t_solid(self, c=None): return self._tex(T_SOLID, color=self.colour() if c is None else c)
    def t_checker(self, a, b, scale): return self._tex(T_CHECKER, a, b, 1.0 / scale)      # the field holds 1 / scale
    def t_noise(self, scale): return self._tex(T_NOISE, scale=scale)
    def t_felt(self): return self._tex(T_FELT, scale=self.rng.uniform(4, 20), color=self.colour(0.3, 0.9), p=(0.08, self.rng.uniform(2, 6), 0.03))
    def t_uvoff(self, base, du, dv): return self._tex(T_UVOFF, a=base, scale=du, p=(dv,))

    def t_noodle(self, octaves):
        d = self.rng.normal(size=3)
        d /= np.linalg.norm(d)
        return self._tex(T_NOODLE, a=octaves, scale=self.rng.uniform(2, 6), color=self.colour(0.5, 1.0),
                         p=tuple(self.colour(0.1, 0.4)) + tuple(d) + (self.rng.uniform(1, 4), self.rng.uniform(0.3, 1.2)))

    def t_image(self, w, h):
        """A small RGB8 image made from the seed, appended to the pool (so later images sit at non-zero byte offsets)."""
        off = len(self.images)
        self.images = np.concatenate([self.images, self.rng.integers(0, 256, w * h * 3, dtype=np.uint8)])
        return self._tex(T_IMAGE, a=off, b=w, c=h)

    def texture_zoo(self):
        """Every texture the tex recipes use: noise, noodle at 0, 1 and 16 octaves, felt, two images, uv_offset over each kind
        it may wrap, checker over noise and image, checker of solids."""
        z = [self.t_noise(self.rng.uniform(1, 6)), self.t_noodle(0), self.t_noodle(1), self.t_noodle(16), self.t_felt(),
             self.t_image(7, 5), self.t_image(4, 9)]
        noise, noodle, felt, image = z[0], z[2], z[4], z[6]
        solid = self.t_solid()
        z += [self.t_uvoff(b, self.rng.uniform(-1.5, 1.5), self.rng.uniform(-0.4, 0.4)) for b in (image, solid, noise, noodle, felt)]
        z += [self.t_checker(noise, image, self.rng.uniform(0.2, 0.8)), self.t_checker(self.t_solid(), self.t_solid(), self.rng.uniform(0.2, 0.8)),
              self.t_checker(image, self.t_solid(), self.rng.uniform(0.2, 0.8))]
        return z

    # ---- materials
    def _mat(self, kind, tex=-1, fuzz=0.0, ior=0.0, albedo=(0, 0, 0)):
        m = np.zeros((), art.MATERIAL_DTYPE)
        m["kind"], m["tex"], m["fuzz"], m["ior"], m["albedo"] = kind, tex, fuzz, ior, albedo
        self.mat.append(m)
        return len(self.mat) - 1

    def lambertian(self, tex=-1): return self._mat(LAMBERTIAN, tex, albedo=self.colour())
    def metal(self, fuzz): return self._mat(METAL, fuzz=fuzz, albedo=self.colour(0.5, 1.0))
    def dielectric(self, ior): return self._mat(DIELECTRIC, ior=ior)
    def light(self): return self._mat(LIGHT, albedo=self.rng.uniform(2, 6, 3))
    def isotropic(self, tex=-1): return self._mat(ISOTROPIC, tex, albedo=self.colour(0.3, 1.0))

    def surface(self, k, tex_pool=()):
        """The k-th of a cycle through all four surface materials: fuzz 0 and 1, ior 0.67, 1.0, 1.5 and 2.4, a light."""
        k %= 12
        if k in (0, 3, 6, 9, 10):
            return self.lambertian(tex_pool[int(self.rng.integers(len(tex_pool)))] if len(tex_pool) else -1)
        if k in (1, 7):
            return self.metal(0.0 if k == 1 else 1.0)
        if k == 4:
            return self.metal(self.rng.uniform(0, 1))
        if k == 11:
            return self.light()
        return self.dielectric((0.67, 1.0, 1.5, 2.4)[int(self.rng.integers(4))] if k != 2 else 1.5)

    # ---- primitives: each returns (prim ref, lo, hi) with the box in float64
    def sphere(self, c, r, mat, vel=(0, 0, 0)):
        s = np.zeros((), art.SPHERE_DTYPE)
        s["c0"], s["radius"], s["vel"], s["mat"] = c, r, vel, mat
        self.sph.append(s)
        c0, v, rr = s["c0"].astype(np.float64), s["vel"].astype(np.float64), abs(float(s["radius"]))
        self.contents.add("sphere_tests")
        return ref(SPHERE, len(self.sph) - 1), np.minimum(c0, c0 + v) - rr, np.maximum(c0, c0 + v) + rr

    def quad(self, Q, u, v, mat, flip=False):
        Q, u, v = (np.asarray(x, np.float32).astype(np.float64) for x in (Q, u, v))
        n = np.cross(u, v)
        unit = n / np.linalg.norm(n) * (-1.0 if flip else 1.0)
        q = np.zeros((), art.QUAD_DTYPE)
        q["Q"], q["u"], q["v"], q["mat"] = Q, u, v, mat
        q["n"], q["D"], q["w"] = unit, float(unit @ Q), n / float(n @ n)
        self.qd.append(q)
        pts = np.stack([Q, Q + u, Q + v, Q + u + v])
        self.contents.add("quad_tests")
        return ref(QUAD, len(self.qd) - 1), pts.min(0) - 1e-3, pts.max(0) + 1e-3

    def box(self, a, b, mat, order=(0, 1, 2, 3, 4, 5)):
        """Six quads; order (0..5) = the reference's make_box order (quad.cuh:145-162), any other permutation is as legal."""
        a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
        mn, mx = np.minimum(a, b), np.maximum(a, b)
        dx, dy, dz = np.array([mx[0] - mn[0], 0, 0]), np.array([0, mx[1] - mn[1], 0]), np.array([0, 0, mx[2] - mn[2]])
        faces = [((mn[0], mn[1], mx[2]), dx, dy), ((mx[0], mn[1], mx[2]), -dz, dy), ((mx[0], mn[1], mn[2]), -dx, dy),
                 ((mn[0], mn[1], mn[2]), dz, dy), ((mn[0], mx[1], mx[2]), dx, -dz), ((mn[0], mn[1], mn[2]), dx, dz)]
        first = len(self.qd)
        mats = mat if isinstance(mat, (list, tuple)) else [mat] * 6
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for k in order:
            _, l, h = self.quad(*faces[k], mats[k])
            lo, hi = np.minimum(lo, l), np.maximum(hi, h)
        b_ = np.zeros((), BOX_DTYPE)
        b_["first_quad"] = first
        self.bx.append(b_)
        self.contents.add("box6_calls")
        return ref(BOX, len(self.bx) - 1), lo, hi

    def instance(self, child, flags, deg=0.0, offset=(0, 0, 0)):
        """translate(rotate_y(child)): a point of the child goes to (c x + s z, y, c z - s x) + offset (hittable.cuh:118-145)."""
        cref, lo, hi = child
        i = np.zeros((), art.INSTANCE_DTYPE)
        i["sin_t"], i["cos_t"] = math.sin(math.radians(deg)), math.cos(math.radians(deg))
        i["offset"], i["child"], i["flags"] = offset, cref, flags
        self.ins.append(i)
        s, c, off = float(i["sin_t"]), float(i["cos_t"]), i["offset"].astype(np.float64)
        if flags & ROTATE_Y:
            xs = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
            w = np.stack([c * xs[:, 0] + s * xs[:, 2], xs[:, 1], c * xs[:, 2] - s * xs[:, 0]], 1)
            lo, hi = w.min(0) - 1e-5, w.max(0) + 1e-5
        if flags & TRANSLATE:
            lo, hi = lo + off, hi + off
        self.contents.add("inst_calls")
        return ref(INSTANCE, len(self.ins) - 1), lo, hi

    def medium(self, boundary, density, mat):
        bref, lo, hi = boundary
        m = np.zeros((), art.MEDIUM_DTYPE)
        m["boundary"], m["neg_inv_density"], m["mat"] = bref, -1.0 / density, mat
        self.med.append(m)
        self.contents.add("medium_calls")
        return ref(MEDIUM, len(self.med) - 1), lo, hi

    def leaf(self, obj):
        r, lo, hi = obj
        self.leaves.append((r, _down(lo), _up(hi)))

    # ---- tree
    def _tree(self, a, b, out):
        """Leaves [a, b) in list order as a pre-order subtree; returns its box."""
        i = len(out)
        out.append(None)
        if b - a == 1:
            r, lo, hi = self.leaves[a]
        else:
            mid = a + 1 + int(self.rng.integers(b - a - 1))          # anywhere, not the median
            lo1, hi1 = self._tree(a, mid, out)
            lo2, hi2 = self._tree(mid, b, out)
            r, lo, hi = -1, np.minimum(lo1, lo2), np.maximum(hi1, hi2)
        out[i] = (lo, len(out), hi, r)
        return lo, hi

    def finish(self, name, camera, nx, ny, ns=4, gamma=2.2, background=(0, 0, 0), gradient=1):
        flat = []
        if self.leaves:
            self._tree(0, len(self.leaves), flat)
        nodes = np.zeros(len(flat), art.NODE_DTYPE)
        for k, (lo, skip, hi, r) in enumerate(flat):
            nodes[k] = (lo, skip, hi, r)

        def arr(items, dtype):
            return np.array(items, dtype) if items else np.zeros(0, dtype)
        arrays = {"nodes": nodes, "spheres": arr(self.sph, art.SPHERE_DTYPE), "quads": arr(self.qd, art.QUAD_DTYPE),
                  "boxes": arr(self.bx, BOX_DTYPE), "instances": arr(self.ins, art.INSTANCE_DTYPE), "media": arr(self.med, art.MEDIUM_DTYPE),
                  "materials": arr(self.mat, art.MATERIAL_DTYPE), "textures": arr(self.tex, TEXTURE_DTYPE),
                  "images": np.ascontiguousarray(self.images)}
        return GenScene(name, arrays, camera, nx, ny, ns, gamma, background, gradient, self.contents)


# ------------------------------------------------------------------------------------------------------------ recipes
def _cells(rng, n, x0=-4.0, x1=4.0, z0=-4.5, z1=3.0):
    """n jittered positions on the ground plane, one per cell of a grid just large enough, and the cell size."""
    cols = max(1, math.ceil(math.sqrt(n * (x1 - x0) / (z1 - z0))))
    rows = max(1, math.ceil(n / cols))
    cell = min((x1 - x0) / cols, (z1 - z0) / rows)
    pick = rng.permutation(cols * rows)[:n]
    xs = x0 + (pick % cols + 0.5) * (x1 - x0) / cols + rng.uniform(-0.15, 0.15, n) * cell
    zs = z0 + (pick // cols + 0.5) * (z1 - z0) / rows + rng.uniform(-0.15, 0.15, n) * cell
    return xs, zs, cell


def _camera(rng, nx, ny, lens=True, shutter=None):
    if shutter is None:
        shutter = (0.25, 0.75) if rng.integers(2) else (0.0, 0.0)
    eye = (rng.uniform(-1, 1), rng.uniform(1.8, 2.6), rng.uniform(8.5, 10))
    return make_camera(eye, (0, 0.4, 0), 40.0, nx / ny, 0.1 if lens else 0.0, 9.0, *shutter)


def _ground(b, tex=-1):
    return b.sphere((0, -200, 0), 200.0, b.lambertian(tex))


def _spheres(b, n, tex_pool=(), ground_tex=-1):
    """A ground sphere and n - 1 small ones, static and moving, every surface material; among them a glass sphere with a
    negative-radius shell inside (two leaves)."""
    rng = b.rng
    b.leaf(_ground(b, ground_tex))
    if n <= 1:
        return
    xs, zs, cell = _cells(rng, n - 1)
    k = 0
    while k < n - 1:
        r = float(rng.uniform(0.3, 0.42) * cell)
        c = (xs[k], r, zs[k])
        if k == 0 and n - 1 >= 2:                               # the shell: same centre as its glass sphere, one cell over is unused
            glass = b.dielectric(1.5)
            b.leaf(b.sphere(c, r, glass))
            b.leaf(b.sphere(c, -0.8 * r, glass))
            k += 2
            continue
        vel = (0, rng.uniform(0.1, 0.5) * cell, 0) if rng.integers(3) == 0 else (0, 0, 0)
        b.leaf(b.sphere(c, r, b.surface(k + int(rng.integers(2)), tex_pool), vel))
        k += 1


def _spheres_recipe(name, rng, nx, ny, level):
    b = Builder(rng)
    n = int(rng.integers(3, 201 if level < 2 else 181))          # (level 2 adds one sphere per texture)
    pool, ground = (), -1
    if level == 1:
        pool = [b.t_checker(b.t_solid(), b.t_solid(), rng.uniform(0.2, 1.0)) for _ in range(3)]
        ground = pool[0]
    elif level == 2:
        pool = b.texture_zoo()
        ground = pool[-3]                                        # checker over noise and image
    _spheres(b, n, pool, ground)
    if level == 2:                                               # every texture of the zoo is on some sphere
        for k, t in enumerate(pool):
            b.leaf(b.sphere((-3.5 + 0.55 * k, 0.25, 3.6), 0.25, b.lambertian(t)))
    return b.finish(name, _camera(rng, nx, ny), nx, ny, gradient=int(rng.integers(4) != 0), background=(0.3, 0.35, 0.5))


def _general(name, rng, nx, ny, tex, with_checker):
    b = Builder(rng)
    pool = b.texture_zoo() if tex else ([b.t_checker(b.t_solid(), b.t_solid(), rng.uniform(0.3, 1.0)) for _ in range(2)] if with_checker else [])
    pick = (lambda: pool[int(rng.integers(len(pool)))]) if pool else (lambda: -1)
    b.leaf(_ground(b, pick()))
    n = int(rng.integers(20, 41))
    xs, zs, cell = _cells(rng, n, z0=-4.0, z1=2.5)
    s = 0.4 * cell
    shared_box = b.box((-s, 0, -s), (s, 1.6 * s, s), [b.lambertian(pick()) for _ in range(6)])       # in object space, under several instances
    shared_sphere = b.sphere((0, s, 0), s, b.lambertian(pick()))
    moving = b.sphere((0, s, 0), 0.8 * s, b.metal(0.2), vel=(0, 0.5 * s, 0))
    glass_mat = b.dielectric(1.5)
    glass, shell = b.sphere((0, s, 0), s, glass_mat), b.sphere((0, s, 0), -0.85 * s, glass_mat)
    flat = b.quad((-s, 0, 0), (2 * s, 0, 0), (0, 2 * s, 0), b.lambertian(pick()))
    for k in range(n):
        x, z, kind = float(xs[k]), float(zs[k]), k % 10
        deg, off = float(rng.uniform(-180, 180)), (x, 0, z)
        if kind == 0:
            b.leaf(b.sphere((x, s, z), s, b.surface(k // 10 + int(rng.integers(12))), (0, 0.3 * s, 0) if rng.integers(2) else (0, 0, 0)))
        elif kind == 1:                                          # an upright quad, oblique to every axis, either facing
            a = rng.uniform(0, math.pi)
            b.leaf(b.quad((x - s * math.cos(a), 0, z - s * math.sin(a)), (2 * s * math.cos(a), 0.2 * s, 2 * s * math.sin(a)), (0, 2 * s, 0),
                          b.surface(int(rng.integers(12)), pool), flip=bool(rng.integers(2))))
        elif kind == 2:                                          # axis-aligned boxes: the reference's face order, and another
            order = (0, 1, 2, 3, 4, 5) if rng.integers(2) else tuple(rng.permutation(6))
            b.leaf(b.box((x - s, 0, z - s), (x + s, rng.uniform(0.5, 2) * s, z + s), b.lambertian(pick()), order))
        elif kind == 3:
            b.leaf(b.instance(shared_box, ROTATE_Y | TRANSLATE, deg, off))
        elif kind == 4:
            b.leaf(b.instance(shared_sphere if k % 20 == 4 else moving, TRANSLATE, 0.0, off))
        elif kind == 5:                                          # rotation alone: about the world's y axis, the child sits away from it
            r0 = math.hypot(x, z)
            child = b.box((r0 - s, 0, -s), (r0 + s, 1.2 * s, s), b.metal(0.0)) if k % 20 == 5 else b.sphere((r0, s, 0), s, b.lambertian(pick()))
            b.leaf(b.instance(child, ROTATE_Y, math.degrees(math.atan2(-z, x))))
        elif kind == 6:
            b.leaf(b.instance(flat, ROTATE_Y | TRANSLATE, deg, off))
        elif kind == 7:                                          # a glass sphere and its negative-radius shell under one transform
            b.leaf(b.instance(glass, ROTATE_Y | TRANSLATE, deg, off))
            b.leaf(b.instance(shell, ROTATE_Y | TRANSLATE, deg, off))
        elif kind == 8:                                          # a light: a quad facing down, or a sphere
            if rng.integers(2):
                b.leaf(b.quad((x - s, 2.5, z - s), (2 * s, 0, 0), (0, 0, 2 * s), b.light()))
            else:
                b.leaf(b.sphere((x, 2.5, z), 0.6 * s, b.light()))
        else:                                                    # a horizontal axis-aligned quad just above the ground
            b.leaf(b.quad((x - s, 0.05, z - s), (2 * s, 0, 0), (0, 0, 2 * s), b.lambertian(pick())))
    return b, pool, pick


def _boundary(b, kind, at, size, rng):
    """A medium's boundary of every kind the ABI allows, around `at`."""
    x, y, z = at
    if kind == 0:
        return b.sphere(at, size, 0)
    if kind == 1:                                                # a negative-radius sphere encloses the same volume
        return b.sphere(at, -size, 0)
    if kind == 2:
        return b.box((x - size, y - size, z - size), (x + size, y + size, z + size), 0)
    if kind == 3:                                                # a single quad encloses nothing: legal, and never scatters
        return b.quad((x - size, y - size, z), (2 * size, 0, 0), (0, 2 * size, 0), 0)
    if kind == 4:
        return b.instance(b.box((-size, -size, -size), (size, size, size), 0), ROTATE_Y | TRANSLATE, float(rng.uniform(0, 90)), at)
    return b.instance(b.sphere((0, 0, 0), size, 0, vel=(0, 0.4 * size, 0)), TRANSLATE, 0.0, at)


# general_plain / general_tex: the media of seed k are GENERAL_MEDIA[k % 6], as kinds of _boundary -- fixed by the seed, not
# drawn, so that the seed list provably holds 0, 1 and 2 media and every boundary kind: sphere (0), negative-radius sphere (1),
# box (2), quad (3), instance of a box (4), instance of a moving sphere (5)
GENERAL_MEDIA = [(2, 0), (0, 3), (2,), (), (1, 4), (5,)]


def _general_recipe(name, rng, nx, ny, tex, seed):
    b, pool, pick = _general(name, rng, nx, ny, tex, with_checker=bool(seed % 2))
    for kind in GENERAL_MEDIA[seed % len(GENERAL_MEDIA)]:
        at = (float(rng.uniform(-2.5, 2.5)), 0.9, float(rng.uniform(-1, 3)))
        b.leaf(b.medium(_boundary(b, kind, at, float(rng.uniform(0.7, 1.1)), rng), float(rng.uniform(0.5, 3)), b.isotropic(pick())))
    return b.finish(name, _camera(rng, nx, ny, shutter=(0.25, 0.75)), nx, ny, gradient=int(rng.integers(4) != 0), background=(0.3, 0.35, 0.5))


def _media_many(name, rng, nx, ny):
    b = Builder(rng)
    _spheres(b, int(rng.integers(8, 30)))
    cam = _camera(rng, nx, ny, shutter=(0.25, 0.75))
    n_media = int(rng.integers(3, 6))
    eye = tuple(float(x) for x in cam.origin)
    b.leaf(b.medium(b.sphere(eye, 14.0, 0), 0.02, b.isotropic()))                      # the camera sits inside this one
    b.leaf(b.medium(_boundary(b, 5, (0.3, 0.9, 1.5), 1.0, rng), 1.5, b.isotropic()))   # an instance of a moving sphere
    for k in range(n_media - 2):                                                       # overlapping each other and the one above
        at = (float(rng.uniform(-1, 1.5)), 0.9, float(rng.uniform(0.5, 2.5)))
        b.leaf(b.medium(_boundary(b, (0, 2, 4)[k % 3], at, float(rng.uniform(0.8, 1.2)), rng), float(rng.uniform(0.5, 2)), b.isotropic()))
    return b.finish(name, cam, nx, ny, gradient=1)


def _limits(name, rng, nx, ny, seed):
    b = Builder(rng)
    count, with_quad = LIMIT_COUNTS[seed % len(LIMIT_COUNTS)], seed >= len(LIMIT_COUNTS)
    b.leaf(_ground(b))
    if count > 1:
        xs, zs, cell = _cells(rng, count - 1, x0=-3.5, x1=3.5, z0=-3.0, z1=3.0)
        for k in range(count - 1):
            r = float(rng.uniform(0.3, 0.42) * min(cell, 2.0))
            if with_quad and k == 0:
                b.leaf(b.quad((xs[k] - r, 0, zs[k]), (2 * r, 0, 0), (0, 2 * r, 0), b.lambertian()))
            else:
                b.leaf(b.sphere((xs[k], r, zs[k]), r, b.surface(k), (0, 0.3 * r, 0) if k % 4 == 1 else (0, 0, 0)))
    elif with_quad:                                              # one leaf, and it is the quad: a floor
        b.leaves.clear(); b.sph.clear(); b.contents.clear()
        b.leaf(b.quad((-30, 0, -30), (60, 0, 0), (0, 0, 60), 0))
    return b.finish(name, _camera(rng, nx, ny, lens=False, shutter=(0.0, 1.0)), nx, ny, gradient=1)


def tiny(nx: int = 48, ny: int = 32) -> GenScene:
    """Three sphere leaves, three instances (each of a quad of its own) and a free quad: three spheres, three instances, four quads."""
    rng = np.random.default_rng(0)
    b = Builder(rng)
    mat = b.lambertian()
    for k in range(3):
        b.leaf(b.sphere((k - 1.0, 0.4, 0.0), 0.4, mat))
    for k in range(3):
        child = b.quad((-0.3, 0, 0), (0.6 + 0.1 * k, 0, 0), (0, 0.6, 0), mat)
        b.leaf(b.instance(child, ROTATE_Y | TRANSLATE, 20.0 * k, (k - 1.0, 0, 1.5)))
    b.leaf(b.quad((-2, 0.05, -2), (4, 0, 0), (0, 0, 4), mat))
    return b.finish("tiny", _camera(rng, nx, ny), nx, ny)


def generate(recipe: str, seed: int, nx: int = 48, ny: int = 32) -> GenScene:
    rng = np.random.default_rng([RECIPES.index(recipe), seed])
    name = f"{recipe}/{seed}"
    if recipe == "spheres_plain":
        return _spheres_recipe(name, rng, nx, ny, 0)
    if recipe == "spheres_checker":
        return _spheres_recipe(name, rng, nx, ny, 1)
    if recipe == "spheres_tex":
        return _spheres_recipe(name, rng, nx, ny, 2)
    if recipe == "general_plain":
        return _general_recipe(name, rng, nx, ny, False, seed)
    if recipe == "general_tex":
        return _general_recipe(name, rng, nx, ny, True, seed)
    if recipe == "media_many":
        return _media_many(name, rng, nx, ny)
    if recipe == "limits":
        return _limits(name, rng, nx, ny, seed)
    raise ValueError(recipe)
