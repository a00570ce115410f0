"""What rt_radiance_rays must return, predicted with the CPU oracle exactly as it is (include/rt_abi.h, "radiance queries").

A radiance query is a pixel of a degenerate camera: with horizontal = vertical = 0, lens_radius = 0, origin = o,
lower_left_corner = p and time0 = time1 = tm, camera_get_ray returns the ray (o, fl(p - o), tm) for every sample whatever
its jitter, lens and shutter draws were; a 1 x 1 frame of that camera at seed_base = s and gamma 1 is the radiance along that
ray for the chain seeded s.  So the expectation of a query is one oracle scene (the description with that camera) rendered
1 x 1, and the device is handed d = fl(p - o).

Oracle scenes are never freed and each copies the image pool: a RayOracle builds one scene per ray and renders it for every
(seeds, ns) asked of it; callers keep rays x image_bytes under 256 MB per test.

Also here, shared by the host and the GPU tests: the scenes and ray sets of the parity test, so that the conditions that
keep them from testing nothing (tests/test_radiance_host.py) are checked on the very sets the GPU test uses.
"""
from __future__ import annotations

import numpy as np

import scene_gen as sg
from test_desc_oracle import ONE_SEED

NX, NY = 48, 32
# (scene, queries): the seven recipes of scene_gen at ONE_SEED, moving spheres, a medium in a box of quads, the Book-2 scene
PARITY = [(f"{r}/{ONE_SEED[r]}", 2048) for r in sg.RECIPES] + [("bouncing", 2048), ("cornell_smoke", 1024), ("final", 96)]
# the batch that outgrows the resident lanes is tiled from this set
LARGE = ("spheres_plain/1", 4096)


def load_scene(art, key):
    """A generated scene ("recipe/seed") or a named one: anything with HostScene's surface."""
    if "/" in key:
        recipe, seed = key.split("/")
        return sg.generate(recipe, int(seed), NX, NY)
    img, iw, ih = art.default_texture(key)
    return art.HostScene(key, NX, NY, img, iw, ih)


def directions(o, p):
    """What the device is given for the query (o, p): p - o in float32."""
    return np.ascontiguousarray(np.asarray(p, np.float32) - np.asarray(o, np.float32), np.float32)


def degenerate_desc(scene, o, p, tm):
    """A copy of the scene's description whose camera sends every sample along (o, fl(p - o), tm)."""
    import accelerated_ray_tracer_amd as art
    d = art.RtSceneDesc.from_buffer_copy(scene.desc)
    c = d.camera
    c.origin[:] = [float(x) for x in o]
    c.lower_left_corner[:] = [float(x) for x in p]
    for field in (c.horizontal, c.vertical, c.u, c.v):
        field[:] = [0.0, 0.0, 0.0]
    c.lens_radius = 0.0
    c.time0 = c.time1 = float(tm)
    return d


class RayOracle:
    """One oracle scene per query (o[i], p[i], tm[i]); expect(seeds, ns) renders each 1 x 1."""

    def __init__(self, orc, scene, o, p, tm, background, gradient):
        o, p = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(p, np.float32).reshape(-1, 3)
        tm = np.zeros(len(o), np.float32) if tm is None else np.asarray(tm, np.float32).reshape(len(o))
        self.n = len(o)
        self.scenes = [orc.OracleScene.from_desc(degenerate_desc(scene, o[i], p[i], tm[i]), 1, 1, 1.0, background, int(gradient))
                       for i in range(self.n)]

    def expect(self, seeds, ns):
        rgb, rays = np.zeros((self.n, 3), np.float32), np.zeros(self.n, np.int64)
        for i, s in enumerate(self.scenes):
            fb, cnt = s.render(ns, gamma=1.0, seed_base=int(seeds[i]), threads=1)
            rgb[i], rays[i] = fb[0, 0], cnt["rays"]
        return rgb, rays


def expect(orc, scene, o, p, tm, seeds, ns, background, gradient):
    """(rgb, rays) of the queries (o, p, tm) with the chains seeded `seeds`, ns samples each."""
    return RayOracle(orc, scene, o, p, tm, background, gradient).expect(seeds, ns)


def default_seeds(n, seed_base=1984):
    return (np.uint64(seed_base) + np.arange(n, dtype=np.uint64)).astype(np.uint64)


def explicit_seeds(n, salt=0):
    return np.random.default_rng(977 + salt).integers(0, 1 << 64, n, dtype=np.uint64)


def ray_set(scene, whole, n):
    """n queries (o, p, tm) of `scene` (whole = its oracle, OracleScene.from_host), in thirds: camera rays through random
    points of the image plane; rays between random points of the box around the small leaves (as _query_rays of
    tests/test_desc_parity.py; the root box where the scene has no small leaf); rays that leave the oracle's hit points of
    the first third along random directions.  Times lie inside the shutter."""
    rng = np.random.default_rng(len(scene.name) + 7 * n + 13 * scene.desc.n_nodes)
    cam = scene.desc.camera
    v = lambda a: np.array(list(a), np.float32)   # noqa: E731
    k = n // 3
    tm = (cam.time0 + rng.random(n) * (cam.time1 - cam.time0)).astype(np.float32)
    s, t = rng.random((2, k, 1), dtype=np.float32)
    o1 = np.ascontiguousarray(np.broadcast_to(v(cam.origin), (k, 3)))
    p1 = (v(cam.lower_left_corner) + s * v(cam.horizontal) + t * v(cam.vertical)).astype(np.float32)
    nodes = scene.nodes()
    small = nodes[(nodes["prim"] >= 0) & ((nodes["bmax"] - nodes["bmin"]).max(1) < 100)]
    if len(small) == 0:
        small = nodes[:1]
    lo, hi = small["bmin"].min(0), small["bmax"].max(0)
    o2 = (lo + rng.random((k, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    p2 = (lo + rng.random((k, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    t1, hp = whole.trace(o1, directions(o1, p1), tm[:k])[:2]
    hit = np.flatnonzero(t1 < np.finfo(np.float32).max)
    assert len(hit) > 0, "no camera ray hits anything"
    m = n - 2 * k
    o3 = hp[hit[np.arange(m) % len(hit)]].astype(np.float32)
    w = rng.normal(size=(m, 3)).astype(np.float32)
    p3 = (o3 + w).astype(np.float32)
    o, p = np.ascontiguousarray(np.concatenate([o1, o2, o3])), np.ascontiguousarray(np.concatenate([p1, p2, p3]))
    d = directions(o, p)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(1).all()
    return o, p, tm


class Case:
    """A parity scene, its oracle, its ray set and the per-ray oracle; expectations cached by (seed kind, ns)."""

    def __init__(self, art, orc, key, n):
        self.key, self.n = key, n
        self.scene = load_scene(art, key)
        self.whole = orc.OracleScene.from_host(self.scene)
        self.o, self.p, self.tm = ray_set(self.scene, self.whole, n)
        self.d = directions(self.o, self.p)
        self.background, self.gradient = self.scene.background, self.scene.use_gradient_bg
        self._orc, self._rays, self._cache = orc, None, {}

    def seeds(self, kind):
        return default_seeds(self.n) if kind == "default" else explicit_seeds(self.n, len(self.key))

    def expect(self, kind, ns):
        if self._rays is None:
            self._rays = RayOracle(self._orc, self.scene, self.o, self.p, self.tm, self.background, self.gradient)
        if (kind, ns) not in self._cache:
            self._cache[(kind, ns)] = self._rays.expect(self.seeds(kind), ns)
        return self._cache[(kind, ns)]
