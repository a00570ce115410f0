"""What rt_render_aov must return, predicted with the CPU oracle exactly as it is (include/rt_abi.h, "feature buffers").

The emissive twin of a description is the same description with every material turned into a diffuse light: lambertian,
isotropic and light keep tex and albedo, metal takes tex = -1, dielectric tex = -1 and albedo = (1, 1, 1).  In the twin every
path ends at its first hit -- a light emits and does not scatter, a miss ends the path -- and consumes no draw, so the twin's
chain is the feature pass's chain: per sample two jitter uniforms, the lens-disk loop, the shutter uniform.  Hence

  * albedo is the oracle's render of the twin at gamma 1 (same ns, seed, background, gradient);
  * the oracle's ray sample of the twin (trace_families.ray_sample, seed 1984) is the pass's primary rays in (row, column,
    sample) order, and OracleScene.trace on them against the ORIGINAL scene gives every sample's t, normal and material;
    summed in float32 in sample order and scaled by (float)(1.0 / (double)(float)ns) they are depth, normal and alpha, and
    sample 0's material is mat.

Also here, shared by the host and the GPU tests: the scenes of the parity test, so that the conditions that keep them from
testing nothing (tests/test_aov_host.py) are checked on the very scenes and frames the GPU test uses.
"""
from __future__ import annotations

import numpy as np

import scene_gen as sg
import trace_families as tf
from test_desc_oracle import ONE_SEED

NX, NY = 48, 32
SEED = 1984                      # orc_ray_sample's fixed seed: every oracle expectation is for seed_base = SEED
FLT_MAX = np.float32(np.finfo(np.float32).max)
# the seven recipes of scene_gen at ONE_SEED, moving spheres behind a shutter, a medium in a box of quads, the Book-2 scene
PARITY = [f"{r}/{ONE_SEED[r]}" for r in sg.RECIPES] + ["bouncing", "cornell_smoke", "final"]
SPHERES, GENERAL = PARITY[2], PARITY[4]          # spheres_tex and general_tex: texture level 2 in both kernel families


def load_scene(art, key):
    """A generated scene ("recipe/seed") or a named one, with the camera of an NX x NY frame."""
    if "/" in key:
        recipe, seed = key.split("/")
        return sg.generate(recipe, int(seed), NX, NY)
    img, iw, ih = art.default_texture(key)
    return art.HostScene(key, NX, NY, img, iw, ih)


def twin_materials(mats):
    """The twin's material array (MATERIAL_DTYPE) of `mats`."""
    out = mats.copy()
    out["kind"] = sg.LIGHT
    out["tex"][mats["kind"] == sg.METAL] = -1
    glass = mats["kind"] == sg.DIELECTRIC
    out["tex"][glass] = -1
    out["albedo"][glass] = 1.0
    return out


class Twin:
    """The emissive twin of anything with HostScene's surface (a HostScene or a scene_gen.GenScene): a copy of the description
    whose materials point at the twin's array; every other array is the original's, which is kept alive here."""

    def __init__(self, art, scene):
        self.original = scene
        self.name = getattr(scene, "name", "desc") + "/twin"
        self._materials = twin_materials(scene.materials())
        self.desc = art.RtSceneDesc.from_buffer_copy(scene.desc)
        self.desc.materials = self._materials.ctypes.data if len(self._materials) else None
        self.nx, self.ny, self.ns, self.gamma = scene.nx, scene.ny, scene.ns, scene.gamma
        self.background, self.use_gradient_bg = scene.background, scene.use_gradient_bg
        self.frame = lambda **kw: art.HostScene.frame(self, **kw)

    def materials(self):
        return self._materials.copy()

    def close(self):
        pass


def scale(ns):
    """store_pixel's factor."""
    return np.float32(1.0 / np.float64(np.float32(ns)))


def _sum_samples(x, ns):
    """x: (ny, nx, ns, ...) float32 -> the sum over the samples in sample order in float32, scaled."""
    acc = np.zeros(x.shape[:2] + x.shape[3:], np.float32)
    for s in range(ns):
        acc = (acc + x[:, :, s]).astype(np.float32)
    return (acc * scale(ns)).astype(np.float32)


def expected(orc, scene, nx, ny, ns, art=None, whole=None, twin=None):
    """albedo / normal / depth / alpha / mat of the whole nx x ny frame of `scene` at ns samples and seed_base SEED, from the
    oracle; also "rays" (the (ny * nx * ns, 8) primary rays), "t" and "mats" (per sample, (ny, nx, ns)) and the twin render's
    counters.  whole / twin: the oracle of the scene and the Twin, when the caller keeps them."""
    if twin is None:
        import accelerated_ray_tracer_amd
        twin = Twin(art or accelerated_ray_tracer_amd, scene)
    if whole is None:
        whole = orc.OracleScene.from_host(scene, nx, ny)
    lit = orc.OracleScene.from_desc(twin.desc, nx, ny, 1.0, scene.background, scene.use_gradient_bg, twin.name)
    albedo, counters = lit.render(ns, gamma=1.0, seed_base=SEED)
    rays = tf.ray_sample(orc, lit, nx, ny, ns)
    assert len(rays) == nx * ny * ns, (len(rays), nx * ny * ns)
    t, _, n, _, mat = whole.trace(rays[:, 0:3], rays[:, 3:6], rays[:, 6])
    hit = t < FLT_MAX
    shape = (ny, nx, ns)
    depth = np.where(hit, t, np.float32(0)).astype(np.float32).reshape(shape)
    normal = np.where(hit[:, None], n, np.float32(0)).astype(np.float32).reshape(shape + (3,))
    mats = np.where(hit, mat, -1).astype(np.int32).reshape(shape)
    return {"albedo": albedo, "normal": _sum_samples(normal, ns), "depth": _sum_samples(depth, ns),
            "alpha": _sum_samples(hit.astype(np.float32).reshape(shape), ns), "mat": mats[:, :, 0].copy(),
            "rays": rays, "t": np.where(hit, t, FLT_MAX).reshape(shape), "twin_t": rays[:, 7].reshape(shape), "mats": mats,
            "counters": counters}


class Case:
    """A parity scene, its twin and its oracle; expectations cached by frame and sample count, left unchanged."""

    def __init__(self, art, orc, key):
        self.key = key
        self.scene = load_scene(art, key)
        self.twin = Twin(art, self.scene)
        self._art, self._orc, self._cache = art, orc, {}

    def expect(self, ns, nx=NX, ny=NY):
        k = (nx, ny, ns)
        if k not in self._cache:
            whole = self._orc.OracleScene.from_host(self.scene, nx, ny)
            self._cache[k] = expected(self._orc, self.scene, nx, ny, ns, self._art, whole, self.twin)
        return self._cache[k]
